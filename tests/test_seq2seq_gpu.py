"""GPU: the cross-attention decode kernel and the memory fill (csrc/attention_cross_decode.hip) against the float64 restatement of
tests/seq2seq_ref.py, and the model of examples/seq2seq.py -- one training step, the reference-written checkpoint and the three
translation modes -- against the reference's fixture (tests/golden/seq2seq_tiny*).

Bounds.  Kernel: assert_close_scaled(tol=1e-4) on O (1e-4 of max(|entry|, the tensor's rms)), atol 1e-6 + rtol 1e-4 on the
probabilities, rows of P sum to 1 within 1e-5.  Training step: the bounds of test_gpt_tiny_step_golden (tests/test_hip_parity.py)."""
import os
import pickle
import sys

import numpy as np
import pytest

import seq2seq_ref as R
from conftest import GOLDEN, ROOT
from lstm_abi import Fenced, dev
from test_hip_parity import assert_close_scaled, grad_list_scale

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
PAD, SOS, EOS = 0, 1, 2
KPI = {32: 128, 64: 64, 128: 64}            # keys per block iteration of attn_cross_decode_kernel<dh> (attention_decode.h: DecLanes::KPI)
B_, H_ = 3, 2


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def host(t):
    return t.detach().cpu().numpy()


def example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import seq2seq
    return seq2seq


def idev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


# ------------------------------------------------------------------------------------------- nnhipAttentionDecodeCross
def cross_call(q, km, vm, kv, O, P, B, H, S, dh, ld_q, scale):
    from neunet_hip._lib import StridedView, call_hip_function, get_current_stream_ptr
    call_hip_function("nnhipAttentionDecodeCross", StridedView(q), km, vm, kv, O, P, B, H, S, dh, ld_q, float(scale),
                      get_current_stream_ptr())


def run_cross(Q, K, V, valid, scale, want_P=True, column_block=False):
    """One call with O and P inside guarded buffers.  Returns (O, P or None) as host arrays after checking the guards and that the
    memory was only read."""
    import torch
    B, H, S, dh = K.shape
    D = H * dh
    km, vm = dev(K), dev(V)
    km0, vm0 = km.clone(), vm.clone()
    if column_block:
        wide = torch.full((B, 3 * D), float("nan"), dtype=torch.float32, device="cuda")
        wide[:, D:2 * D] = dev(Q)
        q, ld_q = wide[:, D:2 * D], 3 * D
    else:
        q, ld_q = dev(Q), D
    fo, fp = Fenced(B, D), Fenced(B, H, S) if want_P else None
    cross_call(q, km, vm, None if valid is None else idev(valid), fo.view, fp.view if want_P else None, B, H, S, dh, ld_q, scale)
    torch.cuda.synchronize()
    assert fo.guards_intact() and (fp is None or fp.guards_intact()), "a guard word was overwritten"
    assert torch.equal(km, km0) and torch.equal(vm, vm0), "the memory was written"
    return fo.host(), fp.host() if want_P else None


def valid_cases(S, rng):
    """NULL, per-row prefixes of different length, a hole in the middle, one fully masked row (with a prefix row and a full row)."""
    prefix = np.zeros((B_, S), np.int32)
    for b, n in enumerate((max(1, S // 3), max(1, (2 * S) // 3), S)):
        prefix[b, :n] = 1
    hole = np.ones((B_, S), np.int32)
    hole[0, S // 3:max(S // 3 + 1, (2 * S) // 3)] = 0
    hole[1, rng.random(S) < 0.3] = 0
    hole[1, 0] = 1
    dark = np.ones((B_, S), np.int32)
    dark[1] = 0
    if S > 1:
        dark[2, S // 2:] = 0
    return {"null": None, "prefix": prefix, "hole": hole, "dark_row": dark}


def check_cross(O, P, Q, K, V, valid, scale, tag):
    Oref, Pref = R.cross_decode_ref(Q, K, V, valid, scale)
    assert_close_scaled(O, Oref, tol=1e-4, err_msg=f"{tag}: O")
    if P is not None:
        np.testing.assert_allclose(P, Pref, rtol=1e-4, atol=1e-6, err_msg=f"{tag}: P")
        np.testing.assert_allclose(P.astype(np.float64).sum(-1), 1.0, rtol=0, atol=1e-5, err_msg=f"{tag}: rows of P")
    return Oref, Pref


@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("S", ["1", "5", "kpi-1", "kpi", "kpi+1", "300", "1500"])
def test_cross_decode_vs_float64(hip, dh, S):
    S = {"kpi-1": KPI[dh] - 1, "kpi": KPI[dh], "kpi+1": KPI[dh] + 1}.get(S) or int(S)
    rng = np.random.default_rng(1000 * dh + S)
    D = H_ * dh
    Q = rng.standard_normal((B_, D)).astype(np.float32)
    K = rng.standard_normal((B_, H_, S, dh)).astype(np.float32)
    V = rng.standard_normal((B_, H_, S, dh)).astype(np.float32)
    scale = 1.0 / np.sqrt(D)                                    # the seq2seq block's scale: 1 / sqrt(d_model)
    for name, valid in valid_cases(S, rng).items():
        tag = f"dh {dh} S {S} {name}"
        O, P = run_cross(Q, K, V, valid, scale)
        _, Pref = check_cross(O, P, Q, K, V, valid, scale, tag)
        if valid is not None:
            assert np.all(P[np.broadcast_to((valid == 0)[:, None, :], P.shape) & (valid.sum(1) > 0)[:, None, None]] == 0.0), tag
        if name == "dark_row":                                  # every key masked: -1e9 each, so the plain average of all S values
            assert_close_scaled(O[1], V[1].astype(np.float64).mean(1).reshape(-1), tol=1e-4, err_msg=f"{tag}: mean of V")
            np.testing.assert_allclose(P[1], 1.0 / S, rtol=1e-4, atol=1e-6, err_msg=f"{tag}: P of the masked row")
        # P NULL vs given: the same O bits; a second run: the same bits; Q as a column block of a [B, 3D] buffer: the same bits
        O2, none = run_cross(Q, K, V, valid, scale, want_P=False)
        assert none is None
        np.testing.assert_array_equal(O2, O, err_msg=f"{tag}: O with P == NULL")
        O3, P3 = run_cross(Q, K, V, valid, scale, column_block=True)
        check_cross(O3, P3, Q, K, V, valid, scale, tag + " ld_q = 3D")
        np.testing.assert_array_equal(O3, O, err_msg=f"{tag}: rerun / column block O")
        np.testing.assert_array_equal(P3, P, err_msg=f"{tag}: rerun / column block P")


def test_cross_decode_large_scores_and_scale(hip):
    """Scores far from 0 (|scale q.k| ~ 30): the online softmax across slots and iterations must not lose the small terms' sum."""
    rng = np.random.default_rng(7)
    dh, S = 64, 200
    Q = (rng.standard_normal((B_, H_ * dh)) * 3).astype(np.float32)
    K = (rng.standard_normal((B_, H_, S, dh)) * 3).astype(np.float32)
    V = rng.standard_normal((B_, H_, S, dh)).astype(np.float32)
    K[:, :, S - 1] = K[:, :, 0]                                  # a tie between the first and the last key
    O, P = run_cross(Q, K, V, None, 0.4)
    check_cross(O, P, Q, K, V, None, 0.4, "large scores")


@pytest.mark.parametrize("dh", [32, 64, 128])
def test_cross_decode_map_equals_unfused_path(hip, dh):
    """P against the attention map of the GEMM + masked-softmax path with one query row (attention_forward, Tq = 1)."""
    import torch
    from neunet_hip.nn.experimental.attention import attention_forward
    rng = np.random.default_rng(dh)
    S, D = 37, H_ * dh
    Q = rng.standard_normal((B_, D)).astype(np.float32)
    Kt = rng.standard_normal((B_, S, D)).astype(np.float32)      # token-major, as the projections leave them
    Vt = rng.standard_normal((B_, S, D)).astype(np.float32)
    valid = np.ones((B_, S), np.int32)
    valid[0, 30:] = 0
    valid[1, 5:9] = 0
    valid[2] = 0
    divisor = float(np.sqrt(D))
    ctx, attn, _ = attention_forward(dev(Q).reshape(B_, 1, D), dev(Kt), dev(Vt), idev(valid), H_, divisor, False)
    torch.cuda.synchronize()
    K = Kt.reshape(B_, S, H_, dh).transpose(0, 2, 1, 3)
    V = Vt.reshape(B_, S, H_, dh).transpose(0, 2, 1, 3)
    O, P = run_cross(Q, K, V, valid, 1.0 / divisor)
    np.testing.assert_allclose(P, host(attn).reshape(B_, H_, S), **TOL)
    np.testing.assert_allclose(O, host(ctx).reshape(B_, D), **TOL)


def test_cross_decode_empty_batch(hip):
    from neunet_hip._lib import load_hip_function
    assert load_hip_function("nnhipAttentionDecodeCross")(None, None, None, None, None, None, 0, 2, 7, 32, 64, 0.1, None) == 0


# ------------------------------------------------------------------------------------------- nnhipKVMemoryFill
@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("fused_kv", [False, True])
def test_kv_memory_fill_is_a_permute(hip, dh, fused_kv):
    import torch
    from neunet_hip._lib import StridedView, call_hip_function, get_current_stream_ptr
    rng = np.random.default_rng(dh + fused_kv)
    B, H, S = 3, 3, 11
    D = H * dh
    if fused_kv:                                                 # the two column blocks of one K|V projection: ld = 2D
        kv = dev(rng.standard_normal((B, S, 2 * D)).astype(np.float32))
        k, v, ld = kv[..., :D], kv[..., D:], 2 * D
    else:
        k, v, ld = dev(rng.standard_normal((B, S, D)).astype(np.float32)), dev(rng.standard_normal((B, S, D)).astype(np.float32)), D
    fk, fv = Fenced(B, H, S, dh), Fenced(B, H, S, dh)
    call_hip_function("nnhipKVMemoryFill", StridedView(k), StridedView(v), fk.view, fv.view, B, H, S, dh, ld, get_current_stream_ptr())
    torch.cuda.synchronize()
    assert fk.guards_intact() and fv.guards_intact()
    assert torch.equal(fk.view, k.reshape(B, S, H, dh).permute(0, 2, 1, 3).contiguous())
    assert torch.equal(fv.view, v.reshape(B, S, H, dh).permute(0, 2, 1, 3).contiguous())


# ------------------------------------------------------------------------------------------- the model of examples/seq2seq.py
@pytest.fixture(scope="module")
def fx(golden):
    g = golden("seq2seq_tiny")
    step = {}
    k = 0
    while os.path.exists(os.path.join(GOLDEN, f"seq2seq_tiny_step_{k}.npz")):
        step.update(golden(f"seq2seq_tiny_step_{k}"))
        k += 1
    with open(os.path.join(GOLDEN, "seq2seq_tiny_state.pkl"), "rb") as f:
        state = pickle.load(f)
    return g, step, state


def build(g):
    V, D, H, F, L, max_len = [int(v) for v in g["cfg"]]
    return example().build_seq2seq(V, D, H, F, L, dropout=0.0, pad_idx=PAD, max_len=max_len)


def test_seq2seq_step_golden(hip, fx):
    """One full training step of the notebook's model (2 + 2 layers, d 64, 2 heads of 32, ragged sources and targets with PAD
    tails): logits, loss, every gradient and every parameter after Adam, through the fused kernels (need_weights=False)."""
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    S = example()
    g, st, _ = fx
    model = build(g)
    params = model.parameters()
    n = int(g["n_params"])
    assert len(params) == n
    for i, p in enumerate(params):
        assert tuple(p.shape) == st[f"p{i}"].shape, (i, p.shape, st[f"p{i}"].shape)
        p.data.copy_(dev(st[f"p{i}"]))
    lr, betas, eps = 3e-4, (0.9, 0.98), 1e-9
    opt = Adam(params, lr=lr, betas=betas, eps=eps)
    loss_fn = nn.CrossEntropyLoss(ignore_index=PAD)
    src, tgt = g["batch_src"], g["batch_tgt"]
    output, attn = model.forward(src, tgt[:, :-1])
    assert attn is None
    np.testing.assert_allclose(host(output.data), g["logits"], rtol=1e-4, atol=1e-4)
    out2 = output.reshape(output.shape[0] * output.shape[1], output.shape[2])
    loss = loss_fn(out2, hip.Tensor(np.ascontiguousarray(tgt[:, 1:]).reshape(-1), dtype=np.int32, requires_grad=False, device="cuda"))
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    gscale = grad_list_scale([st[f"g{i}"] for i in range(n)])
    our_grads = []
    for i, p in enumerate(params):
        assert p.grad is not None, i
        our_grads.append(host(p.grad).reshape(st[f"g{i}"].shape))
        assert_close_scaled(our_grads[i], st[f"g{i}"], err_msg=f"grad {i}", scale=gscale)
    opt.step()
    for i, p in enumerate(params):
        got = host(p.data)
        # (1) the fused Adam applied to OUR gradient == a float64 Adam on the same gradient, everywhere
        np.testing.assert_allclose(got, R.adam_first_steps(st[f"p{i}"], our_grads[i], lr, betas, eps), rtol=1e-5, atol=1e-6,
                                   err_msg=f"param {i} vs float64 Adam")
        # (2) the reference's own post-step parameters wherever the gradient is above rounding noise (eps = 1e-9 makes the first
        #     step lr * sign(g): a ~1e-9 gradient turns rounding noise into a full +-lr step in BOTH implementations)
        sig = np.abs(st[f"g{i}"]) > 1e-5
        np.testing.assert_allclose(got[sig], st[f"p_after{i}"][sig], rtol=1e-4, atol=2e-5, err_msg=f"param {i}")
    # the map the notebook's forward returns: the last decoder layer's cross-attention, on the unfused path
    model2 = build(g)
    for i, p in enumerate(model2.parameters()):
        p.data.copy_(dev(st[f"p{i}"]))
    out_w, attn_w = model2.forward(src, tgt[:, :-1], need_weights=True)
    np.testing.assert_allclose(host(attn_w), g["attn"], **TOL)
    np.testing.assert_allclose(host(out_w.data), g["logits"], **TOL)


@pytest.fixture(scope="module")
def loaded(hip, fx):
    g, _, state = fx
    np.random.seed(99)                                           # a different init: everything must come from the file
    model = build(g)
    sd = hip.load(os.path.join(GOLDEN, "seq2seq_tiny_state.pkl"))
    assert list(model.state_dict()) == list(sd)                  # the reference's key names, in its order
    model.load_state_dict(sd)
    return model


def test_reference_checkpoint_loads_and_round_trips(hip, fx, loaded, tmp_path):
    g, _, sd = fx
    out, _ = loaded.forward(g["batch_src"], g["batch_tgt"][:, :-1])
    np.testing.assert_allclose(host(out.data), g["logits"], rtol=1e-4, atol=1e-4)
    path = str(tmp_path / "ours.pkl")
    hip.save(loaded.state_dict(), path)
    back = hip.load(path)
    assert list(back) == list(sd)
    for k in sd:
        assert isinstance(back[k], np.ndarray) and back[k].dtype == sd[k].dtype
        np.testing.assert_array_equal(back[k], sd[k], err_msg=k)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_teacher_forced_cached_steps(hip, fx, loaded, i):
    """One cached decoder step per fixture token: every step's logits against the float64 restatement's, and the last layer's
    cross-attention map (need_weights=True) against the restatement's row for that step."""
    import torch
    g, _, state = fx
    H, max_length = int(g["cfg"][2]), int(g["max_length"])
    src, tokens, logits64 = g[f"src{i}"], g[f"tokens{i}"], g[f"logits64_{i}"]
    enc64, valid64 = R.encoder_forward(state, src[None], H, PAD)
    _, attn64 = R.decoder_forward(state, tokens[None, :-1], enc64, valid64, H, PAD)          # [1, H, T, S]
    loaded.eval()
    dec = loaded.decoder
    enc_src, src_valid = loaded.encode(src[None])
    np.testing.assert_allclose(host(enc_src.data), enc64, **TOL)
    memory = dec.fill_memory(enc_src.data, src_valid)
    cache = dec.new_cache(1, max_length)
    V, D = dec.fc_out.out_features, dec.fc_out.in_features
    ids_buf = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    tok, pos = torch.empty((1, 1, D), device="cuda"), torch.empty((1, 1, D), device="cuda")
    logits = torch.empty((1, 1, V), device="cuda")
    for t in range(len(tokens) - 1):
        ids_buf.fill_(int(tokens[t]))
        attn = dec.step(ids_buf, cache, memory, tok, pos, logits, need_weights=True)
        assert_close_scaled(host(logits)[0, 0], logits64[t], tol=1e-4, err_msg=f"sentence {i} step {t}")
        assert tuple(attn.shape) == (1, H, 1, len(src))
        np.testing.assert_allclose(host(attn)[0, :, 0], attn64[0, :, t], err_msg=f"sentence {i} step {t}: map", **TOL)
    assert cache.tokens == len(tokens) - 1
    loaded.train()


@pytest.mark.parametrize("mode", ["recompute", "cached", "graph"])
def test_translate_returns_the_reference_tokens(hip, fx, loaded, mode):
    S = example()
    g, _, _ = fx
    max_length = int(g["max_length"])
    want = [g[f"tokens{i}"].tolist() for i in range(3)]
    for i in range(3):
        stats = {}
        got = S.translate(loaded, g[f"src{i}"].tolist(), max_length=max_length, mode=mode, stats=stats)
        assert got == want[i], (mode, i)
        if mode == "graph":
            assert stats["host_syncs_between_tokens"] == 0 and stats["kernel_nodes"] > 0
        else:
            assert stats["host_syncs_between_tokens"] == len(want[i]) - 1
    # the three sentences as one right-padded batch: the same tokens per row
    stats = {}
    got = S.translate(loaded, [g[f"src{i}"].tolist() for i in range(3)], max_length=max_length, mode=mode, stats=stats)
    assert got == want, mode
    if mode == "graph":
        assert stats["host_syncs_between_tokens"] == 0
    assert loaded.training                                        # translate leaves the mode as it found it


def test_translate_need_weights_matches_the_restatement(hip, fx, loaded):
    S = example()
    g, _, state = fx
    H, max_length = int(g["cfg"][2]), int(g["max_length"])
    src, tokens = g["src2"], g["tokens2"]
    enc64, valid64 = R.encoder_forward(state, src[None], H, PAD)
    _, attn64 = R.decoder_forward(state, tokens[None, :-1], enc64, valid64, H, PAD)
    for mode in ("recompute", "cached"):
        stats = {}
        assert S.translate(loaded, src.tolist(), max_length=max_length, mode=mode, stats=stats, need_weights=True) == tokens.tolist()
        a = stats["attention"]
        assert a.shape == ((1, H, len(tokens) - 1, len(src)) if mode == "recompute" else (1, H, 1, len(src)))
        np.testing.assert_allclose(a[0, :, -1], attn64[0, :, -1], err_msg=mode, **TOL)
    with pytest.raises(ValueError, match="need_weights"):
        S.translate(loaded, src.tolist(), mode="graph", need_weights=True)


def test_qkv_projection_without_bias_is_one_gemm_and_matches_three(hip):
    """MultiHeadAttention(bias=False) self-attention: the packed q|k|v GEMM path (fuse_qkv) gives the output and the gradients of
    the three separate projections."""
    import torch
    import neunet_hip.nn as nn
    rng = np.random.default_rng(3)
    B, T, D, H = 2, 9, 64, 2
    X = rng.standard_normal((B, T, D)).astype(np.float32)
    dY = rng.standard_normal((B, T, D)).astype(np.float32)
    valid = np.ones((B, T), np.int32)
    valid[1, 6:] = 0
    np.random.seed(5)
    m = nn.MultiHeadAttention(D, H, bias=False)
    res = []
    for fuse in (True, False):
        m.fuse_qkv = fuse
        for p in m.parameters():
            p.grad = None
        x = hip.Tensor(X, device="cuda")
        y, attn = m(x, x, x, idev(valid), causal=True, need_weights=False)
        assert attn is None
        y.backward(dev(dY))
        res.append([host(y.data), host(x.grad)] + [host(p.grad) for p in m.parameters()])
    assert len(res[0]) == 2 + 5
    for a, b in zip(*res):
        assert_close_scaled(a.reshape(b.shape), b, tol=1e-4)
    torch.cuda.synchronize()
