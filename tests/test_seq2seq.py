"""CPU-only: the seq2seq fixture's own conditions, the float64 restatement (tests/seq2seq_ref.py) against what the reference computed,
the C ABI of the cross-attention decode kernel and of the memory fill (ABI 217; every argument check happens before any device
call), and the host-side logic of examples/seq2seq.py."""
import os
import pickle
import sys

import numpy as np
import pytest

import seq2seq_ref as R
from conftest import GOLDEN, ROOT
from test_abi import lib  # noqa: F401  (fixture: builds the library if it is missing, then loads it)

EINVAL, EALIGN = -1, -2
DUMMY = 0x1000                      # a non-null, 16-byte aligned pointer value nothing dereferences: every check precedes the device
PAD, SOS, EOS = 0, 1, 2


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("seq2seq_tiny")
    with open(os.path.join(GOLDEN, "seq2seq_tiny_state.pkl"), "rb") as f:
        state = pickle.load(f)
    return g, state


def example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import seq2seq
    return seq2seq


# ---- the fixture's own conditions (tools/gen_golden.py asserts the same when it writes the files; no step is exempt) ---------------
def test_fixture_conditions(fx):
    g, state = fx
    V, D, H, F, L, _ = [int(v) for v in g["cfg"]]
    assert (V, D, H, F, L) == (40, 64, 2, 96, 2) and D // H == 32       # head dim 32: the fused and the decode kernels are what is tested
    max_length = int(g["max_length"])
    assert list(state) == [str(n) for n in g["names"]]
    lengths, new_counts = set(), []
    for i in range(3):
        src, tokens, logits64 = g[f"src{i}"], g[f"tokens{i}"], g[f"logits64_{i}"]
        lengths.add(len(src))
        assert tokens[0] == SOS and len(tokens) <= max_length and logits64.shape == (len(tokens) - 1, V)
        assert EOS not in tokens[1:-1].tolist()                            # the loop stops at the first EOS
        assert tokens[-1] == EOS or len(tokens) == max_length              # ... or at max_length, nowhere else
        # float64 picks the tokens of the reference's float32 loop, with a margin at every step
        np.testing.assert_array_equal(np.argmax(logits64, axis=-1), tokens[1:])
        assert R.greedy_margins(logits64).min() >= 1e-3
        new = [t for t in tokens[1:].tolist() if t != EOS]
        assert len(new) >= 8 and len(set(new)) >= 4 and PAD not in new
        new_counts.append(len(new))
    assert len(lengths) == 3                                               # three sources of different lengths
    assert any(n == max_length - 1 for n in new_counts) and any(n < max_length - 1 for n in new_counts)    # both arms of the stop rule
    src, tgt = g["batch_src"], g["batch_tgt"]
    assert src.shape[0] == 3 and len({int((r != PAD).sum()) for r in src}) == 3 and len({int((r != PAD).sum()) for r in tgt}) == 3
    assert (src[:, -1] == PAD).any() and (tgt[:, -1] == PAD).any()         # PAD tails on both sides


# ---- the restatement against the reference ------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_step(fx):
    g, state = fx
    H = int(g["cfg"][2])
    logits, attn = R.seq2seq_forward(state, g["batch_src"], g["batch_tgt"][:, :-1], H, PAD)
    np.testing.assert_allclose(logits, g["logits"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(attn, g["attn"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(attn.sum(-1), 1.0, rtol=0, atol=1e-12)
    for b, row in enumerate(g["batch_src"]):
        assert np.all(attn[b][:, :, row == PAD] == 0.0)                     # source padding gets no weight


@pytest.mark.parametrize("i", [0, 1, 2])
def test_restatement_reproduces_the_reference_tokens(fx, i):
    g, state = fx
    H, max_length = int(g["cfg"][2]), int(g["max_length"])
    tokens, steps, _ = R.greedy(state, g[f"src{i}"], H, max_length, SOS, EOS, PAD)
    assert tokens == g[f"tokens{i}"].tolist()
    # the loop's per-prefix passes and the stored one-pass logits are the same numbers (causality)
    np.testing.assert_allclose(steps, g[f"logits64_{i}"], rtol=1e-4, atol=1e-4)


def test_cross_decode_ref_rules():
    rng = np.random.default_rng(0)
    B, H, S, dh = 2, 2, 5, 4
    Q, K, V = rng.standard_normal((B, H * dh)), rng.standard_normal((B, H, S, dh)), rng.standard_normal((B, H, S, dh))
    valid = np.array([[1, 1, 0, 1, 0], [0, 0, 0, 0, 0]], np.int32)
    O, P = R.cross_decode_ref(Q, K, V, valid, 0.37)
    assert np.all(P[0][:, [2, 4]] == 0.0) and np.allclose(P.sum(-1), 1.0)
    np.testing.assert_allclose(P[1], 1.0 / S)                              # fully masked: -1e9 everywhere, not -inf
    np.testing.assert_allclose(O[1], V[1].mean(1).reshape(-1))
    O2, P2 = R.cross_decode_ref(Q, K, V, None, 0.37)
    s = np.einsum("hd,hsd->hs", Q[0].reshape(H, dh), K[0]) * 0.37
    np.testing.assert_allclose(P2[0], np.exp(s) / np.exp(s).sum(-1, keepdims=True))


# ---- ABI 217 -----------------------------------------------------------------------------------------------------------------------------
def cross(*args):
    from neunet_hip import _lib
    return _lib.load_hip_function("nnhipAttentionDecodeCross")(*args)


def fill(*args):
    from neunet_hip import _lib
    return _lib.load_hip_function("nnhipKVMemoryFill")(*args)


def test_abi_217_symbols_bind(lib):  # noqa: F811
    from neunet_hip import _lib
    assert _lib.load_hip_function("nnhipVersion")() >= 217
    for name in ("nnhipAttentionDecodeCross", "nnhipKVMemoryFill"):
        assert hasattr(lib, name), name
        assert name in _lib.exported_symbols()
        _lib.load_hip_function(name)


def test_cross_decode_status_codes_need_no_device(lib):  # noqa: F811
    from neunet_hip import _lib
    D = DUMMY
    ok = dict(B=2, H=2, S=7, dh=32, ld=64)

    def call(Q=D, K=D, V=D, kv=None, O=D, P=None, **kw):
        a = {**ok, **kw}
        return cross(Q, K, V, kv, O, P, a["B"], a["H"], a["S"], a["dh"], a["ld"], 0.125, None)

    for name in ("Q", "K", "V", "O"):                                       # NULL Q / Kmem / Vmem / O
        assert call(**{name: None}) == EINVAL
        assert "nnhipAttentionDecodeCross" in _lib.last_error() and "null" in _lib.last_error()
    for dh in (0, 16, 48, 96, 256):                                         # head_dim outside {32, 64, 128}
        assert call(dh=dh, ld=1024) == EINVAL
        assert "head dim" in _lib.last_error()
    for S in (0, -3):                                                       # S < 1 with B > 0
        assert call(S=S) == EINVAL
    for ld in (63, 32, 66, 0):                                              # ld_q < D, or not a multiple of 4
        assert call(ld=ld) == EINVAL
        assert "ld_q" in _lib.last_error()
    for name in ("Q", "K", "V", "O"):                                       # 16-byte alignment of the four operands
        for off in (4, 8):
            assert call(**{name: D + off}) == EALIGN
            assert "nnhipAttentionDecodeCross" in _lib.last_error() and "aligned" in _lib.last_error()
    # B == 0: 0 and no launch, whatever the pointers are (S < 1 is only an error with B > 0)
    assert cross(None, None, None, None, None, None, 0, 2, 7, 32, 64, 0.125, None) == 0
    assert cross(None, None, None, None, None, None, 0, 2, 0, 32, 64, 0.125, None) == 0
    assert cross(None, None, None, None, None, None, 0, 2, 7, 48, 64, 0.125, None) == EINVAL   # head_dim is checked for every B


def test_memory_fill_status_codes_need_no_device(lib):  # noqa: F811
    from neunet_hip import _lib
    D = DUMMY

    def call(K=D, V=D, Km=D, Vm=D, B=2, H=2, S=7, dh=32, ld=128):
        return fill(K, V, Km, Vm, B, H, S, dh, ld, None)

    for name in ("K", "V", "Km", "Vm"):
        assert call(**{name: None}) == EINVAL
        assert "nnhipKVMemoryFill" in _lib.last_error() and "null" in _lib.last_error()
        assert call(**{name: D + 4}) == EALIGN
    for dh in (0, 16, 96):
        assert call(dh=dh, ld=1024) == EINVAL
    assert call(S=0) == EINVAL
    for ld in (63, 130):
        assert call(ld=ld) == EINVAL
    assert fill(None, None, None, None, 0, 2, 7, 32, 64, None) == 0


# ---- host logic of the example ----------------------------------------------------------------------------------------------------------
def test_reverse_task_is_deterministic_and_well_formed():
    S = example()
    a = list(S.reverse_batches(40, 4, 3, seed=5))
    b = list(S.reverse_batches(40, 4, 3, seed=5))
    c = list(S.reverse_batches(40, 4, 3, seed=6))
    for (s1, t1), (s2, t2) in zip(a, b):
        np.testing.assert_array_equal(s1, s2)
        np.testing.assert_array_equal(t1, t2)
    assert any(x[0].shape != y[0].shape or (x[0] != y[0]).any() for x, y in zip(a, c))
    for src, tgt in a:
        assert src.dtype == np.int32 and src.shape == tgt.shape and src.shape[0] == 4
        for s_row, t_row in zip(src, tgt):
            s, t = S.trim_at_eos(s_row), S.trim_at_eos(t_row)
            assert s[0] == S.SOS and s[-1] == S.EOS and t[0] == S.SOS and t[-1] == S.EOS
            assert t[1:-1] == s[1:-1][::-1] and min(s[1:-1]) >= 3 and max(s[1:-1]) < 40
            assert all(v == S.PAD for v in s_row[len(s):]) and all(v == S.PAD for v in t_row[len(t):])    # right-padded
    with pytest.raises(ValueError):
        next(S.reverse_batches(3, 2, 1))


def test_masks_are_key_valid_plus_causal(fx):
    """The notebook's masks (cell 9) restated on the host: src_mask is key_valid of the source, tgt_mask is key_valid of the target
    AND the causal triangle -- what the example hands to the kernels as (key_valid, causal)."""
    g, _ = fx
    src, tgt = g["batch_src"], g["batch_tgt"][:, :-1]
    src_valid, tgt_valid = (src != PAD).astype(np.int32), (tgt != PAD).astype(np.int32)
    T = tgt.shape[1]
    pad_mask = lambda x: (x != PAD).astype(int)[:, np.newaxis, :]  # noqa: E731
    sub_mask = np.logical_not(np.triu(np.ones((T, T)), k=1).astype(int))
    np.testing.assert_array_equal(pad_mask(src)[:, 0], src_valid)
    np.testing.assert_array_equal(pad_mask(tgt) & sub_mask, tgt_valid[:, None, :] & np.tril(np.ones((T, T), int))[None])


def test_trim_and_pad_helpers():
    S = example()
    assert S.trim_at_eos([1, 5, 6, 2, 7, 2]) == [1, 5, 6, 2]
    assert S.trim_at_eos([1, 5, 6]) == [1, 5, 6]
    assert S.trim_at_eos(np.array([2, 2], np.int32)) == [2]
    np.testing.assert_array_equal(S.pad_batch([[1, 4, 2], [1, 2]]), np.array([[1, 4, 2], [1, 2, 0]], np.int32))
    with pytest.raises(ValueError):
        S.pad_batch([[1], []])
    with pytest.raises(ValueError, match="bogus"):
        S.translate(None, [1, 5, 2], mode="bogus")
    with pytest.raises(ValueError, match="max_length"):
        S.translate(None, [1, 5, 2], max_length=1)


def test_parser():
    S = example()
    ap = S.build_parser()
    a = ap.parse_args([])
    assert (a.config, a.task, a.mode, a.max_length, a.steps) == ("tiny", "reverse", "graph", 50, 200)
    a = ap.parse_args(["--config", "notebook", "--mode", "cached", "--max-length", "12", "--steps", "3", "--batch", "8"])
    assert (a.config, a.mode, a.max_length, a.steps, a.batch) == ("notebook", "cached", 12, 3, 8)
    assert S.CONFIGS["notebook"] == dict(vocab=15000, d_model=256, n_heads=8, d_ff=512, n_layers=3)
    assert S.CONFIGS["tiny"] == dict(vocab=40, d_model=64, n_heads=2, d_ff=96, n_layers=2)
    for bad in (["--mode", "beam"], ["--config", "huge"], ["--task", "copy"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_multi_head_attention_without_qkv_bias_state_dict():
    import neunet_hip.nn as nn
    m = nn.MultiHeadAttention(64, 2, bias=False, device="cpu")
    assert list(m.state_dict()) == ["wq.weight", "wk.weight", "wv.weight", "fc.weight", "fc.bias"]
    assert m.wq.bias is None and m.wk.bias is None and m.wv.bias is None and m.fc.bias is not None
    assert len(m.parameters()) == 5
    d = nn.MultiHeadAttention(64, 2, device="cpu")                          # the default is unchanged
    assert list(d.state_dict()) == ["wq.weight", "wq.bias", "wk.weight", "wk.bias", "wv.weight", "wv.bias", "fc.weight", "fc.bias"]
    assert m.scale == 8.0                                                   # sqrt(d_model), not sqrt(head_dim)
