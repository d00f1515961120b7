"""CPU: the float64 restatements the GPU tests of the GPT-2 inference path use (tests/gpt2_ref.py) against fixtures recorded from the
reference (tools/gen_golden.py: gen_layernorm_gelu, gen_gpt2), the conditions the greedy fixture must meet, argument errors of the
five new C entries (status codes, no GPU needed: every refusal happens before a launch), and the host-side bookkeeping of KVCache
and load_gpt2_weights."""
import glob
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from gpt2_ref import (attention_decode, cross_entropy_mean, gelu_backward, gelu_forward, gpt2_backward, gpt2_forward, greedy_margins,
                      layernorm_backward, layernorm_forward)
from test_hip_parity import assert_close_scaled, grad_list_scale

LN_CASES = ["layernorm_2d", "layernorm_3d", "layernorm_noaffine", "layernorm_shape2"]


def load_parts(prefix):
    """The arrays of tests/golden/<prefix>_<k>.npz, k = 0, 1, ... (tools/gen_golden.py: save_parts), as one dict in file order."""
    files = sorted(glob.glob(os.path.join(GOLDEN, prefix + "_[0-9]*.npz")), key=lambda f: int(f.rsplit("_", 1)[1][:-4]))
    assert files, prefix
    out = {}
    for f in files:
        out.update(dict(np.load(f, allow_pickle=False)))
    return out


def params_from_hf(hf, n_layer):
    """The model's arrays under its state_dict() names from a Hugging-Face-shaped state dict: the transposes and reshapes of
    load_gpt2_weights (HF's Conv1D holds [in, out]; nn.Linear holds [out, in] and a [1, out] bias).  lm_head is wte (tied)."""
    p = {"wte.weight": hf["transformer.wte.weight"], "wpe.weight": hf["transformer.wpe.weight"],
         "ln_f.weight": hf["transformer.ln_f.weight"], "ln_f.bias": hf["transformer.ln_f.bias"],
         "lm_head.weight": hf["transformer.wte.weight"]}
    for i in range(n_layer):
        for ln in ("ln_1", "ln_2"):
            for wb in ("weight", "bias"):
                p[f"h.{i}.{ln}.{wb}"] = hf[f"transformer.h.{i}.{ln}.{wb}"]
        for lin in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"):
            p[f"h.{i}.{lin}.weight"] = hf[f"transformer.h.{i}.{lin}.weight"].T
            p[f"h.{i}.{lin}.bias"] = hf[f"transformer.h.{i}.{lin}.bias"].reshape(1, -1)
    return p


# ------------------------------------------------------------------------------------------- restatements vs the reference's fixtures
@pytest.mark.parametrize("name", LN_CASES)
def test_layernorm_restatement_matches_reference_fixture(golden, name):
    f = golden(name)
    n_axes = len(f["normalized_shape"])
    Y, cache = layernorm_forward(f["X"], f.get("w"), f.get("b"), float(f["eps"]), n_axes)
    np.testing.assert_allclose(Y, f["Y"], rtol=1e-5, atol=1e-5)
    dX, dw, db = layernorm_backward(cache, f["dY"])
    np.testing.assert_allclose(dX, f["dX"], rtol=1e-4, atol=1e-5)
    if "w" in f:
        # (layernorm_3d: the reference's axis-0 sum was finished by apply_grad's reverse broadcast; the fixture holds the full sum)
        assert f["dw"].shape == f["w"].shape and f["db"].shape == f["b"].shape
        np.testing.assert_allclose(dw, f["dw"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(db, f["db"], rtol=1e-4, atol=1e-5)


def test_gelu_restatement_matches_reference_fixture(golden):
    f = golden("gelu")
    assert f["X"].min() <= -6 and f["X"].max() >= 6
    np.testing.assert_allclose(gelu_forward(f["X"]), f["Y"], rtol=1e-5, atol=1e-6)
    # the reference's backward rounds its constants to six digits (activations.py:396-401); the exact derivative differs from it by
    # less than the 1e-4 the GPU test allows
    dX = gelu_backward(f["X"], f["dY"])
    np.testing.assert_allclose(dX, f["dX"], rtol=1e-4, atol=1e-5)
    assert np.abs(dX - f["dX"]).max() < 2e-5


def test_attention_decode_restatement_is_softmax_attention():
    rng = np.random.default_rng(0)
    B, H, T, dh = 2, 3, 7, 8
    q, K, V = rng.standard_normal((B, H, dh)), rng.standard_normal((B, H, T, dh)), rng.standard_normal((B, H, T, dh))
    out = attention_decode(q, K, V, [T, 3], 0.3)
    for b, n in ((0, T), (1, 3)):
        for h in range(H):
            s = K[b, h, :n] @ q[b, h] * 0.3
            p = np.exp(s - s.max())
            np.testing.assert_allclose(out[b, h], (p / p.sum()) @ V[b, h, :n], rtol=1e-12)


# ------------------------------------------------------------------------------------------- gpt2_tiny
@pytest.fixture(scope="module")
def tiny(golden):
    f = golden("gpt2_tiny")
    hf, grads = load_parts("gpt2_tiny_hf"), load_parts("gpt2_tiny_grad")
    n_embd, n_head, n_layer, vocab, n_pos = (int(v) for v in f["cfg"])
    return dict(f=f, hf=hf, grads=grads, cfg=dict(n_embd=n_embd, n_head=n_head, n_layer=n_layer, vocab_size=vocab, n_positions=n_pos),
                params=params_from_hf(hf, n_layer))


def test_gpt2_tiny_fixture_shape(tiny):
    f, cfg = tiny["f"], tiny["cfg"]
    assert cfg == dict(n_embd=128, n_head=2, n_layer=2, vocab_size=512, n_positions=64)
    assert f["batch"].shape == (2, 25) and f["logits"].shape == (2, 24, 512)
    assert f["prompt"].shape == (8,) and f["tokens"].shape == (40,) and f["logits64"].shape == (40, 512)
    np.testing.assert_array_equal(f["tokens"][:8], f["prompt"])
    assert sorted(tiny["grads"]) == sorted(tiny["params"])
    for k, g in tiny["grads"].items():
        assert g.shape == tiny["params"][k].shape, k


def test_gpt2_tiny_greedy_fixture_conditions(tiny):
    """What tools/gen_golden.py asserted when it recorded the continuation, re-asserted on the stored arrays: in the float64
    restatement every step's top-1 minus top-2 margin is >= 1e-3 of that step's largest |logit|, the float64 argmax is the token the
    reference's float32 loop picked at EVERY one of the 32 steps, and the continuation has at least 8 distinct tokens."""
    f = tiny["f"]
    tokens = f["tokens"]
    logits64, _ = gpt2_forward(tiny["params"], tokens[None], tiny["cfg"]["n_head"])
    np.testing.assert_allclose(logits64[0], f["logits64"], rtol=1e-9, atol=1e-11)        # the stored float64 logits are the restatement's
    steps = f["logits64"][7:39]                                                          # position t predicts token t + 1
    margins = greedy_margins(steps)
    assert margins.shape == (32,) and margins.min() >= 1e-3, margins.min()
    np.testing.assert_array_equal(np.argmax(steps, axis=-1), tokens[8:])
    assert len(set(tokens[8:].tolist())) >= 8


def test_gpt2_restatement_matches_reference_fixture(tiny):
    f, params, H = tiny["f"], tiny["params"], tiny["cfg"]["n_head"]
    batch = f["batch"]
    logits, cache = gpt2_forward(params, batch[:, :-1], H)
    np.testing.assert_allclose(logits, f["logits"], rtol=1e-4, atol=1e-4)
    loss, dlogits = cross_entropy_mean(logits, batch[:, 1:])
    assert abs(loss - float(f["loss"])) < 1e-5
    grads = gpt2_backward(cache, dlogits)
    scale = grad_list_scale(list(tiny["grads"].values()))
    for k, ref in tiny["grads"].items():
        # (the reference computes in float32: 1e-4 of max(|entry|, tensor rms), as the GPU test holds the kernels to)
        assert_close_scaled(grads[k], ref, err_msg=k, scale=scale if k.endswith("c_attn.bias") else 0.0)


def test_gpt2_restatement_embedding_gradient_modes(tiny):
    """The batch repeats ids: the reference's assignment gradient keeps the last occurrence only; "sum" is the mathematical one."""
    f, params, H = tiny["f"], tiny["params"], tiny["cfg"]["n_head"]
    ids = f["batch"][:, :-1]
    assert len(np.unique(ids)) < ids.size
    logits, cache = gpt2_forward(params, ids, H)
    _, d = cross_entropy_mean(logits, f["batch"][:, 1:])
    ga, gs = gpt2_backward(cache, d)["wte.weight"], gpt2_backward(cache, d, embedding_grad="sum")["wte.weight"]
    rep = int(f["batch"][0, 3])
    assert np.any(ga[rep] != gs[rep])
    once = [t for t in np.unique(ids) if np.sum(ids == t) == 1]
    np.testing.assert_array_equal(ga[once], gs[once])


# ------------------------------------------------------------------------------------------- C ABI: refusals before any launch
@pytest.fixture(scope="module")
def lib():
    import neunet_hip
    from neunet_hip import _lib
    neunet_hip.load_library()
    return _lib


def test_abi_212_and_new_symbols(lib):
    assert lib.load_hip_function("nnhipVersion")() >= 212
    for name in ("nnhipLayerNormForward", "nnhipLayerNormBackward", "nnhipLayerNormBackwardEx", "nnhipGELUForward", "nnhipGELUBackward",
                 "nnhipAttentionDecode", "nnhipAttentionDecodeWorkspace", "nnhipKVCacheFill"):
        assert name in lib.exported_symbols()
        lib.load_hip_function(name)


def test_layernorm_argument_errors(lib):
    E = lib.NeunetHipError
    with pytest.raises(E, match="nnhipLayerNormForward: negative size"):
        lib.call_hip_function("nnhipLayerNormForward", 16, None, None, 16, 16, 16, -1, 8, 1e-5, None)
    with pytest.raises(E, match="nnhipLayerNormForward: null pointer"):
        lib.call_hip_function("nnhipLayerNormForward", None, None, None, 16, 16, 16, 4, 8, 1e-5, None)
    with pytest.raises(E, match="nnhipLayerNormForward: null pointer"):
        lib.call_hip_function("nnhipLayerNormForward", 16, None, None, 16, None, 16, 4, 8, 1e-5, None)     # mean is not optional
    with pytest.raises(E, match="nnhipLayerNormForward: misaligned"):
        lib.call_hip_function("nnhipLayerNormForward", 18, None, None, 16, 16, 16, 4, 8, 1e-5, None)
    with pytest.raises(E, match="nnhipLayerNormBackward: negative size"):
        lib.call_hip_function("nnhipLayerNormBackward", 16, 16, 16, 16, 16, 16, 16, 16, 4, -8, None)
    with pytest.raises(E, match="nnhipLayerNormBackward: null pointer"):
        lib.call_hip_function("nnhipLayerNormBackward", 16, 16, None, 16, 16, None, None, None, 4, 8, None)   # dX
    with pytest.raises(E, match="nnhipLayerNormBackward: null pointer"):
        lib.call_hip_function("nnhipLayerNormBackwardEx", None, 16, None, 16, 16, 16, 16, None, None, 4, 8, None)
    # empty problems are not errors
    assert lib.call_hip_function("nnhipLayerNormForward", None, None, None, None, None, None, 0, 8, 1e-5, None) == 0
    assert lib.call_hip_function("nnhipLayerNormBackward", None, None, None, None, None, None, None, None, 4, 0, None) == 0


def test_gelu_argument_errors(lib):
    E = lib.NeunetHipError
    with pytest.raises(E, match="nnhipGELUForward: negative size"):
        lib.call_hip_function("nnhipGELUForward", 16, 16, -1, None)
    with pytest.raises(E, match="nnhipGELUForward: null pointer"):
        lib.call_hip_function("nnhipGELUForward", None, 16, 4, None)
    with pytest.raises(E, match="nnhipGELUBackward: negative size"):
        lib.call_hip_function("nnhipGELUBackward", 16, 16, 16, -4, None)
    with pytest.raises(E, match="nnhipGELUBackward: null pointer"):
        lib.call_hip_function("nnhipGELUBackward", 16, None, 16, 4, None)
    with pytest.raises(E, match="nnhipGELUBackward: misaligned"):
        lib.call_hip_function("nnhipGELUBackward", 16, 16, 17, 4, None)
    assert lib.call_hip_function("nnhipGELUForward", None, None, 0, None) == 0


def test_attention_decode_argument_errors(lib):
    E = lib.NeunetHipError
    call = lambda *a: lib.call_hip_function("nnhipAttentionDecode", *a)  # noqa: E731
    #     qkv Kc  Vc  len  O  ws   B  H  Tmax dh  ld  scale stream
    with pytest.raises(E, match="unsupported head dim 48"):
        call(16, 16, 16, 16, 16, 16, 2, 2, 64, 48, 288, 0.1, None)
    with pytest.raises(E, match="nnhipAttentionDecode: negative size"):
        call(16, 16, 16, 16, 16, 16, -2, 2, 64, 64, 384, 0.1, None)
    with pytest.raises(E, match="nnhipAttentionDecode: null pointer"):
        call(16, 16, 16, None, 16, 16, 2, 2, 64, 64, 384, 0.1, None)
    with pytest.raises(E, match="nnhipAttentionDecode: null pointer"):
        call(None, 16, 16, 16, 16, 16, 2, 2, 64, 64, 384, 0.1, None)
    with pytest.raises(E, match="Tmax must be >= 1"):
        call(16, 16, 16, 16, 16, 16, 2, 2, 0, 64, 384, 0.1, None)
    with pytest.raises(E, match="ld_qkv smaller"):
        call(16, 16, 16, 16, 16, 16, 2, 2, 64, 64, 383, 0.1, None)
    with pytest.raises(E, match="null workspace"):
        call(16, 16, 16, 16, 16, None, 1, 2, 1024, 64, 384, 0.1, None)          # this shape splits the keys: partials needed
    with pytest.raises(E, match="16-byte aligned"):
        call(20, 16, 16, 16, 16, 16, 2, 2, 64, 64, 384, 0.1, None)
    assert call(None, None, None, None, None, None, 0, 2, 64, 64, 384, 0.1, None) == 0


def test_attention_decode_workspace_query(lib):
    ws = lib.load_hip_function("nnhipAttentionDecodeWorkspace")
    assert ws(1, 12, 1024, 64) == 12 * 16 * 66 * 4            # 16 splits of 64 keys, (max, sum, o[64]) each
    assert ws(64, 12, 1024, 64) == 64 * 12 * 2 * 66 * 4       # 768 (b, h) already cover the chip: 2 splits of 512 keys
    assert ws(2048, 2, 64, 32) == 0                           # one split: the block writes O itself
    assert ws(0, 12, 1024, 64) == 0
    assert ws(1, 12, 1024, 80) < 0 and "unsupported head dim" in lib.last_error()
    assert ws(1, -1, 1024, 64) < 0 and "negative size" in lib.last_error()
    with pytest.raises(lib.NeunetHipError, match="unsupported head dim"):
        from neunet_hip.nn.experimental.causal_attention import decode_workspace_bytes
        decode_workspace_bytes(1, 2, 64, 96)


def test_kv_cache_fill_argument_errors(lib):
    E = lib.NeunetHipError
    call = lambda *a: lib.call_hip_function("nnhipKVCacheFill", *a)  # noqa: E731
    #     qkv Kc  Vc  len  B  H  T  Tmax dh  ld stream
    with pytest.raises(E, match="unsupported head dim"):
        call(16, 16, 16, None, 2, 2, 8, 64, 40, 240, None)
    with pytest.raises(E, match="nnhipKVCacheFill: negative size"):
        call(16, 16, 16, None, 2, 2, -8, 64, 64, 384, None)
    with pytest.raises(E, match="do not fit"):
        call(16, 16, 16, None, 2, 2, 65, 64, 64, 384, None)
    with pytest.raises(E, match="nnhipKVCacheFill: null pointer"):
        call(16, None, 16, None, 2, 2, 8, 64, 64, 384, None)
    with pytest.raises(E, match="16-byte aligned"):
        call(16, 16, 16, None, 2, 2, 8, 64, 64, 386, None)
    assert call(None, None, None, None, 2, 2, 0, 64, 64, 384, None) == 0


# ------------------------------------------------------------------------------------------- host layers without a device
def test_layernorm_and_gelu_module_contract(golden):
    import neunet_hip.nn as nn
    from neunet_hip.nn.experimental import HIPGELU, HIPLayerNorm
    assert nn.LayerNorm is HIPLayerNorm and nn.GELU is HIPGELU
    m = nn.LayerNorm(48, device="cpu")
    assert m.normalized_shape == (48,) and m.eps == 1e-5 and m.elementwise_affine
    assert list(m.state_dict()) == ["weight", "bias"] and len(m.parameters()) == 2
    assert m.weight.data.dtype == np.float32 and np.all(m.weight.data == 1) and not np.any(m.bias.data)
    m2 = nn.LayerNorm((4, 32), eps=1e-6, device="cpu")
    assert m2.weight.shape == (4, 32) and m2.bias.shape == (4, 32) and m2.eps == 1e-6
    m3 = nn.LayerNorm(16, elementwise_affine=False, device="cpu")
    assert m3.weight is None and m3.bias is None and m3.parameters() == [] and list(m3.state_dict()) == []
    from neunet_hip import Tensor
    with pytest.raises(NotImplementedError, match="HIP device"):          # no CPU fallback
        m(Tensor(np.zeros((2, 48), np.float32)))
    with pytest.raises(NotImplementedError, match="HIP device"):
        nn.GELU()(Tensor(np.zeros((2, 48), np.float32)))


def test_kv_cache_bookkeeping(monkeypatch):
    """KVCache on host tensors: shapes, the per-layer views, the host mirror of the lengths, capacity errors; the decode / fill
    wrappers hand the right buffers and sizes to the library (the calls themselves are replaced: no device here)."""
    import torch
    from neunet_hip.nn.experimental import causal_attention as CA
    c = CA.KVCache(3, 96, 2, 4, 64, device="cpu")
    assert c.k.shape == c.v.shape == (2, 3, 4, 96, 64) and c.cache_len.dtype == torch.int32 and c.cache_len.tolist() == [0, 0, 0]
    assert c.workspace is not None and c.workspace.numel() * 4 >= CA.decode_workspace_bytes(3, 4, 96, 64) > 0
    l1 = c.layer(1)
    assert l1.owner is c and l1.k.data_ptr() == c.k[1].data_ptr() and l1.k.is_contiguous() and l1.k.shape == (3, 4, 96, 64)
    assert c.room() == 96
    c.advance(90)
    assert c.tokens == 90 and c.cache_len.tolist() == [90, 90, 90] and c.room() == 6
    c.advance()
    assert c.cache_len.tolist() == [91] * 3
    with pytest.raises(ValueError, match="do not fit"):
        c.advance(6)
    assert c.cache_len.tolist() == [91] * 3                               # a refused advance changes nothing
    c.replayed(1)
    assert c.tokens == 92 and c.cache_len.tolist() == [91] * 3            # (a replayed graph advances the device side itself)
    c.set_lengths([0, 5, 95])
    assert c.tokens == 95 and c.cache_len.tolist() == [0, 5, 95]
    with pytest.raises(ValueError, match="one length"):
        c.set_lengths([0, 5, 97])
    c.reset()
    assert c.tokens == 0 and c.cache_len.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="head dim 48"):
        CA.KVCache(1, 8, 1, 2, 48, device="cpu")
    calls = []
    monkeypatch.setattr(CA, "call_hip_function", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(CA, "get_current_stream_ptr", lambda: 0)
    qkv = torch.zeros((3, 1, 768))
    out = torch.zeros((3, 1, 256))
    CA.attention_decode(qkv, l1, out, 0.125)
    name, a = calls[-1]
    assert name == "nnhipAttentionDecode" and a[1] is l1.k and a[2] is l1.v and a[3] is c.cache_len and a[4] is out and a[5] is c.workspace
    assert a[6:] == (3, 4, 96, 64, 768, 0.125, 0)
    CA.kv_cache_fill(torch.zeros((3, 7, 768)), c.layer(0), 7)
    name, a = calls[-1]
    assert name == "nnhipKVCacheFill" and a[1] is c.layer(0).k and a[3] is c.cache_len and a[4:] == (3, 4, 7, 96, 64, 768, 0)


def test_load_gpt2_weights_key_mapping(tiny):
    """A CPU skeleton of the example's model takes the fixture's Hugging-Face-shaped checkpoint key for key: every parameter ends
    up as the array the restatement uses (transposed Linear weights, [1, out] biases), the head stays tied, a missing key and a
    wrongly shaped array are errors, and the `transformer.` prefix is optional."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import gpt2_infer as G
    cfg, hf = tiny["cfg"], tiny["hf"]
    m = G.GPT2(cfg, device="cpu")
    names = list(m.state_dict())
    assert names[:4] == ["wte.weight", "wpe.weight", "h.0.ln_1.weight", "h.0.ln_1.bias"] and names[-1] == "lm_head.weight"
    assert sorted(names) == sorted(tiny["params"])
    G.load_gpt2_weights(m, hf)
    sd = m.state_dict()
    for k, v in tiny["params"].items():
        np.testing.assert_array_equal(sd[k], v, err_msg=k)
    assert m.lm_head.weight is m.wte.weight
    m.to("cpu")
    assert m.lm_head.weight is m.wte.weight
    bare = {k.replace("transformer.", "", 1): v for k, v in hf.items()}
    m2 = G.GPT2(cfg, device="cpu")
    G.load_gpt2_weights(m2, bare)
    np.testing.assert_array_equal(m2.h[1].mlp.c_fc.weight.data, tiny["params"]["h.1.mlp.c_fc.weight"])
    missing = dict(hf)
    del missing["transformer.h.1.ln_2.bias"]
    with pytest.raises(KeyError, match="ln_2.bias"):
        G.load_gpt2_weights(G.GPT2(cfg, device="cpu"), missing)
    wrong = dict(hf)
    wrong["transformer.h.0.attn.c_attn.weight"] = hf["transformer.h.0.attn.c_attn.weight"].T.copy()
    with pytest.raises(ValueError, match="shape mismatch"):
        G.load_gpt2_weights(G.GPT2(cfg, device="cpu"), wrong)
    rs = G.random_gpt2_state(cfg, 3)
    assert sorted(rs) == sorted(hf) and all(rs[k].shape == hf[k].shape for k in hf)


def test_generate_argument_errors():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import gpt2_infer as G
    m = G.GPT2(dict(n_embd=64, n_head=2, n_layer=1, vocab_size=32, n_positions=16), device="cpu")
    with pytest.raises(ValueError, match="exceed n_positions"):
        G.generate(m, np.zeros((1, 10), np.int32), 7, mode="cached")
    with pytest.raises(ValueError, match="at least one token"):
        G.generate(m, np.zeros((1, 0), np.int32), 4)
