"""GPU: the GPT-2 inference path -- nn.LayerNorm and nn.GELU (csrc/rowops.hip, csrc/elementwise.hip), the KV-cached decode
attention kernel (csrc/attention_decode.hip) and the model of examples/gpt2_infer.py -- against the reference's fixtures and the
float64 restatements of tests/gpt2_ref.py.

Tolerances are the ones the LSTM fixture tests use: rtol = atol = 1e-4 on outputs, assert_close_scaled (1e-4 of max(|entry|, the
tensor's rms)) on gradients and on the decode kernel's outputs, as the fused-attention parity tests do."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from gpt2_ref import attention_decode, gelu_backward, gelu_forward, layernorm_backward, layernorm_forward
from lstm_abi import Fenced, dev
from test_gpt2 import LN_CASES, load_parts, params_from_hf
from test_hip_parity import assert_close_scaled, grad_list_scale

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)


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


def make_layernorm(shape, w, b, eps=1e-5):
    import torch
    import neunet_hip.nn as nn
    m = nn.LayerNorm(shape, eps=eps, elementwise_affine=w is not None)
    if w is not None:
        m.weight.data.copy_(torch.from_numpy(np.ascontiguousarray(w, np.float32)))
        m.bias.data.copy_(torch.from_numpy(np.ascontiguousarray(b, np.float32)))
    return m


def run_layernorm(hip, X, w, b, dY, shape=None, eps=1e-5):
    m = make_layernorm(shape if shape is not None else X.shape[-1], w, b, eps)
    x = hip.Tensor(X, device="cuda")
    y = m(x)
    y.backward(dev(dY))
    return host(y.data), host(x.grad), (host(m.weight.grad), host(m.bias.grad)) if w is not None else (None, None)


# ------------------------------------------------------------------------------------------- LayerNorm / GELU
@pytest.mark.parametrize("name", LN_CASES)
def test_layernorm_fixture(hip, golden, name):
    f = golden(name)
    shape = tuple(int(v) for v in f["normalized_shape"])
    Y, dX, (dw, db) = run_layernorm(hip, f["X"], f.get("w"), f.get("b"), f["dY"], shape if len(shape) > 1 else shape[0], float(f["eps"]))
    np.testing.assert_allclose(Y, f["Y"], **TOL)
    assert dX.shape == f["X"].shape
    assert_close_scaled(dX, f["dX"], err_msg="dX")
    if "w" in f:
        assert dw.shape == f["w"].shape and db.shape == f["b"].shape
        assert_close_scaled(dw, f["dw"], err_msg="dw")
        assert_close_scaled(db, f["db"], err_msg="db")


def test_gelu_fixture(hip, golden):
    import neunet_hip.nn as nn
    f = golden("gelu")
    x = hip.Tensor(f["X"], device="cuda")
    y = nn.GELU()(x)
    y.backward(dev(f["dY"]))
    np.testing.assert_allclose(host(y.data), f["Y"], **TOL)
    np.testing.assert_allclose(host(x.grad), f["dX"], **TOL)


@pytest.mark.parametrize("cols", [768, 3072])
def test_layernorm_gpt2_size_vs_float64(hip, cols):
    rng = np.random.default_rng(cols)
    rows = 16384
    X = (rng.standard_normal((rows, cols)) * 1.3 + 0.2).astype(np.float32)
    dY = rng.standard_normal((rows, cols)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, cols).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, cols).astype(np.float32)
    Y, dX, (dw, db) = run_layernorm(hip, X, w, b, dY)
    Yr, cache = layernorm_forward(X, w, b)
    dXr, dwr, dbr = layernorm_backward(cache, dY)
    np.testing.assert_allclose(Y, Yr, **TOL)
    assert_close_scaled(dX, dXr, err_msg="dX")
    assert_close_scaled(dw, dwr, err_msg="dw")
    assert_close_scaled(db, dbr, err_msg="db")


@pytest.mark.parametrize("cols", [768, 3072])
def test_gelu_gpt2_size_vs_float64(hip, cols):
    import neunet_hip.nn as nn
    rng = np.random.default_rng(cols + 1)
    X = (rng.standard_normal((16384, cols)) * 2).astype(np.float32)
    dY = rng.standard_normal(X.shape).astype(np.float32)
    x = hip.Tensor(X, device="cuda")
    y = nn.GELU()(x)
    y.backward(dev(dY))
    np.testing.assert_allclose(host(y.data), gelu_forward(X), **TOL)
    np.testing.assert_allclose(host(x.grad), gelu_backward(X, dY), **TOL)


@pytest.mark.parametrize("cols", [1, 63, 65, 1000])
@pytest.mark.parametrize("affine", [True, False])
def test_layernorm_ragged_columns(hip, cols, affine):
    """Column counts that are no multiple of the 4-float vector, of the 64-lane row or of anything else; 37 rows leave the last
    4-row block ragged too.  cols == 1: the row IS its mean -- Y = bias and dw = 0 exactly, dX = 0 up to the cancellation below."""
    rng = np.random.default_rng(cols * 2 + affine)
    X = (rng.standard_normal((37, cols)) + 0.5).astype(np.float32)
    dY = rng.standard_normal((37, cols)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, cols).astype(np.float32) if affine else None
    b = rng.uniform(-0.5, 0.5, cols).astype(np.float32) if affine else None
    Y, dX, (dw, db) = run_layernorm(hip, X, w, b, dY)
    Yr, cache = layernorm_forward(X, w, b)
    dXr, dwr, dbr = layernorm_backward(cache, dY)
    np.testing.assert_allclose(Y, Yr, **TOL)
    # cols == 1: dX = rstd (g - mean(g)) is mathematically ZERO, the difference of two terms of size rstd |g| with rstd =
    # 1/sqrt(eps) = 316 (the variance is 0).  assert_close_scaled's `scale` is made for exactly this: the magnitude the tensor
    # would have if its terms did not cancel -- here the rms of rstd * g, from the float64 side.
    g = dY.astype(np.float64) * (w if affine else 1.0)
    scale = float(np.sqrt(np.mean((cache["rstd"] * g) ** 2))) if cols == 1 else 0.0
    assert_close_scaled(dX, dXr, err_msg="dX", scale=scale)
    if affine:
        assert_close_scaled(dw, dwr, err_msg="dw")
        assert_close_scaled(db, dbr, err_msg="db")


@pytest.mark.parametrize("rows,cols", [(64, 768), (37, 1000), (5, 20000)])
def test_layernorm_backward_addend_is_plain_plus_addend_bit_for_bit(hip, rows, cols):
    """nnhipLayerNormBackwardEx folds an already accumulated gradient of X into dX.  BIT FOR BIT the plain entry's dX plus the
    addend: the kernel adds it with a separately rounded add (no contraction into the preceding multiply), so the comparison is
    array_equal against one float32 add of the two arrays -- not a 1-ulp allowance.  (5, 20000): the looped kernels of rows wider
    than the register tile.)  dW / dB do not depend on the addend."""
    import torch
    from neunet_hip.nn.experimental.layernorm import layernorm_backward as hip_bwd, layernorm_forward as hip_fwd
    rng = np.random.default_rng(rows + cols)
    X, dY, add = (dev(rng.standard_normal((rows, cols))) for _ in range(3))
    w = dev(rng.uniform(0.5, 1.5, cols))
    b = dev(rng.uniform(-0.5, 0.5, cols))
    Y, mean, rstd = torch.empty_like(X), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    hip_fwd(X, w, b, Y, mean, rstd, cols, 1e-5)
    outs = []
    for addend in (None, add):
        dX, dw, db = torch.empty_like(X), torch.empty_like(w), torch.empty_like(b)
        hip_bwd(X, w, dY, dX, dw, db, mean, rstd, cols, grad_X_addend=addend)
        outs.append((host(dX), host(dw), host(db)))
    np.testing.assert_array_equal(outs[1][0], outs[0][0] + host(add))
    np.testing.assert_array_equal(outs[1][1], outs[0][1])
    np.testing.assert_array_equal(outs[1][2], outs[0][2])
    Yr, cache = layernorm_forward(host(X), host(w), host(b))
    np.testing.assert_allclose(host(Y), Yr, **TOL)
    assert_close_scaled(outs[0][0], layernorm_backward(cache, host(dY))[0], err_msg="dX")


def test_layernorm_residual_gradient_is_folded(hip):
    """x + f(LayerNorm(x)): the residual branch's gradient is already on x when the LayerNorm node runs, and the Ex entry folds it."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(5)
    X = rng.standard_normal((6, 10, 96)).astype(np.float32)
    dY = rng.standard_normal(X.shape).astype(np.float32)
    m = make_layernorm(96, rng.uniform(0.5, 1.5, 96), rng.uniform(-0.5, 0.5, 96))
    x = hip.Tensor(X, device="cuda")
    out = x + nn.GELU()(m(x))
    out.backward(dev(dY))
    Yr, cache = layernorm_forward(X, host(m.weight.data), host(m.bias.data))
    dXr = dY + layernorm_backward(cache, gelu_backward(Yr, dY))[0]
    assert_close_scaled(host(x.grad), dXr, err_msg="dX")


def layernorm_abi(rows, cols, seed, off=0):
    """Inputs for the C entries, forward already run.  off: every buffer starts `off` floats into its allocation.  Returns the
    device tensors, an allocator of such buffers, and the float64 (Y, dX, dw, db)."""
    import torch
    from neunet_hip.nn.experimental.layernorm import layernorm_forward as hip_fwd
    rng = np.random.default_rng(seed)

    def buf(*shape, fill=float("nan")):
        return torch.full((int(np.prod(shape)) + off,), fill, device="cuda")[off:].view(*shape)

    def put(a):
        t = buf(*a.shape)
        t.copy_(dev(a))
        return t

    X = put(rng.standard_normal((rows, cols)) * 1.3 + 0.2)
    dY = put(rng.standard_normal((rows, cols)))
    w, b = put(rng.uniform(0.5, 1.5, cols)), put(rng.uniform(-0.5, 0.5, cols))
    Y, mean, rstd = buf(rows, cols), buf(rows), buf(rows)
    hip_fwd(X, w, b, Y, mean, rstd, cols, 1e-5)
    Yr, cache = layernorm_forward(host(X), host(w), host(b))
    return dict(X=X, dY=dY, w=w, b=b, Y=Y, mean=mean, rstd=rstd), buf, (Yr,) + layernorm_backward(cache, host(dY))


@pytest.mark.parametrize("cols,off", [(1024, 0), (1028, 0), (4096, 0), (8192, 0), (12000, 0), (16384, 0), (4096, 1)])
def test_layernorm_every_tier_at_few_rows(hip, cols, off):
    """Nine rows through every (threads per row, vectors per thread) tier of the register-tile kernels above 512 columns, forward
    and backward, affine, against float64: 1024 is the widest wave-per-row tier, 1028 / 4096 / 8192 the block-per-row tiers with
    the next row prefetched, 12000 / 16384 the 1024-thread tier without prefetch (16384: a full tile).  off = 1: every buffer
    starts 4 bytes into its allocation -- 4-byte aligned, so the entries accept it, but not 16-byte aligned: the scalar variant of
    the 4096 tier."""
    from neunet_hip.nn.experimental.layernorm import layernorm_backward as hip_bwd
    t, buf, (Yr, dXr, dwr, dbr) = layernorm_abi(9, cols, cols + off, off)
    assert all(v.data_ptr() % 16 == 4 * off for v in t.values())
    dX, dw, db = buf(9, cols), buf(cols), buf(cols)
    hip_bwd(t["X"], t["w"], t["dY"], dX, dw, db, t["mean"], t["rstd"], cols)
    np.testing.assert_allclose(host(t["Y"]), Yr, **TOL)
    assert_close_scaled(host(dX), dXr, err_msg="dX")
    assert_close_scaled(host(dw), dwr, err_msg="dw")
    assert_close_scaled(host(db), dbr, err_msg="db")


@pytest.mark.parametrize("rows,cols", [(37, 1000), (37, 1001), (5, 16388)])
def test_layernorm_backward_nullable_outputs(hip, rows, cols):
    """nnhipLayerNormBackward with dW, dB or both NULL.  (37, 1000) / (37, 1001): the register tile, vector and scalar variant (1001
    is no multiple of 4), a ragged last 4-row block; (5, 16388): the looped dX kernel and the column pass.  What is asked for is BIT-identical to the call that asks for both, dX
    is the same in all four, and a buffer that was not passed keeps its sentinel."""
    import torch
    from neunet_hip.nn.experimental.layernorm import layernorm_backward as hip_bwd
    t, buf, (_, dXr, dwr, dbr) = layernorm_abi(rows, cols, rows + cols)
    outs = {}
    for want_w, want_b in [(True, True), (True, False), (False, True), (False, False)]:
        dX, dw, db = buf(rows, cols), buf(cols, fill=123.0), buf(cols, fill=321.0)
        hip_bwd(t["X"], t["w"], t["dY"], dX, dw if want_w else None, db if want_b else None, t["mean"], t["rstd"], cols)
        outs[want_w, want_b] = (dX, dw, db)
    dX0, dw0, db0 = outs[True, True]
    assert_close_scaled(host(dX0), dXr, err_msg="dX")
    assert_close_scaled(host(dw0), dwr, err_msg="dw")
    assert_close_scaled(host(db0), dbr, err_msg="db")
    for (want_w, want_b), (dX, dw, db) in outs.items():
        assert torch.equal(dX, dX0), (want_w, want_b)
        assert torch.equal(dw, dw0) if want_w else bool((dw == 123.0).all()), (want_w, want_b)
        assert torch.equal(db, db0) if want_b else bool((db == 321.0).all()), (want_w, want_b)


def test_norm_backward_deferred_column_sums_interleaved(hip):
    """The mirror of test_rmsnorm_backward_deferred_column_sums for the queue that RMSNorm and LayerNorm share: inside one
    nnhipWeightGradDefer window their backward calls interleave -- LayerNorm with both, one and none of dW / dB.  The queue holds
    jobs of one width class: the 512-wide job flushes the 4096-wide one before it (another slice width), (33, 1000) joins the
    512-wide jobs (same slice width, vector), and the last job, 1001 wide (no multiple of 4: the scalar class), flushes them all
    while LayerNorm jobs are queued.  dX is there at once; the dW / dB of a queued job keep their sentinels until the queue is
    flushed (by that last job for the ones before it, by nnhipWeightGradFlush for the last one), and every output is then
    BIT-identical to the same calls outside the window."""
    import torch
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    rng = np.random.default_rng(62)
    st = get_current_stream_ptr()
    # (norm, rows, cols, dW, dB)
    specs = [("rms", 64, 4096, True, False), ("ln", 300, 512, True, True), ("rms", 300, 512, True, True),
             ("ln", 777, 512, True, False), ("ln", 64, 512, False, False), ("ln", 33, 1000, True, True), ("ln", 33, 1001, True, True)]
    jobs = []
    for norm, rows, cols, want_w, want_b in specs:
        X, dY = dev(rng.standard_normal((rows, cols)) * 1.3 + 0.2), dev(rng.standard_normal((rows, cols)))
        w = dev(rng.uniform(0.5, 1.5, cols))
        if norm == "rms":
            stats = (torch.sqrt((X * X).mean(dim=1) + 1e-6).contiguous(), None)
        else:
            stats = (X.mean(dim=1).contiguous(), (1.0 / torch.sqrt(X.var(dim=1, unbiased=False) + 1e-5)).contiguous())
        jobs.append((X, dY, w, stats))

    def sentinels_intact(outs):
        torch.cuda.synchronize()
        return all(bool((o == s).all()) for _, dw, db in outs for o, s in ((dw, 123.0), (db, 321.0)))

    def submit(outs, defer):
        for (norm, rows, cols, want_w, want_b), (X, dY, w, stats) in zip(specs, jobs):
            if defer and len(outs) == len(specs) - 1:
                assert sentinels_intact(outs[1:]), "a deferred column sum ran before the queue was flushed"
            dx = torch.full_like(X, float("nan"))
            dw, db = torch.full((cols,), 123.0, device="cuda"), torch.full((cols,), 321.0, device="cuda")
            pw, pb = dw if want_w else None, db if want_b else None
            if norm == "rms":
                call_hip_function("nnhipRMSNormBackward", dY, X, w, stats[0], None, dx, pw, pb, rows, cols, st)
            else:
                call_hip_function("nnhipLayerNormBackward", dY, X, w, stats[0], stats[1], dx, pw, pb, rows, cols, st)
            outs.append((dx, dw, db))
        if defer:
            assert sentinels_intact(outs[-1:]), "a deferred column sum ran before the flush"
            assert not any(bool(torch.isnan(dx).any()) for dx, _, _ in outs), "dX must not wait for the flush"

    def run(defer):
        outs = []
        if defer:
            call_hip_function("nnhipWeightGradDefer", 1, st)
        try:
            submit(outs, defer)
        finally:                              # a failed assertion must not leave the window open for the tests that follow
            if defer:
                call_hip_function("nnhipWeightGradFlush", st)
                call_hip_function("nnhipWeightGradDefer", 0, st)
            torch.cuda.synchronize()
        return outs

    a, b = run(True), run(False)
    for (dxa, dwa, dba), (dxb, dwb, dbb), (norm, rows, cols, want_w, want_b), (X, dY, w, stats) in zip(a, b, specs, jobs):
        assert torch.equal(dxa, dxb) and torch.equal(dwa, dwb) and torch.equal(dba, dbb), (norm, rows, cols)
        assert bool((dwa == 123.0).all()) != want_w and bool((dba == 321.0).all()) != want_b, (norm, rows, cols)
        if norm == "ln":
            dXr, dwr, dbr = layernorm_backward(layernorm_forward(host(X), host(w))[1], host(dY))
            assert_close_scaled(host(dxa), dXr, err_msg="dX")
            if want_w:
                assert_close_scaled(host(dwa), dwr, err_msg="dw")
            if want_b:
                assert_close_scaled(host(dba), dbr, err_msg="db")


# ------------------------------------------------------------------------------------------- the decode kernel
def decode_case(seed, B, H, dh, Tmax, lengths):
    """Random q|k|v rows and a cache whose rows hold lengths[b] live tokens; everything past the live length is NaN."""
    rng = np.random.default_rng(seed)
    D = H * dh
    qkv = rng.standard_normal((B, 3 * D)).astype(np.float32)
    K = rng.standard_normal((B, H, Tmax, dh)).astype(np.float32)
    V = rng.standard_normal((B, H, Tmax, dh)).astype(np.float32)
    for b, n in enumerate(lengths):
        K[b, :, n:] = np.nan
        V[b, :, n:] = np.nan
    return qkv, K, V


def decode_expect(qkv, K, V, lengths, H, dh, scale):
    """float64: the caches with the new token appended at index lengths[b], and the attention over keys 0 .. lengths[b]."""
    B, D = qkv.shape[0], H * dh
    K2, V2 = K.astype(np.float64), V.astype(np.float64)
    for b, n in enumerate(lengths):
        K2[b, :, n] = qkv[b, D:2 * D].reshape(H, dh)
        V2[b, :, n] = qkv[b, 2 * D:].reshape(H, dh)
    out = attention_decode(qkv[:, :D].reshape(B, H, dh), K2, V2, [n + 1 for n in lengths], scale)
    return out.reshape(B, D), K2, V2


def ragged_lengths(seed, B, Tmax):
    """cache_len per row: 0 (first token) and Tmax - 1 (last slot) are always there when the batch has room for both."""
    rng = np.random.default_rng(seed)
    n = [int(v) for v in rng.integers(0, Tmax, B)]
    n[0] = 0
    n[-1] = Tmax - 1 if B > 1 else n[-1]
    if B > 2:
        n[1] = 63                      # the last key of the first 64-key pass; the new token opens the next one
    return n


@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_attention_decode_vs_float64(hip, dh, B):
    import torch
    from neunet_hip.nn.experimental.causal_attention import KVCache, attention_decode as hip_decode
    H, Tmax = 4, 200
    scale = 1.0 / np.sqrt(dh)
    cases = [ragged_lengths(dh + B, B, Tmax)] + ([[Tmax - 1], [70]] if B == 1 else [])
    for lengths in cases:
        qkv, K, V = decode_case(dh * 100 + B, B, H, dh, Tmax, lengths)
        c = KVCache(B, Tmax, 1, H, dh)
        c.k[0].copy_(torch.from_numpy(K))
        c.v[0].copy_(torch.from_numpy(V))
        c.set_lengths(lengths)
        if c.workspace is not None:
            c.workspace.fill_(float("nan"))
        out = torch.full((B, H * dh), float("nan"), device="cuda")
        hip_decode(dev(qkv), c.layer(0), out, scale)
        ref, K2, V2 = decode_expect(qkv, K, V, lengths, H, dh, scale)
        got = host(out)
        assert np.isfinite(got).all(), "a key past the live length was read (NaN poison), or a row was not written"
        assert_close_scaled(got, ref, tol=1e-4, err_msg=f"O dh={dh} B={B} lengths={lengths[:4]}")
        # the appended rows are in the cache, bit for bit; every other cache word is what it was (NaN poison included)
        np.testing.assert_array_equal(host(c.k[0]), K2.astype(np.float32))
        np.testing.assert_array_equal(host(c.v[0]), V2.astype(np.float32))
        assert c.cache_len.tolist() == lengths, "the kernel must not change cache_len"
        # a second run (same lengths: the same slot is rewritten with the same values) is bit-identical
        out2 = torch.full_like(out, float("nan"))
        hip_decode(dev(qkv), c.layer(0), out2, scale)
        np.testing.assert_array_equal(host(out2).view(np.uint32), got.view(np.uint32))


def test_attention_decode_long_cache_and_row_stride(hip):
    """GPT-2 small's shape (12 heads of 64, Tmax 1024: 16 splits of 64 keys per head at batch 1, 2 of 512 at batch 64) through the C
    ABI directly, with qkv a column block of a wider buffer (ld_qkv > 3D)."""
    import torch
    from neunet_hip._lib import StridedView, call_hip_function, get_current_stream_ptr, load_hip_function
    H, dh, Tmax = 12, 64, 1024
    D = H * dh
    for B, lengths in ((1, [1023]), (1, [500]), (64, ragged_lengths(9, 64, Tmax))):
        qkv, K, V = decode_case(B, B, H, dh, Tmax, lengths)
        wide = torch.full((B, 3 * D + 8), float("nan"), device="cuda")
        wide[:, :3 * D].copy_(torch.from_numpy(qkv))
        Kd, Vd = dev(K), dev(V)
        nbytes = load_hip_function("nnhipAttentionDecodeWorkspace")(B, H, Tmax, dh)
        assert nbytes > 0
        ws = torch.full((nbytes // 4,), float("nan"), device="cuda")
        out = torch.full((B, D), float("nan"), device="cuda")
        cl = torch.tensor(lengths, dtype=torch.int32, device="cuda")
        call_hip_function("nnhipAttentionDecode", StridedView(wide), Kd, Vd, cl, out, ws, B, H, Tmax, dh, 3 * D + 8, 0.125,
                          get_current_stream_ptr())
        ref, K2, V2 = decode_expect(qkv, K, V, lengths, H, dh, 0.125)
        assert_close_scaled(host(out), ref, tol=1e-4, err_msg=f"O B={B}")
        np.testing.assert_array_equal(host(Kd), K2.astype(np.float32))
        np.testing.assert_array_equal(host(Vd), V2.astype(np.float32))


def test_attention_decode_full_cache_is_refused(hip):
    """cache_len[b] == Tmax: the row is refused -- the device error word is raised, nothing of that row is written (cache, output)
    and nothing outside the buffers is touched (NaN guard words around K, V, O and the workspace); the other row of the same
    launch is computed.  One call of a refusal the kernel was designed to make."""
    import torch
    from neunet_hip._lib import NeunetHipError, call_hip_function, get_current_stream_ptr, load_hip_function
    B, H, dh, Tmax = 2, 4, 64, 128
    D = H * dh
    lengths = [Tmax, 5]
    qkv, K, V = decode_case(77, B, H, dh, Tmax, [Tmax, 5])
    Kf, Vf, Of = Fenced(B, H, Tmax, dh), Fenced(B, H, Tmax, dh), Fenced(B, D)
    Kf.view.copy_(torch.from_numpy(K))
    Vf.view.copy_(torch.from_numpy(V))
    nbytes = load_hip_function("nnhipAttentionDecodeWorkspace")(B, H, Tmax, dh)
    Wf = Fenced(max(nbytes // 4, 4))
    cl = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    assert load_hip_function("nnhipDeviceError")() == 0
    try:
        call_hip_function("nnhipAttentionDecode", dev(qkv), Kf.view, Vf.view, cl, Of.view, Wf.view, B, H, Tmax, dh, 3 * D, 0.125,
                          get_current_stream_ptr())
        torch.cuda.synchronize()
        assert load_hip_function("nnhipDeviceError")() == -5
        with pytest.raises(NeunetHipError, match="KV-cache"):
            call_hip_function("nnhipDeviceError")
        with pytest.raises(NeunetHipError, match="status -5"):              # sticky: the next decode call is refused on the host
            call_hip_function("nnhipAttentionDecode", dev(qkv), Kf.view, Vf.view, cl, Of.view, Wf.view, B, H, Tmax, dh, 3 * D,
                              0.125, get_current_stream_ptr())
    finally:
        load_hip_function("nnhipClearDeviceError")()
    assert load_hip_function("nnhipDeviceError")() == 0
    for f in (Kf, Vf, Of, Wf):
        assert f.guards_intact(), "a refused row wrote outside a buffer"
    np.testing.assert_array_equal(Kf.host()[0], K[0])                       # the full row's cache: untouched
    np.testing.assert_array_equal(Vf.host()[0], V[0])
    assert np.isnan(Of.host()[0]).all()                                     # its output row: not written
    ref, K2, V2 = decode_expect(qkv[1:], K[1:], V[1:], [5], H, dh, 0.125)
    assert_close_scaled(Of.host()[1:], ref, tol=1e-4, err_msg="the other row")
    np.testing.assert_array_equal(Kf.host()[1:], K2.astype(np.float32))


def test_kv_cache_fill_moves_the_prompt(hip):
    import torch
    from neunet_hip.nn.experimental.causal_attention import KVCache, kv_cache_fill
    B, H, dh, T, Tmax = 3, 4, 32, 11, 40
    D = H * dh
    rng = np.random.default_rng(3)
    qkv = rng.standard_normal((B, T, 3 * D)).astype(np.float32)
    c = KVCache(B, Tmax, 2, H, dh)
    c.k.fill_(float("nan"))
    c.v.fill_(float("nan"))
    kv_cache_fill(dev(qkv), c.layer(1), T)
    k = host(c.k[1])
    np.testing.assert_array_equal(k[:, :, :T], qkv[:, :, D:2 * D].reshape(B, T, H, dh).transpose(0, 2, 1, 3))
    np.testing.assert_array_equal(host(c.v[1])[:, :, :T], qkv[:, :, 2 * D:].reshape(B, T, H, dh).transpose(0, 2, 1, 3))
    assert np.isnan(k[:, :, T:]).all() and np.isnan(host(c.k[0])).all()


def test_kv_cache_fill_offsets_null_lengths_and_refusal(hip):
    """nnhipKVCacheFill through the C ABI with ragged non-zero cache_len (tokens land at cache_len[b] + i), with cache_len NULL
    (offset 0), and with one row that has no room for T tokens: that row is skipped entirely, the others are written, the device
    error word is raised, and nothing outside the buffers is touched."""
    import torch
    from neunet_hip._lib import NeunetHipError, call_hip_function, get_current_stream_ptr, load_hip_function
    B, H, dh, T, Tmax = 3, 2, 64, 5, 16
    D = H * dh
    rng = np.random.default_rng(4)
    qkv = rng.standard_normal((B, T, 3 * D)).astype(np.float32)
    kref = qkv[:, :, D:2 * D].reshape(B, T, H, dh).transpose(0, 2, 1, 3)
    vref = qkv[:, :, 2 * D:].reshape(B, T, H, dh).transpose(0, 2, 1, 3)
    lengths = [3, 12, 11]                                   # row 1: 12 + 5 > 16, no room; row 2: 11 + 5 == 16, the last slots
    Kf, Vf = Fenced(B, H, Tmax, dh), Fenced(B, H, Tmax, dh)
    cl = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    assert load_hip_function("nnhipDeviceError")() == 0
    try:
        call_hip_function("nnhipKVCacheFill", dev(qkv), Kf.view, Vf.view, cl, B, H, T, Tmax, dh, 3 * D, get_current_stream_ptr())
        torch.cuda.synchronize()
        with pytest.raises(NeunetHipError, match="KV-cache"):
            call_hip_function("nnhipDeviceError")
    finally:
        load_hip_function("nnhipClearDeviceError")()
    assert Kf.guards_intact() and Vf.guards_intact()
    k, v = Kf.host(), Vf.host()
    for b, n in ((0, 3), (2, 11)):
        np.testing.assert_array_equal(k[b, :, n:n + T], kref[b])
        np.testing.assert_array_equal(v[b, :, n:n + T], vref[b])
        assert np.isnan(k[b, :, :n]).all() and np.isnan(k[b, :, n + T:]).all()
    assert np.isnan(k[1]).all() and np.isnan(v[1]).all()    # the refused row
    K0, V0 = Fenced(B, H, Tmax, dh), Fenced(B, H, Tmax, dh)
    call_hip_function("nnhipKVCacheFill", dev(qkv), K0.view, V0.view, None, B, H, T, Tmax, dh, 3 * D, get_current_stream_ptr())
    torch.cuda.synchronize()
    assert load_hip_function("nnhipDeviceError")() == 0 and K0.guards_intact() and V0.guards_intact()
    np.testing.assert_array_equal(K0.host()[:, :, :T], kref)
    np.testing.assert_array_equal(V0.host()[:, :, :T], vref)
    assert np.isnan(K0.host()[:, :, T:]).all()


# ------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def tiny(hip, golden):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import gpt2_infer as G
    f = golden("gpt2_tiny")
    hf, grads = load_parts("gpt2_tiny_hf"), load_parts("gpt2_tiny_grad")
    n_embd, n_head, n_layer, vocab, n_pos = (int(v) for v in f["cfg"])
    cfg = dict(n_embd=n_embd, n_head=n_head, n_layer=n_layer, vocab_size=vocab, n_positions=n_pos)
    np.random.seed(0)
    model = G.GPT2(cfg)
    G.load_gpt2_weights(model, hf)
    return dict(G=G, f=f, grads=grads, cfg=cfg, model=model, params=params_from_hf(hf, n_layer))


def test_gpt2_tiny_logits_and_gradients(hip, tiny):
    """The training path through LayerNorm, GELU and HIPCausalSelfAttention: logits, loss and the gradient of every parameter
    against the reference.  The reference's loader leaves lm_head an untied CLONE of wte (gpt2_infer.py:289) while this model keeps
    them tied, as GPT-2 is: the tied gradient is the sum of the reference's two."""
    import neunet_hip.nn as nn
    f, model = tiny["f"], tiny["model"]
    batch = f["batch"]
    model.train()
    for p in model.parameters():
        p.grad = None
    out = model(batch[:, :-1])
    np.testing.assert_allclose(host(out.data), f["logits"], **TOL)
    loss = nn.CrossEntropyLoss()(out.reshape(out.shape[0] * out.shape[1], out.shape[2]),
                                 hip.Tensor(batch[:, 1:].reshape(-1), dtype=np.int32, requires_grad=False, device="cuda"))
    assert abs(loss.item() - float(f["loss"])) < 1e-4
    loss.backward()
    ref = dict(tiny["grads"])
    ref["wte.weight"] = ref["wte.weight"] + ref.pop("lm_head.weight")
    scale = grad_list_scale(list(ref.values()))
    got = {}

    def walk(mod, prefix):
        for name, item in mod.__dict__.items():
            if item.__class__.__name__ == "Parameter":
                got[prefix + name] = item
            elif hasattr(item, "modules") and isinstance(item.modules, list):
                for i, m in enumerate(item.modules):
                    walk(m, f"{prefix}{name}.{i}.")
            elif hasattr(item, "state_dict"):
                walk(item, prefix + name + ".")

    walk(model, "")
    assert got.pop("lm_head.weight") is got["wte.weight"]
    assert sorted(got) == sorted(ref)
    for k, r in ref.items():
        g = got[k].grad
        assert g is not None, k
        # (softmax is shift-invariant: the key third of c_attn's bias gradient is mathematically zero -- rounding noise on both sides)
        assert_close_scaled(host(g).reshape(r.shape), r, err_msg=k, scale=scale if k.endswith("c_attn.bias") else 0.0)


def test_gpt2_tiny_teacher_forced_cached_decode(hip, tiny):
    """The fixture's 40 tokens fed one at a time through the KV cache (from an EMPTY cache: the first step runs the decode kernel
    with cache_len 0): the logits of every step against the float64 logits of that position."""
    f, model = tiny["f"], tiny["model"]
    model.eval()
    tokens = f["tokens"]
    cache = model.new_cache(1, 40)
    for t in range(40):
        logits = model(tokens[None, t:t + 1], cache=cache)
        assert_close_scaled(host(logits.data)[0, 0], f["logits64"][t], tol=1e-4, err_msg=f"step {t}")
    assert cache.tokens == 40 and cache.cache_len.tolist() == [40]
    # prefill + decode: the prompt in one causal pass, the rest token by token
    cache = model.new_cache(1, 40)
    logits = model(tokens[None, :8], cache=cache)
    assert_close_scaled(host(logits.data)[0], f["logits64"][:8], tol=1e-4, err_msg="prefill")
    for t in range(8, 40):
        logits = model(tokens[None, t:t + 1], cache=cache)
        assert_close_scaled(host(logits.data)[0, 0], f["logits64"][t], tol=1e-4, err_msg=f"step {t} after prefill")


@pytest.mark.parametrize("mode", ["recompute", "cached", "graph"])
def test_gpt2_tiny_generate_returns_the_fixture_tokens(hip, tiny, mode):
    f, G = tiny["f"], tiny["G"]
    stats = {}
    out = G.generate(tiny["model"], f["prompt"], 32, mode=mode, stats=stats)
    assert out.shape == (1, 40) and out.dtype == np.int32
    np.testing.assert_array_equal(out[0], f["tokens"])
    if mode == "graph":
        # the captured step is kernels only (no memcpy / host / empty node) and there is one replay per token after the first: nothing
        # in a step can hand a value to the host.  graph.count_graph_nodes on the captured hipGraph
        assert stats["replays"] == 31
        assert stats["kernel_nodes"] is not None and stats["kernel_nodes"] > 0
        assert stats["graph_nodes"] == stats["kernel_nodes"], stats


def test_gpt2_tiny_generate_batch_and_sampling(hip, tiny):
    """Batch 3 (the same prompt in every row: every row must be the fixture) in graph mode, and top-k sampling in the graph and the
    cached mode drawing the same tokens from the same seed (both read the logits on the host)."""
    f, G, model = tiny["f"], tiny["G"], tiny["model"]
    out = G.generate(model, np.tile(f["prompt"], (3, 1)), 32, mode="graph")
    for b in range(3):
        np.testing.assert_array_equal(out[b], f["tokens"])
    a = G.generate(model, f["prompt"], 12, temperature=0.9, top_k=5, mode="cached", seed=4)
    b = G.generate(model, f["prompt"], 12, temperature=0.9, top_k=5, mode="graph", seed=4)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a[0, 8:], f["tokens"][8:20])


def test_causal_self_attention_unfused_head_dim(hip):
    """A head dim outside FUSED_HEAD_DIMS (48) takes the GEMM + masked-softmax path: same maths, checked against float64 through
    the model restatement's attention block; a KV cache for it is an error, not a wrong answer."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(8)
    D, H, B, T = 96, 2, 2, 9
    np.random.seed(1)
    m = nn.CausalSelfAttention(D, H)
    X = rng.standard_normal((B, T, D)).astype(np.float32)
    dY = rng.standard_normal((B, T, D)).astype(np.float32)
    x = hip.Tensor(X, device="cuda")
    y = m(x)
    y.backward(dev(dY))
    Wa, ba = host(m.c_attn.weight.data).astype(np.float64), host(m.c_attn.bias.data).astype(np.float64).reshape(-1)
    Wp, bp = host(m.c_proj.weight.data).astype(np.float64), host(m.c_proj.bias.data).astype(np.float64).reshape(-1)
    qkv = X @ Wa.T + ba
    q, k, v = (qkv[..., j * D:(j + 1) * D].reshape(B, T, H, D // H).transpose(0, 2, 1, 3) for j in range(3))
    s = np.where(np.tril(np.ones((T, T), bool)), q @ k.transpose(0, 1, 3, 2) / np.sqrt(D // H), -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = (p @ v).transpose(0, 2, 1, 3).reshape(B, T, D) @ Wp.T + bp
    np.testing.assert_allclose(host(y.data), ref, **TOL)
    # backward in float64: c_proj, attention (softmax backward), c_attn
    dctx = (dY.astype(np.float64) @ Wp).reshape(B, T, H, D // H).transpose(0, 2, 1, 3)
    dp = dctx @ v.transpose(0, 1, 3, 2)
    ds = p * (dp - (dp * p).sum(-1, keepdims=True)) / np.sqrt(D // H)
    dq, dk, dv = ds @ k, ds.transpose(0, 1, 3, 2) @ q, p.transpose(0, 1, 3, 2) @ dctx
    dqkv = np.concatenate([t.transpose(0, 2, 1, 3).reshape(B, T, D) for t in (dq, dk, dv)], axis=-1)
    assert_close_scaled(host(x.grad), dqkv @ Wa, err_msg="dX")
    assert_close_scaled(host(m.c_attn.weight.grad), dqkv.reshape(-1, 3 * D).T @ X.reshape(-1, D).astype(np.float64), err_msg="dW c_attn")
    assert_close_scaled(host(m.c_proj.bias.grad).reshape(-1), dY.reshape(-1, D).sum(0), err_msg="db c_proj")
    with pytest.raises(ValueError, match="head dim 48"):
        nn.KVCache(B, 16, 1, H, D // H)
