"""GPU parity tests: every HIP kernel, called through the ctypes C-ABI, against the CPU oracle on the
same seeded inputs and against the committed golden vectors (generated from the real reference).

Mirrors the reference's CUDA tests one-to-one: same shapes, tolerances tightened where the
fp32 MFMA path allows (LinearSwish 1e-4 instead of the reference's TF32 1e-3).
Tolerances: fp32 outputs rtol=atol=1e-4 (north_star) unless a tighter one is written; argmax bit-exact.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import neunet_oracle as O  # noqa: E402  (checker only)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()  # fail loudly if the extension is missing
    return neunet_hip


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def T(hip, a, **kw):
    return hip.Tensor(a, device="cuda", **kw)


TOL = dict(rtol=1e-4, atol=1e-4)

# ---- error bounds that mean something ------------------------------------------------------------------------------
# north_star: "within 1e-4 fp32".  rtol = atol = 1e-4 (TOL) is that statement for tensors whose entries are O(1).  Two
# kinds of tensor need it restated rather than loosened (round-2 review: every atol above 1e-4 was unexplained):
#   * a dot product of K terms carries an fp32 rounding error proportional to sum_k |a_k||b_k| whatever its own value is
#     (cancellation): assert_dot_close() bounds |got - float64| by c * 2^-24 * sum|a||b| per element.  Measured on this
#     kernel (tools/gemm_accuracy.py, profiles/r02c_gemm_accuracy.txt): max 6.3 units for K up to 4096, uniform / normal
#     operands, in either GEMM mode; c = 32 leaves 5x head-room and is ~K/100 times tighter than the worst-case K * 2^-24;
#   * a gradient tensor whose entries span orders of magnitude (dW = sum over thousands of rows): assert_close_scaled()
#     holds every entry to 1e-4 of max(|its reference value|, the tensor's rms) -- pure 1e-4 relative for the entries that
#     matter, 1e-4 of the typical magnitude for the near-zero ones.
U24 = 2.0 ** -24


def dot_bound(A, B, c=32.0):
    """c * 2^-24 * (|A| @ |B|), elementwise; A (m, k), B (k, n)."""
    return c * U24 * (np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(B, np.float64)))


def assert_within(got, ref, bound, err_msg=""):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    if np.any(err > bound) or not np.all(np.isfinite(err)):
        ratio = err / np.maximum(bound, 1e-300)
        i = np.unravel_index(np.nanargmax(ratio), ratio.shape)
        raise AssertionError(f"{err_msg}: error {err[i]:.3e} is {ratio[i]:.2f} x the bound {bound[i]:.3e} at {i} "
                             f"({int(np.sum(err > bound))} of {err.size} entries over)")


def assert_dot_close(got, A, B, c=32.0, plus=None, err_msg=""):
    """got ~= A @ B (+ plus), against float64, within c * 2^-24 * sum|a||b| per element."""
    ref = np.asarray(A, np.float64) @ np.asarray(B, np.float64)
    if plus is not None:
        ref = ref + plus
    assert_within(got, ref, dot_bound(A, B, c) + 4 * U24 * np.abs(ref), err_msg)


def rms_of(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a ** 2))) if a.size else 0.0


def assert_close_scaled(got, ref, tol=1e-4, err_msg="", scale=0.0):
    """|got - ref| <= tol * max(|ref|, rms(ref), scale) per element.  `scale`: the magnitude the tensor WOULD have if its
    terms did not cancel, for tensors that are mathematically zero -- e.g. the bias gradient of attention's key projection
    (softmax is shift-invariant, so d/db_k is exactly 0 and both sides hold rounding noise of a sum over all rows); callers
    pass the natural scale of that sum (for a Linear fed unit-variance inputs: the rms of its weight gradient)."""
    ref = np.asarray(ref, np.float64)
    assert_within(got, ref, tol * np.maximum(np.maximum(np.abs(ref), rms_of(ref)), scale) + 1e-30, err_msg)


def grad_list_scale(refs):
    """Median rms of a model's gradient tensors: the `scale` for the mathematically-zero ones among them."""
    r = [rms_of(a) for a in refs if a is not None and np.size(a)]
    return float(np.median(r)) if r else 0.0


# ------------------------------------------------------------------------------------------- Linear
@pytest.mark.parametrize("name", ["linear_2d", "linear_3d", "linear_nobias"])
def test_linear_golden(hip, golden, name):
    g = golden(name)
    from neunet_hip.nn.experimental import HIPLinear
    layer = HIPLinear(24, 40, bias="b" in g)
    layer.weight.data.copy_(dev(g["W"]))
    if "b" in g:
        layer.bias.data.copy_(dev(g["b"]))
    x = T(hip, g["X"])
    out = layer(x)
    np.testing.assert_allclose(host(out.data), g["O"], rtol=1e-5, atol=1e-5)
    out.backward(g["dO"])
    np.testing.assert_allclose(host(x.grad), g["dX"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(layer.weight.grad), g["dW"], rtol=1e-5, atol=1e-5)
    if "b" in g:
        assert tuple(layer.bias.grad.shape) == (1, 40)
        np.testing.assert_allclose(host(layer.bias.grad), g["db"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("rows,inf,outf,bias", [
    (128, 256, 512, True),     # tests/test_linear_cuda.py:15-89
    (32, 784, 128, True),      # C1 layer 1
    (32, 128, 10, True),       # C1 layer 2: N=10 -> scalar-load edge path
    (200, 130, 70, False),     # nothing is a tile multiple, K%4 != 0
    (1, 8, 8, True),
    (513, 512, 300, True),     # M/N edges on a vector path
    (2048, 64, 64, True),      # dW reduction long enough to take split-K
])
def test_linear_vs_oracle(hip, rows, inf, outf, bias):
    from neunet_hip.nn.experimental import HIPLinear
    rng = np.random.default_rng(rows * 7 + inf)
    X = rng.uniform(-1, 1, (rows, inf)).astype(np.float32)
    W = rng.uniform(-0.1, 0.1, (outf, inf)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, (1, outf)).astype(np.float32) if bias else None
    dO = rng.uniform(-1, 1, (rows, outf)).astype(np.float32)
    layer = HIPLinear(inf, outf, bias=bias)
    layer.weight.data.copy_(dev(W))
    if bias:
        layer.bias.data.copy_(dev(b))
    x = T(hip, X)
    out = layer(x)
    np.testing.assert_allclose(host(out.data), O.linear_forward(X, W, b), **TOL)
    out.backward(dO)
    dX, dW, db = O.linear_backward(X, W, b, dO)
    np.testing.assert_allclose(host(x.grad), dX, **TOL)
    assert_close_scaled(host(layer.weight.grad), dW)
    if bias:
        assert_close_scaled(host(layer.bias.grad), db)


@pytest.mark.parametrize("rows,inf,outf", [
    (40, 40, 40),        # K = 40 = 32 + 8 in all three GEMMs: one whole k-tile + a shifted partial tile; single clamped tile
    (72, 136, 264),      # tails of 8 / 8 / 8, row clamps in both operands of every orientation
    (32, 32, 32),        # exactly one k-tile, no tail
    (1000, 520, 392),    # dW reduces over 1000 rows = 31 tiles + 8; forward tail 8, dX tail 8
    (6008, 64, 136),     # split-K dW whose LAST split is only a partial tile (6008 = 187 * 32 + 24)
    (130, 1000, 260),    # K = 1000 = 31 * 32 + 8 with M, N just past a tile edge
])
def test_gemm_fast_fetch_edges(hip, rows, inf, outf):
    """The vectorised GEMM kernels fetch through buffer descriptors with clamped rows and a shifted partial last k-tile
    (csrc/gemm_common.h): every orientation (forward k/k, dX k/outer, dW outer/outer with db from the row sums of dO) at
    sizes where K % 32 != 0, K % 8 == 0 and M, N are not tile multiples, against float64."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    import torch
    rng = np.random.default_rng(rows * 31 + inf * 7 + outf)
    st = get_current_stream_ptr()
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    W = (rng.standard_normal((outf, inf)) / np.sqrt(inf)).astype(np.float32)
    b = rng.standard_normal((1, outf)).astype(np.float32)
    dO = rng.standard_normal((rows, outf)).astype(np.float32)
    x, w, bb, do = (dev(a) for a in (X, W, b, dO))
    X64, W64, dO64 = X.astype(np.float64), W.astype(np.float64), dO.astype(np.float64)
    o = torch.empty((rows, outf), device="cuda")
    call("nnhipLinearModuleForward", x, w, bb, o, rows, inf, outf, st)
    assert_dot_close(host(o), X64, W64.T, plus=b, err_msg="forward")
    dx, dw, db = torch.empty((rows, inf), device="cuda"), torch.empty((outf, inf), device="cuda"), torch.empty((1, outf), device="cuda")
    call("nnhipLinearModuleBackward", x, w, do, dx, dw, db, rows, inf, outf, st)
    assert_dot_close(host(dx), dO64, W64, err_msg="dX")
    assert_dot_close(host(dw), dO64.T, X64, err_msg="dW")
    assert_dot_close(host(db), np.ones((1, rows)), dO64, err_msg="db")


@pytest.mark.parametrize("rows,inf,outf", [(8192, 64, 1100), (8192, 512, 1100), (16384, 96, 520), (4096, 992, 2200)])
def test_gemm_persistent_forward(hip, rows, inf, outf):
    """csrc/gemm_pst.hip: a forward Linear whose grid has more 128x128 tiles than resident slots (and K <= 1024, K % 32 == 0,
    rows % 128 == 0) runs the persistent kernel -- one k-step stream across a block's tiles, the finished tile's stores inside the
    next tile's first step.  Against float64, and BIT-IDENTICAL to the classic kernel, which the same rows take when they
    are computed in chunks small enough to stay under the slot count (same k order, same fmaf chain; K < 1024 so that no
    chunk takes the classic kernel's split-K, which sums in a different order)."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    import torch
    rng = np.random.default_rng(rows + inf + outf)
    st = get_current_stream_ptr()
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    W = (rng.standard_normal((outf, inf)) / np.sqrt(inf)).astype(np.float32)
    b = rng.standard_normal((1, outf)).astype(np.float32)
    x, w, bb = dev(X), dev(W), dev(b)
    o = torch.full((rows, outf), float("nan"), device="cuda")
    call("nnhipLinearModuleForward", x, w, bb, o, rows, inf, outf, st)
    got = host(o)
    assert_dot_close(got, X, W.T, plus=b)
    tiles_n = -(-outf // 128)
    chunk = max(128, (400 // tiles_n) * 128)
    chunk = -(-(-(-rows // -(-rows // chunk))) // 128) * 128   # <= 400 tiles per call: the classic kernel; even chunks (a short last one would take split-K)
    o2 = torch.full((rows, outf), float("nan"), device="cuda")
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        call("nnhipLinearModuleForward", x[r0:r0 + n], w, bb, o2[r0:r0 + n], n, inf, outf, st)
    np.testing.assert_array_equal(got, host(o2))


@pytest.mark.parametrize("rows,inf,outf,beta,save", [(8192, 96, 1100, 1.0, 1), (16384, 512, 2048, 1.0, 1), (8192, 128, 1100, 1.5, 0),
                                                     (4096, 992, 2200, 0.7, 1)])
def test_gemm_persistent_swish(hip, rows, inf, outf, beta, save):
    """The fused Linear->Swish forward (nnhipLinearSwishForward, with and without the saved pre-activation) on the persistent
    kernel's Swish epilogue: against the float64 oracle formula, and BIT-IDENTICAL (both outputs) to the classic kernel's
    epilogue, which row chunks under the slot count take."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    import torch
    rng = np.random.default_rng(rows + inf + outf)
    st = get_current_stream_ptr()
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    W = (rng.standard_normal((outf, inf)) / np.sqrt(inf)).astype(np.float32)
    b = rng.standard_normal((1, outf)).astype(np.float32)
    x, w, bb = dev(X), dev(W), dev(b)
    o = torch.full((rows, outf), float("nan"), device="cuda")
    z = torch.full((rows, outf), float("nan"), device="cuda")
    call("nnhipLinearSwishForward", x, w, bb, o, z if save else None, rows, inf, outf, beta, save, st)
    z64 = X.astype(np.float64) @ W.astype(np.float64).T + b
    sig = 1.0 / (1.0 + np.exp(-beta * z64))
    zb = dot_bound(X, W.T) + 4 * U24 * np.abs(z64)             # bound on z; swish'(z) carries it into the output
    assert_within(host(o), z64 * sig, zb * (np.abs(sig) + np.abs(beta * z64 * sig * (1 - sig))) + 16 * U24 * np.abs(z64 * sig), "swish(z)")
    if save:
        assert_within(host(z), z64, zb, "z")
    else:
        assert bool(torch.isnan(z).all())                      # nothing may be written without save_preactivation
    tiles_n = -(-outf // 128)
    chunk = max(128, (400 // tiles_n) * 128)
    chunk = -(-(-(-rows // -(-rows // chunk))) // 128) * 128   # even chunks: a short last one (<= 64 tiles) would take split-K
    o2, z2 = torch.empty_like(o), torch.empty_like(z)
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        call("nnhipLinearSwishForward", x[r0:r0 + n], w, bb, o2[r0:r0 + n], z2[r0:r0 + n] if save else None, n, inf, outf, beta,
             save, st)
    assert torch.equal(o, o2)
    if save:
        assert torch.equal(z, z2)


@pytest.mark.parametrize("rows,inf,outf,beta", [(16384, 512, 2048, 1.0), (8192, 96, 1100, 1.3), (200, 64, 256, 0.8), (16384, 128, 128, 1.0)])
def test_linear_swish_saved_derivative(hip, rows, inf, outf, beta):
    """ABI 210: nnhipLinearSwishForward(save_preactivation = 2) leaves D = swish'(z) = s + beta z s (1 - s) in `preact` (the
    reference saves z, linear_swish_cutlass.py:68-98; its backward -- activations.py:223-232 -- needs nothing but this product's
    factor), and nnhipLinearInputGradScaled / nnhipLinearSwishBackward(recompute_preactivation = 2) multiply by it.  Against
    float64; the persistent kernel's epilogues (EPI 3 / EPI 4, 16384-row cases) BIT-IDENTICAL to the classic kernel's (row chunks
    under the slot count); the output O equal to the z-saving mode's bit for bit."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    rng = np.random.default_rng(rows + inf + outf)
    st = get_current_stream_ptr()
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    W = (rng.standard_normal((outf, inf)) / np.sqrt(inf)).astype(np.float32)
    b = rng.standard_normal((1, outf)).astype(np.float32)
    x, w, bb = dev(X), dev(W), dev(b)
    o, d = torch.full((rows, outf), float("nan"), device="cuda"), torch.full((rows, outf), float("nan"), device="cuda")
    o1, z1 = torch.empty_like(o), torch.empty_like(o)
    call("nnhipLinearSwishForward", x, w, bb, o, d, rows, inf, outf, beta, 2, st)
    call("nnhipLinearSwishForward", x, w, bb, o1, z1, rows, inf, outf, beta, 1, st)
    assert torch.equal(o, o1)
    z64 = X.astype(np.float64) @ W.astype(np.float64).T + b
    sig = 1.0 / (1.0 + np.exp(-beta * z64))
    d64 = sig + beta * z64 * sig * (1 - sig)
    zb = dot_bound(X, W.T) + 4 * U24 * np.abs(z64)
    # |dD/dz| <= beta (2 + beta |z|) / 4 ... bounded by beta (1 + |beta z|): z's error carried through, plus a few ulp of the evaluation
    assert_within(host(d), d64, zb * beta * (1 + np.abs(beta * z64)) + 32 * U24 * (1 + np.abs(d64)), "swish'(z)")
    # chunks under the slot count take the classic kernel: same bits
    tiles_n = -(-outf // 128)
    chunk = max(128, (400 // tiles_n) * 128)
    chunk = -(-(-(-rows // -(-rows // chunk))) // 128) * 128
    o2, d2 = torch.empty_like(o), torch.empty_like(d)
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        call("nnhipLinearSwishForward", x[r0:r0 + n], w, bb, o2[r0:r0 + n], d2[r0:r0 + n], n, inf, outf, beta, 2, st)
    assert torch.equal(o, o2) and torch.equal(d, d2)
    # backward: the next layer's input gradient times D, in place over D (EPI 4 at 16384 rows) and out of place
    outf2 = 512 if rows == 16384 and outf == 2048 else 96
    dO = rng.standard_normal((rows, outf2)).astype(np.float32)
    W2 = (rng.standard_normal((outf2, outf)) / np.sqrt(outf2)).astype(np.float32)
    ddo, w2 = dev(dO), dev(W2)
    dx64 = dO.astype(np.float64) @ W2.astype(np.float64)
    want = dx64 * host(d).astype(np.float64)
    inpl, outp = d.clone(), torch.empty_like(d)
    call("nnhipLinearInputGradScaled", ddo, w2, inpl, inpl, rows, outf, outf2, st)
    call("nnhipLinearInputGradScaled", ddo, w2, d, outp, rows, outf, outf2, st)
    assert torch.equal(inpl, outp)
    assert_within(host(outp), want, dot_bound(dO, W2) * np.abs(host(d)) + 8 * U24 * np.abs(want), "dX * D")
    o3 = torch.empty_like(d)
    tiles_n = -(-outf // 128)
    chunk = max(128, (400 // tiles_n) * 128)
    chunk = -(-(-(-rows // -(-rows // chunk))) // 128) * 128
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        call("nnhipLinearInputGradScaled", ddo[r0:r0 + n], w2, d[r0:r0 + n], o3[r0:r0 + n], n, outf, outf2, st)
    assert torch.equal(outp, o3)
    # ... and the unfolded backward entry with tmp = D equals the z-saving one to rounding (dZ = dO * swish'(z))
    g = dev(rng.standard_normal((rows, outf)).astype(np.float32))
    t2, t1 = d.clone(), z1.clone()
    dX2, dW2, db2 = torch.empty_like(x), torch.empty_like(w), torch.empty_like(bb)
    dX1, dW1, db1 = torch.empty_like(x), torch.empty_like(w), torch.empty_like(bb)
    call("nnhipLinearSwishBackward", x, w, bb, g, t2, dX2, dW2, db2, rows, inf, outf, beta, 2, st)
    call("nnhipLinearSwishBackward", x, w, bb, g, t1, dX1, dW1, db1, rows, inf, outf, beta, 0, st)
    np.testing.assert_allclose(host(t2), host(t1), rtol=2e-5, atol=2e-6)
    assert_close_scaled(host(dX2), host(dX1))
    assert_close_scaled(host(dW2), host(dW1))


@pytest.mark.parametrize("rows,inf,outf,inplace", [(8192, 1100, 160, True), (16384, 2048, 512, True), (8192, 1100, 192, False),
                                                   (4096, 2200, 992, True)])
def test_gemm_persistent_input_grad(hip, rows, inf, outf, inplace):
    """The input-gradient layout (B = W outer-major) on the persistent kernel: plain dX = dO W, and
    nnhipLinearInputGradSwish's dZ = (dO W) * swish'(z) -- in place over z, as the fused Linear->Swish backward uses it, and
    out of place -- whose z values are fetched a k-step ahead of the quarter of the tile they scale.  Against float64, and
    BIT-IDENTICAL to the classic kernel (row chunks under the slot count)."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    import torch
    rng = np.random.default_rng(rows + inf + outf)
    st = get_current_stream_ptr()
    beta = 1.25
    dO = rng.standard_normal((rows, outf)).astype(np.float32)
    W = (rng.standard_normal((outf, inf)) / np.sqrt(outf)).astype(np.float32)
    Z = rng.standard_normal((rows, inf)).astype(np.float32) * 2
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    g, w, x = dev(dO), dev(W), dev(X)
    tiles_n = -(-inf // 128)
    chunk = max(128, (400 // tiles_n) * 128)
    chunk = -(-(-(-rows // -(-rows // chunk))) // 128) * 128   # even chunks: a short last one (<= 64 tiles) would take split-K
    dx64 = dO.astype(np.float64) @ W.astype(np.float64)
    # plain dX
    dx = torch.full((rows, inf), float("nan"), device="cuda")
    call("nnhipLinearModuleBackward", x, w, g, dx, None, None, rows, inf, outf, st)
    assert_dot_close(host(dx), dO, W, err_msg="dX")
    dx2 = torch.empty_like(dx)
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        call("nnhipLinearModuleBackward", x[r0:r0 + n], w, g[r0:r0 + n], dx2[r0:r0 + n], None, None, n, inf, outf, st)
    assert torch.equal(dx, dx2)
    # dZ = dX * swish'(z)
    z = dev(Z)
    dz = z.clone() if inplace else torch.full((rows, inf), float("nan"), device="cuda")
    call("nnhipLinearInputGradSwish", g, w, dz if inplace else z, dz, rows, inf, outf, beta, st)
    s64 = 1.0 / (1.0 + np.exp(-beta * Z.astype(np.float64)))
    f64 = Z * s64
    sp64 = beta * f64 + s64 * (1 - beta * f64)          # swish'(z): v_exp / v_rcp in the epilogue, a few ulp of its own
    spmag = np.abs(beta * f64) + s64 * (1 + np.abs(beta * f64))   # magnitude of swish's terms: they cancel where swish' ~ 0
    assert_within(host(dz), dx64 * sp64, dot_bound(dO, W) * np.abs(sp64) + 16 * U24 * np.abs(dx64) * spmag, "dX * swish'")
    dz2 = z.clone()
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        call("nnhipLinearInputGradSwish", g[r0:r0 + n], w, dz2[r0:r0 + n], dz2[r0:r0 + n], n, inf, outf, beta, st)
    assert torch.equal(dz, dz2)


@pytest.mark.parametrize("rows,inf,outf", [(32, 128, 10), (256, 784, 10), (37, 50, 33), (100, 40, 260), (2048, 1024, 384)])
@pytest.mark.parametrize("kind", [1, 2])
def test_linear_backward_act(hip, rows, inf, outf, kind):
    """nnhipLinearModuleBackwardAct: dZ = (dO W) * act'(arg), dW = dO^T X, db from one call -- for small layers from ONE launch
    (gemm_small_pair_kernel).  Against float64, and dZ bit-identical to nnhipLinearInputGradSwish / ReLU (the same tiles in a
    separate launch); dW / db equal to nnhipLinearModuleBackward(dX = NULL)'s up to the summation order."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    import torch
    rng = np.random.default_rng(rows + inf + outf + kind)
    st = get_current_stream_ptr()
    beta = 1.3
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    W = (rng.standard_normal((outf, inf)) / np.sqrt(inf)).astype(np.float32)
    dO = rng.standard_normal((rows, outf)).astype(np.float32)
    A = rng.standard_normal((rows, inf)).astype(np.float32)              # z (swish) or the ReLU output f
    if kind == 2:
        A = np.maximum(A, 0)
    x, w, g, a = dev(X), dev(W), dev(dO), dev(A)
    dz = a.clone() if kind == 1 else torch.full((rows, inf), float("nan"), device="cuda")
    dw = torch.full((outf, inf), float("nan"), device="cuda")
    db = torch.full((outf,), float("nan"), device="cuda")
    call("nnhipLinearModuleBackwardAct", x, w, g, dz if kind == 1 else a, kind, beta, dz, dw, db, rows, inf, outf, st)
    dx64 = dO.astype(np.float64) @ W.astype(np.float64)
    if kind == 1:
        s64 = 1.0 / (1.0 + np.exp(-beta * A.astype(np.float64)))
        f64 = A * s64
        want = dx64 * (beta * f64 + s64 * (1 - beta * f64))
    else:
        want = dx64 * (A > 0)
    if kind == 1:
        fac, facmag = np.abs(beta * f64 + s64 * (1 - beta * f64)), np.abs(beta * f64) + s64 * (1 + np.abs(beta * f64))
    else:
        fac = facmag = (A > 0).astype(np.float64)
    assert_within(host(dz), want, dot_bound(dO, W) * fac + 16 * U24 * np.abs(dx64) * facmag, "dZ")
    assert_dot_close(host(dw), dO.T, X, err_msg="dW")
    assert_dot_close(host(db).reshape(1, -1), np.ones((1, rows)), dO, err_msg="db")
    dz2 = a.clone() if kind == 1 else torch.empty_like(dz)
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    if kind == 1:
        call("nnhipLinearInputGradSwish", g, w, dz2, dz2, rows, inf, outf, beta, st)
    else:
        call("nnhipLinearInputGradReLU", g, w, a, dz2, rows, inf, outf, st)
    call("nnhipLinearModuleBackward", x, w, g, None, dw2, db2, rows, inf, outf, st)
    assert torch.equal(dz, dz2)
    # (the pair launch gives both problems the larger of their two wave counts: dW / db can differ from the separate launch in
    # the order their K partial sums meet)
    np.testing.assert_allclose(host(dw), host(dw2), rtol=1e-5, atol=1e-6 * np.sqrt(rows))
    np.testing.assert_allclose(host(db), host(db2), rtol=1e-5, atol=1e-6 * np.sqrt(rows))


@pytest.mark.parametrize("rows,inf,outf", [(300, 96, 200), (128, 512, 512), (37, 50, 33), (4096, 1024, 128)])
def test_linear_addend_extensions(hip, rows, inf, outf):
    """nnhipLinearModuleForwardEx / BackwardEx: O = XW^T + b + R and dX = dO W + G from the GEMM epilogue (also through
    the split-K reduce and the scalar epilogue), db produced by the dW GEMM; host level: residual= and the folding of a
    gradient X already holds give exactly what `x + linear(h)` and Tensor.apply_grad's accumulation give."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(rows + inf)
    lin = nn.Linear(inf, outf)
    W, b = host(lin.weight.data), host(lin.bias.data)
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    R = rng.standard_normal((rows, outf)).astype(np.float32)
    dY = rng.standard_normal((rows, outf)).astype(np.float32)
    G = rng.standard_normal((rows, inf)).astype(np.float32)
    x, r = T(hip, X), T(hip, R)
    x.grad = dev(G)                                   # a gradient x received earlier in the backward pass
    y = lin(x, residual=r)
    np.testing.assert_allclose(host(y.data), O.linear_forward(X, W, b) + R, **TOL)
    y.backward(dY)
    dX, dW, db = O.linear_backward(X, W, b, dY)
    assert_close_scaled(host(x.grad), dX + G)
    np.testing.assert_allclose(host(r.grad), dY, rtol=0, atol=0)
    assert_close_scaled(host(lin.weight.grad), dW)
    assert_close_scaled(host(lin.bias.grad), db.reshape(1, -1))


def test_linear_entry_points_fuzz(hip):
    """40 random (rows, in, out) triples through every Linear entry point and epilogue option -- forward (+addend),
    backward (dX +addend, dW, db: inside the dW GEMM or by the column-sum pass), the Swish-folding dX -- covering the
    float4 and scalar epilogues (sizes not divisible by 4), split-K (few tiles, long or short K), single-tile and
    multi-tile grids.  Reference: float64 NumPy."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    import torch
    rng = np.random.default_rng(2024)
    st = get_current_stream_ptr()
    sizes = [1, 2, 3, 4, 7, 8, 31, 32, 33, 64, 100, 128, 129, 200, 256, 300, 512, 640, 1000, 1024, 1500, 2048, 2500]
    for case in range(40):
        rows, inf, outf = (int(rng.choice(sizes)) for _ in range(3))
        if case % 5 == 0:
            rows = int(rng.choice([4096, 6000]))            # long reductions for dW -> split-K with few tiles
        X = rng.standard_normal((rows, inf)).astype(np.float32)
        W = (rng.standard_normal((outf, inf)) / np.sqrt(inf)).astype(np.float32)
        b = rng.standard_normal((1, outf)).astype(np.float32)
        R = rng.standard_normal((rows, outf)).astype(np.float32)
        dO = rng.standard_normal((rows, outf)).astype(np.float32)
        G = rng.standard_normal((rows, inf)).astype(np.float32)
        Z = rng.standard_normal((rows, inf)).astype(np.float32)
        x, w, bb, r, do, gg, zz = (dev(a) for a in (X, W, b, R, dO, G, Z))
        X64, W64, dO64 = X.astype(np.float64), W.astype(np.float64), dO.astype(np.float64)
        tag = f"case {case}: rows {rows} in {inf} out {outf}"
        # forward, with and without addend
        o = torch.empty((rows, outf), device="cuda")
        call("nnhipLinearModuleForward", x, w, bb, o, rows, inf, outf, st)
        ref = X64 @ W64.T + b
        assert_within(host(o), ref, dot_bound(X, W.T) + 4 * U24 * np.abs(ref), tag + " fwd")
        call("nnhipLinearModuleForwardEx", x, w, None, r, o, rows, inf, outf, st)
        assert_within(host(o), ref - b + R, dot_bound(X, W.T) + 4 * U24 * (np.abs(ref) + np.abs(R)), tag + " fwd+addend")
        # backward: everything, then dX with an addend, then db alone (column-sum pass)
        dx, dw, db = torch.empty((rows, inf), device="cuda"), torch.empty((outf, inf), device="cuda"), torch.empty((1, outf), device="cuda")
        call("nnhipLinearModuleBackward", x, w, do, dx, dw, db, rows, inf, outf, st)
        dXr, dWr, dbr = dO64 @ W64, dO64.T @ X64, dO64.sum(0, keepdims=True)
        assert_within(host(dx), dXr, dot_bound(dO, W) + 4 * U24 * np.abs(dXr), tag + " dX")
        assert_dot_close(host(dw), dO.T, X, err_msg=tag + " dW")
        assert_dot_close(host(db), np.ones((1, rows)), dO, err_msg=tag + " db")
        call("nnhipLinearModuleBackwardEx", x, w, do, gg, dx, None, None, rows, inf, outf, st)
        assert_within(host(dx), dXr + G, dot_bound(dO, W) + 4 * U24 * (np.abs(dXr) + np.abs(G)), tag + " dX+addend")
        db.zero_()
        call("nnhipLinearModuleBackward", x, w, do, None, None, db, rows, inf, outf, st)
        assert_dot_close(host(db), np.ones((1, rows)), dO, err_msg=tag + " db alone")
        # Swish backward folded into dX, in place over z
        beta = 1.3
        sg = 1.0 / (1.0 + np.exp(-beta * Z.astype(np.float64)))
        f = Z * sg
        dzr = dXr * (beta * f + sg * (1 - beta * f))
        call("nnhipLinearInputGradSwish", do, w, zz, zz, rows, inf, outf, beta, st)
        sp = beta * f + sg * (1 - beta * f)
        spmag = np.abs(beta * f) + sg * (1 + np.abs(beta * f))
        assert_within(host(zz), dzr, dot_bound(dO, W) * np.abs(sp) + 16 * U24 * np.abs(dXr) * spmag, tag + " dX*swish'")


@pytest.mark.parametrize("save_derivative", [True, False])
@pytest.mark.parametrize("rows,dm,dff,beta", [(200, 64, 256, 1.0), (16384, 128, 128, 1.0), (50, 30, 70, 1.7), (16384, 512, 2048, 1.0)])
def test_ffn_swish_backward_folded_into_dx(hip, monkeypatch, rows, dm, dff, beta, save_derivative):
    """fc_2(LinearSwish fc_1(x)): fc_2's dX GEMM applies swish'(z) in its epilogue (nnhipLinearInputGradSwish, in place
    over the saved z; also through split-K and the scalar epilogue) and hands dz to fc_1 -- same gradients as the
    oracle's Linear -> Swish -> Linear chain; a second consumer of h disables the folding."""
    import neunet_hip.nn as nn
    from neunet_hip.nn.experimental import linear_swish as LS
    # what the forward keeps for the backward: swish'(z) (the default since round 6: the fold is one multiply) or z
    monkeypatch.setattr(LS, "_SAVE_DERIVATIVE", save_derivative)
    rng = np.random.default_rng(rows + dff)
    fc1, fc2 = nn.LinearSwish(dm, dff, swish_beta=beta), nn.Linear(dff, dm)
    W1, b1, W2, b2 = [host(t.data) for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
    X = rng.standard_normal((rows, dm)).astype(np.float32)
    dY = rng.standard_normal((rows, dm)).astype(np.float32)
    z = O.linear_forward(X, W1, b1)
    h = O.swish_forward(z, beta)
    dh, dW2, db2 = O.linear_backward(h, W2, b2, dY)
    dz = O.swish_backward(z, dh, beta)
    dX, dW1, db1 = O.linear_backward(X, W1, b1, dz)
    for second_consumer in (False, True):
        for p in (fc1.weight, fc1.bias, fc2.weight, fc2.bias):
            p.grad = None
        x = T(hip, X)
        hh = fc1(x)
        assert hh.args[8] == (2 if save_derivative else 1)
        y = fc2(hh)
        if second_consumer:
            y2 = fc2(hh)                      # h consumed twice: plain path, gradients accumulate
            (y + y2).backward(dY * 0.5)
        else:
            y.backward(dY)
        assert_close_scaled(host(x.grad), dX)
        assert_close_scaled(host(fc1.weight.grad), dW1)
        assert_close_scaled(host(fc1.bias.grad), db1.reshape(1, -1))
        assert_close_scaled(host(fc2.weight.grad), dW2)
        assert_close_scaled(host(fc2.bias.grad), db2.reshape(1, -1))


@pytest.mark.parametrize("rows,cols", [(64, 512), (33, 100), (16, 4096), (8, 12000)])
def test_rmsnorm_backward_addend(hip, rows, cols):
    import neunet_hip.nn as nn
    rng = np.random.default_rng(rows + cols)
    X = rng.standard_normal((rows, cols)).astype(np.float32)
    dY = rng.standard_normal((rows, cols)).astype(np.float32)
    G = rng.standard_normal((rows, cols)).astype(np.float32)
    norm = nn.RMSNorm(cols)
    norm.weight.data.copy_(dev(rng.standard_normal(cols).astype(np.float32)))
    w = host(norm.weight.data)
    x = T(hip, X)
    x.grad = dev(G)
    y = norm(x)
    y.backward(dY)
    dX, dw, _ = O.rmsnorm_backward(X, w, False, dY, 1e-6)
    np.testing.assert_allclose(host(x.grad), dX + G, rtol=1e-4, atol=1e-4)
    assert_close_scaled(host(norm.weight.grad), dw)


@pytest.mark.parametrize("rows,inf,hid,outf", [(32, 784, 128, 10), (37, 50, 33, 7), (256, 300, 64, 16), (5, 16, 16, 1)])
def test_mlp_chain_backward_one_launch(hip, rows, inf, hid, outf):
    """Linear2(relu(Linear1(x))) with x needing no gradient: nnhipLinearReLULinearBackward produces dW2, db2, dW1, db1 in one
    launch (dZ formed inside the dW1 tiles).  Against the oracle, and against the general two-launch path (NNHIP_MLP_CHAIN off):
    dW2 / db2 bit-identical (same tile code), dW1 / db1 to 1e-6 (dZ's 10-term dot products are summed in a different order)."""
    from neunet_hip.nn.experimental import HIPLinear, HIPReLU
    from neunet_hip.nn.experimental import linear as L
    rng = np.random.default_rng(rows + hid)
    X = rng.uniform(-1, 1, (rows, inf)).astype(np.float32)
    dY = rng.standard_normal((rows, outf)).astype(np.float32)
    l1, l2, relu = HIPLinear(inf, hid), HIPLinear(hid, outf), HIPReLU()
    W1, b1, W2, b2 = (host(t.data) for t in (l1.weight, l1.bias, l2.weight, l2.bias))
    res = {}
    for chain in (True, False):
        old, L._MLP_CHAIN = L._MLP_CHAIN, chain
        try:
            for t in (l1.weight, l1.bias, l2.weight, l2.bias):
                t.grad = None
            x = T(hip, X, requires_grad=False)
            y = l2(relu(l1(x)))
            n0 = None
            y.backward(dY)
            res[chain] = [host(t.grad).copy() for t in (l1.weight, l1.bias, l2.weight, l2.bias)]
        finally:
            L._MLP_CHAIN = old
    z = O.linear_forward(X, W1, b1)
    h = O.relu_forward(z)
    dh, dW2, db2 = O.linear_backward(h, W2, b2, dY)
    dz = O.relu_backward(h, dh)
    _, dW1, db1 = O.linear_backward(X, W1, b1, dz)
    for got, ref in zip(res[True], (dW1, db1, dW2, db2)):
        assert_close_scaled(got, ref)
    np.testing.assert_array_equal(res[True][2], res[False][2])
    np.testing.assert_array_equal(res[True][3], res[False][3])
    assert_close_scaled(res[True][0], res[False][0], tol=1e-5)
    assert_close_scaled(res[True][1], res[False][1], tol=1e-5)
    # with an input that DOES need its gradient the chain must not be taken (dX1 would be missing)
    x = T(hip, X)
    for t in (l1.weight, l1.bias, l2.weight, l2.bias):
        t.grad = None
    l2(relu(l1(x))).backward(dY)
    np.testing.assert_allclose(host(x.grad), O.linear_backward(X, W1, b1, dz)[0], **TOL)


@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("opt_name", ["Adam", "AdamW"])
def test_mlp_optimizer_in_backward_is_bit_identical(hip, graphed, opt_name, monkeypatch):
    """The README quick-start MLP's one-launch backward also applies Adam / AdamW to the four parameters (W1 / b1 by the thread
    that produced the gradient element; W2 / b2 -- inputs of the same launch -- by the last block to finish, from agent-scope
    published gradients).  Three ways to get there -- the DEFAULT path (the backward launch waits for optimizer.step(), round 5),
    optimizer.fuse_backward(True) (launched inside backward()), and the default path with somebody reading a gradient in between
    (plain backward at that moment + separate Adam launch) -- against backward and Adam as two launches (NNHIP_AUTO_FUSE_STEP=0).
    Same arithmetic on the same gradients: parameters, m, v and the gradients after 5 steps (an LR change in between) are
    BIT-IDENTICAL, eager and replayed."""
    import neunet_hip.nn as nn
    import neunet_hip.nn.experimental.linear as L
    from neunet_hip import optim
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    rng = np.random.default_rng(8)
    Xs = rng.uniform(-1, 1, (6, 32, 784)).astype(np.float32)
    Ys = rng.integers(0, 10, (6, 32)).astype(np.int32)

    def run(mode):
        np.random.seed(11)
        monkeypatch.setattr(L, "_AUTO_FUSE_STEP", mode != "two-launches")

        class MLP(nn.Module):
            def __init__(self):
                super().__init__()
                self.l1, self.relu, self.l2 = nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)

            def forward(self, x):
                return self.l2(self.relu(self.l1(x)))

        model = MLP()
        ps = model.parameters()
        opt = getattr(optim, opt_name)(ps, lr=1e-3, weight_decay=1e-2)
        if mode == "opt-in":
            opt.fuse_backward(True)
        x = T(hip, Xs[0], requires_grad=False)
        y = T(hip, Ys[0], dtype=np.int32, requires_grad=False)
        loss_fn = nn.CrossEntropyLoss()
        seen = []

        def fb():
            loss = loss_fn(model(x), y)
            loss.backward()
            seen.append((ps[0]._pending is not None, bool(opt._stepped_in_backward)))
            if mode == "peek":
                assert ps[2].grad is not None and ps[0]._pending is None    # the read ran the plain backward
            return loss

        step = None
        if graphed:
            step = GraphedTrainStep(fb, opt, GradBucket(ps), warmup=1)
        losses = []
        for s_ in range(5):
            x.data.copy_(dev(Xs[s_ + 1]))
            y.data.copy_(dev(Ys[s_ + 1]))
            if s_ == 3:
                opt.lr = 5e-4
            if graphed:
                losses.append(step().item())
            else:
                opt.zero_grad()
                losses.append(fb().item())
                opt.step()
        out = [host(p.data).copy() for p in ps] + [host(m).copy() for m in opt.m] + [host(v).copy() for v in opt.v] + \
              [host(p.grad).copy() for p in ps]
        if graphed:
            step.release()
        # what happened after each backward(): (launch still waiting, update already applied)
        want = {"auto": (True, False), "peek": (True, False), "opt-in": (False, True), "two-launches": (False, False)}[mode]
        assert all(s_ == want for s_ in seen), (mode, seen)
        return out, losses, opt.t

    b, lb, tb = run("two-launches")
    for mode in ("auto", "opt-in", "peek"):
        a, la, ta = run(mode)
        assert ta == tb and la == lb, mode
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)


def test_mlp_backward_waiting_for_the_optimizer_is_unobservable(hip):
    """Round 5: the README MLP's backward launch waits for optimizer.step() (so that ONE kernel does backward + Adam without any
    opt-in).  Everything a user can do between backward() and step() must see what the reference's eager backward leaves
    (autograd.py:85-93, optim.py:17-33): reading p.grad gives the finished gradient; zero_grad() drops it; assigning p.grad wins
    over it; a second backward() accumulates; gradient clipping through grad_divisor keeps the two-launch path; an in-place
    refill of the input batch before anybody asked for the gradients raises instead of differentiating the wrong batch."""
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    rng = np.random.default_rng(23)
    X = rng.uniform(-1, 1, (32, 784)).astype(np.float32)
    X2 = rng.uniform(-1, 1, (32, 784)).astype(np.float32)
    Y = rng.integers(0, 10, 32).astype(np.int32)

    def build():
        np.random.seed(5)

        class MLP(nn.Module):
            def __init__(self):
                super().__init__()
                self.l1, self.relu, self.l2 = nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)

            def forward(self, x):
                return self.l2(self.relu(self.l1(x)))

        m = MLP()
        return m, m.parameters(), Adam(m.parameters(), lr=1e-2)

    def backward(m, x):
        loss = nn.CrossEntropyLoss()(m(x), T(hip, Y, dtype=np.int32, requires_grad=False))
        loss.backward()
        return loss

    # 1. a read sees the finished gradient, and it equals the eager path's (NNHIP_AUTO_FUSE_STEP=0 equivalent: read right away)
    m, ps, opt = build()
    backward(m, T(hip, X, requires_grad=False))
    assert all(p._pending is not None for p in ps)
    g_first = [host(p.grad).copy() for p in ps]
    assert all(p._pending is None for p in ps)
    m2, ps2, opt2 = build()
    backward(m2, T(hip, X, requires_grad=False))
    opt2.step()                                              # the fused launch; gradients are still written
    for a, b in zip(g_first, ps2):
        np.testing.assert_array_equal(a, host(b.grad))
    # 2. zero_grad() after backward(): nothing is launched, nothing is left, the next step is a first step
    m3, ps3, opt3 = build()
    backward(m3, T(hip, X2, requires_grad=False))
    opt3.zero_grad()
    assert all(p._pending is None and p.grad is None for p in ps3)
    backward(m3, T(hip, X, requires_grad=False))
    opt3.step()
    opt.step()                                               # (model 1: separate launch on the gradients read above)
    for a, b, c in zip(ps, ps2, ps3):
        np.testing.assert_array_equal(host(a.data), host(b.data))
        np.testing.assert_array_equal(host(a.data), host(c.data))
    # 3. an assignment wins; the other three gradients are still produced
    m4, ps4, opt4 = build()
    backward(m4, T(hip, X, requires_grad=False))
    mine = dev(np.full(host(ps4[1].data).shape, 0.5, np.float32))
    ps4[1].grad = mine
    assert ps4[1]._pending is None and ps4[0]._pending is not None
    assert ps4[1].grad is mine
    for k in (0, 2, 3):
        np.testing.assert_array_equal(host(ps4[k].grad), g_first[k])
    # 4. two backward() calls accumulate (the second finds a waiting launch: it runs, then the sum)
    m5, ps5, opt5 = build()
    backward(m5, T(hip, X, requires_grad=False))
    backward(m5, T(hip, X, requires_grad=False))
    for k in range(4):
        np.testing.assert_allclose(host(ps5[k].grad), 2 * g_first[k], rtol=1e-6, atol=1e-7)
    # 5. a refilled input batch before anybody asked for the gradients: loud, not wrong
    m6, ps6, opt6 = build()
    x6 = T(hip, X, requires_grad=False)
    backward(m6, x6)
    x6.data.copy_(dev(X2))
    t6 = opt6.t
    with pytest.raises(RuntimeError, match="written in place"):
        opt6.step()
    assert all(p._pending is None for p in ps6)
    assert opt6.t == t6                                      # nothing was applied: the step counter did not run ahead (advisor, round 5)
    # 6. a gradient divisor switched ON for a step and OFF again (conditional clipping): the fused launch of the third step must not
    #    divide by the divisor the ordinary step() bound to the library handle (advisor, round 5: a stale, possibly freed, pointer)
    def three_steps(toggle):
        m7, ps7, opt7 = build()
        for k in range(3):
            opt7.zero_grad()
            backward(m7, T(hip, X if k != 1 else X2, requires_grad=False))
            if k == 1:
                if toggle:
                    opt7.grad_divisor = dev(np.array([4.0], np.float32))
                else:                                        # the same arithmetic without a divisor: pre-divided gradients
                    for p in ps7:
                        p.grad = p.grad / 4.0
            opt7.step()
            if toggle and k == 1:
                opt7.grad_divisor.fill_(1e30)                # what a recycled allocation would hold
                opt7.grad_divisor = None
        return [host(p.data).copy() for p in ps7]
    for a, b in zip(three_steps(True), three_steps(False)):
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-7)


def test_fused_backward_adam_makes_pending_outputs_stale(hip):
    """optimizer.fuse_backward(True): the backward launch itself updates the parameters, so an output that is still pending --
    the hidden Linear's, whose GEMM rode in the ReLU's launch -- must raise when read between backward() and step(), not
    silently recompute with the updated W1 / b1 (advisor, round 3).  Without fuse_backward the same read is legal and returns the
    forward-time pre-activation."""
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (32, 784)).astype(np.float32)
    Y = rng.integers(0, 10, 32).astype(np.int32)

    def build(fuse):
        np.random.seed(3)

        class MLP(nn.Module):
            def __init__(self):
                super().__init__()
                self.l1, self.relu, self.l2 = nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)

            def forward(self, x):
                self.z1 = self.l1(x)
                return self.l2(self.relu(self.z1))

        m = MLP()
        opt = Adam(m.parameters(), lr=1e-2)
        if fuse:
            opt.fuse_backward(True)
        return m, opt

    for fuse in (False, True):
        model, opt = build(fuse)
        W1, b1 = host(model.l1.weight.data).copy(), host(model.l1.bias.data).copy()
        opt.zero_grad()
        out = model(T(hip, X, requires_grad=False))
        loss = nn.CrossEntropyLoss()(out, T(hip, Y, dtype=np.int32, requires_grad=False))
        assert model.z1.pending()
        loss.backward()
        if fuse:
            assert opt._stepped_in_backward                    # the one-launch backward + Adam really ran
            with pytest.raises(RuntimeError, match="never materialised"):
                model.z1.data
        else:
            np.testing.assert_allclose(host(model.z1.data), O.linear_forward(X, W1, b1), **TOL)
        opt.step()


def test_fused_backward_adam_refuses_grids_that_cannot_be_co_resident(hip):
    """The optimizer-in-backward kernel polls an in-kernel arrival board; the library only launches it when its polling blocks
    (the dW2 tiles) fit on half the chip, so the blocks they wait for always find a slot (advisor, round 3).  A hidden layer of
    32768 units has 2048 dW2 tiles -- more than that: fuse_backward must fall back to backward + separate Adam launch, with the
    same bits as an optimizer that never asked for the fusion."""
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    rng = np.random.default_rng(17)
    X = rng.uniform(-1, 1, (32, 64)).astype(np.float32)
    Y = rng.integers(0, 10, 32).astype(np.int32)

    def run(fuse):
        np.random.seed(21)

        class MLP(nn.Module):
            def __init__(self):
                super().__init__()
                self.l1, self.relu, self.l2 = nn.Linear(64, 32768), nn.ReLU(), nn.Linear(32768, 10)

            def forward(self, x):
                return self.l2(self.relu(self.l1(x)))

        m = MLP()
        opt = Adam(m.parameters(), lr=1e-3)
        if fuse:
            opt.fuse_backward(True)
        stepped = []
        for _ in range(2):
            opt.zero_grad()
            nn.CrossEntropyLoss()(m(T(hip, X, requires_grad=False)), T(hip, Y, dtype=np.int32, requires_grad=False)).backward()
            stepped.append(bool(opt._stepped_in_backward))
            opt.step()
        return [p.numpy().copy() for p in m.parameters()], stepped

    a, sa = run(True)
    b, _ = run(False)
    assert sa == [False, False], "the in-kernel barrier was launched on a grid it cannot hold"
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_deferred_linear_output_read_late(hip):
    """A Linear output whose GEMM rode in its activation's launch is still pending.  Read within the same step it is
    z = XW^T + b of the forward-time operands (the reference's eager Linear holds exactly that,
    neunet/nn/layers/linear.py:48-58); read after optimizer.step() updated W in place it would silently be something else,
    so it raises (round-2 advisor finding)."""
    from neunet_hip.nn.experimental import HIPLinear, HIPReLU
    from neunet_hip.optim import Adam
    rng = np.random.default_rng(41)
    X = rng.uniform(-1, 1, (40, 24)).astype(np.float32)
    layer = HIPLinear(24, 16)
    W, b = host(layer.weight.data), host(layer.bias.data)
    opt = Adam(layer.parameters(), lr=1e-1)
    lin = layer(T(hip, X))
    y = HIPReLU()(lin)
    assert lin.pending()
    y.backward(dev(np.ones((40, 16), np.float32)))
    lin2 = layer(T(hip, X))
    y2 = HIPReLU()(lin2)
    np.testing.assert_allclose(host(lin.data), O.linear_forward(X, W, b), **TOL)     # same step: forward-time value
    assert not lin.pending()
    opt.step()
    assert lin2.pending()
    with pytest.raises(RuntimeError, match="never materialised"):
        lin2.data
    np.testing.assert_allclose(host(lin.data), O.linear_forward(X, W, b), **TOL)     # materialised before the step: unchanged
    del y2


@pytest.mark.parametrize("act_name", ["relu", "sigmoid", "swish"])
def test_linear_activation_deferred_fusion(hip, act_name):
    """act(Linear(x)): the Linear's GEMM is deferred until its output is read, so an activation applied first runs as the
    GEMM's epilogue (one launch).  Same values and gradients as the two-launch path (output read before the activation)
    and as the oracle; the Linear node's own output stays available (Swish: written by the same launch as z)."""
    from neunet_hip.nn.experimental import HIPLinear, HIPReLU, HIPSigmoid, HIPSwish
    rng = np.random.default_rng(4)
    rows, inf, outf = 96, 70, 52
    X = rng.uniform(-1, 1, (rows, inf)).astype(np.float32)
    dY = rng.uniform(-1, 1, (rows, outf)).astype(np.float32)
    layer = HIPLinear(inf, outf)
    W, b = host(layer.weight.data), host(layer.bias.data)
    act = {"relu": HIPReLU(), "sigmoid": HIPSigmoid(), "swish": HIPSwish(1.5)}[act_name]
    res = []
    for fused in (True, False):
        layer.weight.grad = layer.bias.grad = None
        x = T(hip, X)
        lin = layer(x)
        assert lin.pending() and lin.shape == (rows, outf)
        if not fused:
            _ = lin.data                                   # reading the output first materialises the plain GEMM
            assert not lin.pending()
        y = act(lin)
        assert lin.pending() == (fused and act_name != "swish")
        y.backward(dY)
        assert lin.pending() == (fused and act_name != "swish")   # the backward pass never needed the un-activated output
        res.append((host(y.data), host(x.grad), host(layer.weight.grad), host(layer.bias.grad)))
    for a, c in zip(*res):
        np.testing.assert_allclose(a, c, rtol=1e-5, atol=1e-6)
    z = O.linear_forward(X, W, b)
    if act_name == "relu":
        yr, dz = O.relu_forward(z), O.relu_backward(O.relu_forward(z), dY)
    elif act_name == "sigmoid":
        yr = O.sigmoid_forward(z)
        dz = O.sigmoid_backward(yr, dY)
    else:
        yr, dz = O.swish_forward(z, 1.5), O.swish_backward(z, dY, 1.5)
    dX, dW, db = O.linear_backward(X, W, b, dz)
    np.testing.assert_allclose(res[0][0], yr, **TOL)
    np.testing.assert_allclose(res[0][1], dX, **TOL)
    np.testing.assert_allclose(res[0][2], dW, **TOL)
    np.testing.assert_allclose(res[0][3], db, **TOL)


def test_relu_backward_folded_into_next_linear(hip):
    """l2(relu(l1(x))): the ReLU backward runs in the epilogue of l2's dX GEMM when nothing else consumes the ReLU output;
    with a second consumer the plain path is taken.  Both == oracle."""
    from neunet_hip.nn.experimental import HIPLinear, HIPReLU
    rng = np.random.default_rng(6)
    X = rng.uniform(-1, 1, (64, 40)).astype(np.float32)
    dY = rng.uniform(-1, 1, (64, 24)).astype(np.float32)
    l1, l2, relu = HIPLinear(40, 56), HIPLinear(56, 24), HIPReLU()
    W1, b1, W2, b2 = [host(t.data) for t in (l1.weight, l1.bias, l2.weight, l2.bias)]
    z = O.linear_forward(X, W1, b1)
    h = O.relu_forward(z)
    dh, dW2, db2 = O.linear_backward(h, W2, b2, dY)
    dz = O.relu_backward(h, dh)
    dX, dW1, db1 = O.linear_backward(X, W1, b1, dz)
    x = T(hip, X)
    hidden = relu(l1(x))
    out = l2(hidden)
    out.backward(dY)
    assert getattr(hidden, "_consumers", 0) == 1
    np.testing.assert_allclose(host(x.grad), dX, **TOL)
    np.testing.assert_allclose(host(l1.weight.grad), dW1, **TOL)
    np.testing.assert_allclose(host(l2.weight.grad), dW2, **TOL)
    np.testing.assert_allclose(host(hidden.grad), dz, **TOL)     # what the ReLU node received is already masked
    # two consumers of the ReLU output: no folding, gradients accumulate on the tape
    for t in (l1.weight, l1.bias, l2.weight, l2.bias):
        t.grad = None
    x = T(hip, X)
    hidden = relu(l1(x))
    (l2(hidden) + l2(hidden)).backward(dY)
    assert_close_scaled(host(x.grad), 2 * dX)
    assert_close_scaled(host(l2.weight.grad), 2 * dW2)


# ------------------------------------------------------------------------------ lock-step GEMM mode (opt-in)
@pytest.mark.parametrize("rows,inf,outf", [(2048, 4096, 2048), (1100, 2048, 515), (4096, 2304, 1024)])
def test_gemm_lockstep_is_bit_identical(hip, rows, inf, outf):
    """nnhipSetGemmLockstep(1) only changes WHEN the two blocks of a CU issue (s_setprio driven by a progress board), never what
    they compute: Linear forward / dX / dW (+db) with reductions >= 2048 give the same bits as the default mode, twice over (the
    board holds the previous launch's values when the next one starts)."""
    from neunet_hip._lib import call_hip_function
    from neunet_hip.nn.experimental import HIPLinear
    rng = np.random.default_rng(rows + outf)
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    dO = rng.standard_normal((rows, outf)).astype(np.float32)
    np.random.seed(inf + outf)
    layer = HIPLinear(inf, outf)
    assert call_hip_function("nnhipGetGemmLockstep") == 0
    got = []
    try:
        for mode in (0, 1, 1):
            call_hip_function("nnhipSetGemmLockstep", mode)
            layer.weight.grad = layer.bias.grad = None
            x = T(hip, X)
            out = layer(x)
            o = host(out.data)
            out.backward(dO)
            got.append((o, host(x.grad), host(layer.weight.grad), host(layer.bias.grad)))
    finally:
        call_hip_function("nnhipSetGemmLockstep", 0)
    for other in got[1:]:
        for name, a, b in zip(("O", "dX", "dW", "db"), got[0], other):
            assert np.array_equal(a, b), name
    assert_close_scaled(got[0][0], X.astype(np.float64) @ host(layer.weight.data).astype(np.float64).T + host(layer.bias.data))


# ------------------------------------------------------------------------------ split-bf16 GEMM mode (opt-in)
@pytest.fixture
def bf16x3(hip):
    from neunet_hip._lib import call_hip_function
    call_hip_function("nnhipSetGemmMode", 1)
    yield
    call_hip_function("nnhipSetGemmMode", 0)


@pytest.mark.parametrize("rows,inf,outf", [(512, 512, 512), (1000, 520, 300), (4096, 1024, 2048), (300, 4096, 515),
                                           (16384, 512, 512), (2048, 64, 640)])
def test_bf16x3_gemm_is_fp32_accurate(hip, bf16x3, rows, inf, outf):
    """nnhipSetGemmMode(1): every fp32 operand split exactly into three bf16 pieces, six piece products on the bf16 matrix
    cores.  Linear forward / dX / dW / db at shapes that take the 128x128-tile kernel in all three operand layouts (and
    split-K), against float64: the error is of the order of fp32 rounding -- within 2x of what the exact-fp32 MFMA kernel
    itself leaves on the same inputs, and inside the 1e-4 parity tolerance by orders of magnitude."""
    from neunet_hip._lib import call_hip_function
    from neunet_hip.nn.experimental import HIPLinear
    rng = np.random.default_rng(rows + inf)
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    dO = rng.standard_normal((rows, outf)).astype(np.float32)
    np.random.seed(rows + outf)                            # the layer draws its weights from the global generator
    layer = HIPLinear(inf, outf)
    W, b = host(layer.weight.data).astype(np.float64), host(layer.bias.data).astype(np.float64)
    X64, dO64 = X.astype(np.float64), dO.astype(np.float64)
    refs = (X64 @ W.T + b, dO64 @ W, dO64.T @ X64, dO64.sum(0, keepdims=True))
    errs = []
    for mode in (1, 0):
        call_hip_function("nnhipSetGemmMode", mode)
        layer.weight.grad = layer.bias.grad = None
        x = T(hip, X)
        out = layer(x)
        o = host(out.data)
        out.backward(dO)
        got = (o, host(x.grad), host(layer.weight.grad), host(layer.bias.grad))
        errs.append([float(np.abs(g - r).max() / np.abs(r).max()) for g, r in zip(got, refs)])
    call_hip_function("nnhipSetGemmMode", 1)
    for name, e3, e1 in zip(("O", "dX", "dW", "db"), errs[0], errs[1]):
        assert e3 < 2e-6, (name, e3)                       # relative to the largest entry: ~fp32 rounding at these K
        assert e3 <= 2.5 * e1 + 3e-7, (name, e3, e1)       # the same order as the exact-fp32 kernel's own error (max over
                                                           # ~1e6 entries of two different summation orders: not a tight ratio)


def test_bf16x3_split_is_exact_on_hard_inputs(hip, bf16x3):
    """Operands that stress the three-way split: huge dynamic range inside a row, values with all 24 significand bits set,
    exact powers of two, zeros, denormal-adjacent magnitudes.  x * 1 must come back EXACTLY (hi + mid + lo = x, and
    1 = bf16(1)), and a long all-positive dot product stays within 2^-22 of float64."""
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    rng = np.random.default_rng(9)
    M = K = 512                                            # 16 tiles of 128x128: the big kernel, not gemm_small
    A = rng.standard_normal((M, K)).astype(np.float32) * np.exp2(rng.integers(-60, 60, (M, K))).astype(np.float32)
    A[0, :8] = [np.float32(1) - np.float32(2) ** -24, np.float32(1.9999999), 2.0 ** -100, -2.0 ** 100, 0.0, 3.0, 1e-30, 16777215.0]
    I = np.eye(K, dtype=np.float32)
    a_d, i_d, c_d = dev(A), dev(I), torch.empty((M, K), device="cuda")
    call_hip_function("nnhipGemmF32", a_d, i_d, c_d, None, M, K, K, K, K, K, 1, 1, 1, 0, 0, 0, get_current_stream_ptr())
    np.testing.assert_array_equal(host(c_d), A)            # A @ I^T: every product is x*1 and the rest are exact zeros
    P = rng.uniform(0.5, 1.5, (512, 4096)).astype(np.float32)
    Q = rng.uniform(0.5, 1.5, (512, 4096)).astype(np.float32)
    c2 = torch.empty((512, 512), device="cuda")
    call_hip_function("nnhipGemmF32", dev(P), dev(Q), c2, None, 512, 512, 4096, 4096, 4096, 512, 1, 1, 1, 0, 0, 0,
                      get_current_stream_ptr())
    ref = P.astype(np.float64) @ Q.astype(np.float64).T
    assert float(np.abs(host(c2) - ref).max() / ref.max()) < 2.0 ** -21


def _bf3_launches():
    from neunet_hip._lib import call_hip_function
    return int(call_hip_function("nnhipGemmLaunchCount", 3))


def test_bf16x3_gpt_tiny_step_golden(hip, golden, bf16x3):
    """The notebook's GPT step golden (reference logits, loss, every gradient) in split-bf16 mode, same tolerances as the
    exact-fp32 run.  NOTE what this does and does not exercise: the golden model is d32 / vocab 50, so most of its GEMMs are
    routed to gemm_small (exact in either mode); the launch counter says how many reached gemm_bf3_kernel -- the
    full-size evidence for that kernel is test_bf16x3_linear_c2_full_size / test_bf16x3_gpt_c4_full_size below."""
    n0 = _bf3_launches()
    test_gpt_tiny_step_golden(hip, golden, True)
    print(f"gemm_bf3_kernel launches during the d32 golden step: {_bf3_launches() - n0}")


def test_bf16x3_linear_c2_full_size(hip, bf16x3):
    """BASELINE C2 (4096^3) forward / dX / dW / db and linearity with every GEMM on gemm_bf3_kernel (asserted through the
    launch counter): the same float64 row samples and tolerances as the exact-fp32 run."""
    n0 = _bf3_launches()
    test_linear_c2_full_size_properties(hip)
    assert _bf3_launches() - n0 >= 5, "the C2 GEMMs did not run on gemm_bf3_kernel"


def test_bf16x3_gpt_c4_full_size(hip, bf16x3):
    """BASELINE C4 at full size (16384 x 15000 logits) in split-bf16 mode: every check of the exact-fp32 run (sampled rows
    against float64 dot products, losses, gradient rows, fused == unfused attention, Adam) at the same tolerances, with
    the Linear GEMMs on gemm_bf3_kernel (>= 6 layers x 6 + the head's 3 launches, asserted)."""
    n0 = _bf3_launches()
    test_gpt_c4_full_size_properties(hip)
    assert _bf3_launches() - n0 >= 6 * 6 + 3, "the C4 Linear GEMMs did not run on gemm_bf3_kernel"


def test_bf16x3_gemm_batched_all_layouts(hip, bf16x3):
    test_gemm_batched_all_layouts(hip)


def test_linear_transpose_detecting(hip):
    """A = I against an asymmetric B catches a swapped C-write (guide rule 16)."""
    from neunet_hip.nn.experimental import HIPLinear
    n = 160
    layer = HIPLinear(n, n, bias=False)
    W = (np.arange(n * n, dtype=np.float32).reshape(n, n) % 97) / 97.0
    layer.weight.data.copy_(dev(W))
    out = layer(T(hip, np.eye(n, dtype=np.float32)))
    np.testing.assert_allclose(host(out.data), W.T, rtol=0, atol=0)


def test_linear_3d_input_flattens(hip):
    from neunet_hip.nn.experimental import HIPLinear
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (4, 16, 512)).astype(np.float32)
    W = rng.uniform(-0.05, 0.05, (2048, 512)).astype(np.float32)
    b = rng.uniform(-0.05, 0.05, (1, 2048)).astype(np.float32)
    dO = rng.uniform(-1, 1, (4, 16, 2048)).astype(np.float32)
    layer = HIPLinear(512, 2048)
    layer.weight.data.copy_(dev(W))
    layer.bias.data.copy_(dev(b))
    x = T(hip, X)
    out = layer(x)
    assert out.shape == (4, 16, 2048)
    np.testing.assert_allclose(host(out.data), O.linear_forward(X, W, b), **TOL)
    out.backward(dO)
    dX, dW, db = O.linear_backward(X, W, b, dO)
    np.testing.assert_allclose(host(x.grad), dX, **TOL)
    assert_close_scaled(host(layer.weight.grad), dW)
    assert_close_scaled(host(layer.bias.grad), db)


def test_gemm_batched_all_layouts(hip):
    """nnhipGemmF32: 4 operand-layout combinations, batched, odd sizes."""
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    rng = np.random.default_rng(9)
    Bt, M, N, K = 3, 70, 45, 52
    A = rng.standard_normal((Bt, M, K)).astype(np.float32)
    Bm = rng.standard_normal((Bt, K, N)).astype(np.float32)
    ref = np.matmul(A, Bm)
    for akm in (1, 0):
        for bkm in (1, 0):
            a = A if akm else np.ascontiguousarray(A.transpose(0, 2, 1))      # (M,K) or (K,M)
            b = np.ascontiguousarray(Bm.transpose(0, 2, 1)) if bkm else Bm    # (N,K) or (K,N)
            da, db_, dc = dev(a), dev(b), torch.empty(Bt, M, N, device="cuda")
            call_hip_function("nnhipGemmF32", da, db_, dc, None, M, N, K, a.shape[2], b.shape[2], N, akm, bkm,
                              Bt, a.shape[1] * a.shape[2], b.shape[1] * b.shape[2], M * N,
                              get_current_stream_ptr())
            np.testing.assert_allclose(host(dc), ref, rtol=1e-4, atol=1e-4, err_msg=f"akm={akm} bkm={bkm}")


# ------------------------------------------------------------------------------------ Linear -> Swish
@pytest.mark.parametrize("rows,inf,outf,beta,save", [
    (128, 256, 512, 1.0, True), (128, 256, 512, 1.5, False),   # tests/test_linear_swish_cutlass_cuda.py
    (64, 128, 256, 1.5, True), (64, 128, 256, 1.0, False),
])
def test_linear_swish_vs_oracle(hip, rows, inf, outf, beta, save):
    from neunet_hip.nn.experimental import HIPLinearSwish
    rng = np.random.default_rng(rows + outf)
    X = rng.uniform(-1, 1, (rows, inf)).astype(np.float32)
    W = rng.uniform(-0.2, 0.2, (outf, inf)).astype(np.float32)
    b = rng.uniform(-0.2, 0.2, (1, outf)).astype(np.float32)
    dY = rng.uniform(-1, 1, (rows, outf)).astype(np.float32)
    layer = HIPLinearSwish(inf, outf, swish_beta=beta, save_preactivation=save)
    layer.weight.data.copy_(dev(W))
    layer.bias.data.copy_(dev(b))
    x = T(hip, X)
    y = layer(x)
    yr, _ = O.linear_swish_forward(X, W, b, beta)
    np.testing.assert_allclose(host(y.data), yr, **TOL)      # reference tolerance here is 1e-3 (TF32)
    y.backward(dY)
    dX, dW, db = O.linear_swish_backward(X, W, b, dY, beta)
    np.testing.assert_allclose(host(x.grad), dX, **TOL)
    assert_close_scaled(host(layer.weight.grad), dW)
    assert_close_scaled(host(layer.bias.grad), db)


def test_linear_swish_golden(hip, golden):
    g = golden("linear_swish")
    from neunet_hip.nn.experimental import HIPLinearSwish
    layer = HIPLinearSwish(24, 40, swish_beta=float(g["beta"]))
    layer.weight.data.copy_(dev(g["W"]))
    layer.bias.data.copy_(dev(g["b"]))
    x = T(hip, g["X"])
    y = layer(x)
    np.testing.assert_allclose(host(y.data), g["Y"], rtol=1e-5, atol=1e-5)
    y.backward(g["dY"])
    np.testing.assert_allclose(host(x.grad), g["dX"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(layer.weight.grad), g["dW"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(layer.bias.grad), g["db"], rtol=1e-5, atol=1e-5)


# -------------------------------------------------------------------------------------- activations
def test_relu(hip, golden):
    g = golden("relu")
    from neunet_hip.nn.experimental import HIPReLU
    x = T(hip, g["X"])
    y = HIPReLU()(x)
    np.testing.assert_array_equal(host(y.data), g["Y"])
    y.backward(g["dY"])
    np.testing.assert_array_equal(host(x.grad), g["dX"])


@pytest.mark.parametrize("name", ["swish_b1.0", "swish_b1.5"])
def test_swish_golden(hip, golden, name):
    g = golden(name)
    from neunet_hip.nn.experimental import HIPSwish
    x = T(hip, g["X"])
    y = HIPSwish(float(g["beta"]))(x)
    np.testing.assert_allclose(host(y.data), g["Y"], rtol=1e-5, atol=1e-5)
    y.backward(g["dY"])
    np.testing.assert_allclose(host(x.grad), g["dX"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", [(32, 128), (7, 33), (1, 1), (4096, 1030)])
def test_swish_vs_oracle(hip, shape):
    from neunet_hip.nn.experimental import HIPSwish
    rng = np.random.default_rng(42)
    X = (rng.standard_normal(shape) * 3).astype(np.float32)
    dY = rng.standard_normal(shape).astype(np.float32)
    x = T(hip, X)
    y = HIPSwish(1.5)(x)
    np.testing.assert_allclose(host(y.data), O.swish_forward(X, 1.5), rtol=1e-5, atol=1e-5)
    y.backward(dY)
    np.testing.assert_allclose(host(x.grad), O.swish_backward(X, dY, 1.5), rtol=1e-5, atol=1e-5)


def test_swish_fast_sigmoid_accuracy_sweep(hip):
    """Swish / SwiGLU use the hardware exp2 + rcp (1 ulp each) instead of libm expf + IEEE divide.  Sweep the whole
    finite range of the sigmoid argument, [-88, 88], densely: the result stays within 1e-6 absolute + 1 ulp of the
    float64 evaluation of the oracle's formula: forward within 1e-6 absolute + 2 ulp (rcp 1 ulp, 1+e and the final
    product half an ulp each; at |x| = 88 one ulp of the output is 7.6e-6, so a pure absolute bound cannot hold there),
    backward within 1e-6 + 2 ulp of its largest INTERMEDIATE, 1 + |beta f|: the reference's formula
    beta f + s (1 - beta f) (activations.py:212-216) cancels two terms of size beta*x for large x, so its own float32
    evaluation is only that accurate."""
    from neunet_hip.nn.experimental import HIPFusedSwishAndMul, HIPSwish
    X = np.linspace(-88.0, 88.0, 1 << 20, dtype=np.float32).reshape(1024, 1024)
    dY = np.ones_like(X)
    for beta in (1.0, 1.5, 0.5):
        Xb = (X / np.float32(max(beta, 1.0))).astype(np.float32)
        x = T(hip, Xb)
        y = HIPSwish(beta)(x)
        ref = O.swish_forward(Xb.astype(np.float64), beta)
        err = np.abs(host(y.data).astype(np.float64) - ref)
        assert np.all(err <= 1e-6 + 2 * np.spacing(np.abs(ref).astype(np.float32))), float(err.max())
        y.backward(dY)
        refg = O.swish_backward(Xb.astype(np.float64), dY.astype(np.float64), beta)
        errg = np.abs(host(x.grad).astype(np.float64) - refg)
        mag = 1.0 + np.abs(beta * ref)
        assert np.all(errg <= 1e-6 + 2 * np.spacing(mag.astype(np.float32))), float((errg / np.spacing(mag.astype(np.float32))).max())
    # the same sigmoid inside the SwiGLU gate: gate = sweep, up = 1
    G = np.concatenate([X[:, :512], np.ones((1024, 512), np.float32)], axis=1)
    g = T(hip, np.ascontiguousarray(G))
    out = HIPFusedSwishAndMul(1.0)(g)
    ref = O.swish_forward(X[:, :512].astype(np.float64), 1.0)
    err = np.abs(host(out.data).astype(np.float64) - ref)
    assert np.all(err <= 1e-6 + 2 * np.spacing(np.abs(ref).astype(np.float32))), float(err.max())


@pytest.mark.parametrize("name", ["swiglu_2d", "swiglu_3d"])
def test_swiglu_golden(hip, golden, name):
    g = golden(name)
    from neunet_hip.nn.experimental import HIPFusedSwishAndMul
    x = T(hip, g["X"])
    y = HIPFusedSwishAndMul(float(g["beta"]))(x)
    np.testing.assert_allclose(host(y.data), g["Y"], rtol=1e-5, atol=1e-5)
    y.backward(g["dY"])
    np.testing.assert_allclose(host(x.grad), g["dX"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape,h,beta", [((32, 256), 128, 1.0), ((8, 16, 128), 64, 1.5), ((16, 128), 64, 1.0),
                                          ((5, 14), 7, 1.0)])
def test_swiglu_vs_oracle(hip, shape, h, beta):
    """tests/test_fused_swish_and_mul_cuda.py shapes, module + raw kernels."""
    from neunet_hip.nn.experimental.activations import (HIPFusedSwishAndMul, hip_fused_swish_and_mul,
                                                        hip_fused_swish_and_mul_backward)
    rng = np.random.default_rng(123)
    X = rng.standard_normal(shape).astype(np.float32)
    dY = rng.standard_normal(shape[:-1] + (h,)).astype(np.float32)
    x = T(hip, X)
    y = HIPFusedSwishAndMul(beta)(x)
    np.testing.assert_allclose(host(y.data), O.swiglu_forward(X, beta), rtol=1e-5, atol=1e-5)
    y.backward(dY)
    np.testing.assert_allclose(host(x.grad), O.swiglu_backward(X, dY, beta), rtol=1e-5, atol=1e-5)
    out = torch.empty(shape[:-1] + (h,), device="cuda")
    hip_fused_swish_and_mul(dev(X), out, beta)
    np.testing.assert_allclose(host(out), O.swiglu_forward(X, beta), rtol=1e-5, atol=1e-5)
    gin = torch.empty(shape, device="cuda")
    hip_fused_swish_and_mul_backward(gin, dev(dY), dev(X), beta)
    np.testing.assert_allclose(host(gin), O.swiglu_backward(X, dY, beta), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", ["softmax_last", "softmax_axis1_4d", "softmax_axis1_2d"])
def test_softmax_golden(hip, golden, name):
    g = golden(name)
    from neunet_hip.nn.experimental import HIPSoftmax
    x = T(hip, g["X"])
    y = HIPSoftmax(axis=int(g["axis"]))(x)
    np.testing.assert_allclose(host(y.data), g["Y"], rtol=1e-5, atol=1e-6)
    y.backward(g["dY"])
    np.testing.assert_allclose(host(x.grad), g["dX"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape,axis", [
    ((32, 128), -1), ((16, 256), 1),               # tests/test_softmax_cuda.py
    ((4, 8, 64, 64), -1),                          # attention scores layout
    ((64, 4096), -1), ((8, 8192), -1), ((3, 15000), -1), ((2, 20000), -1),   # each row-width bucket + looped
    ((5, 10), 1), ((6, 1023), -1), ((3, 7, 5), 1), ((3, 7, 5), 0),
])
def test_softmax_vs_oracle(hip, shape, axis):
    from neunet_hip.nn.experimental import HIPSoftmax
    rng = np.random.default_rng(42)
    X = (rng.standard_normal(shape) * 2).astype(np.float32)
    dY = rng.standard_normal(shape).astype(np.float32)
    x = T(hip, X)
    y = HIPSoftmax(axis=axis)(x)
    yr = O.softmax_forward(X, axis)
    np.testing.assert_allclose(host(y.data), yr, rtol=1e-5, atol=1e-6)
    y.backward(dY)
    assert_close_scaled(host(x.grad), O.softmax_backward(yr, dY, axis))


def test_rmsnorm_backward_deferred_column_sums(hip):
    """Round 5: while parameter gradients are deferred (nnhipWeightGradDefer, i.e. inside Tensor.backward()) a RMSNorm backward leaves
    its per-block dw / db partials in an arena and the finishing column sums of ALL queued layers go out as one launch at the flush.
    dx is there at once; dw / db are untouched until the flush and then BIT-identical to the immediate path."""
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr, load_hip_function
    rng = np.random.default_rng(61)
    st = get_current_stream_ptr()
    shapes = [(64, 4096, False), (1024, 512, False), (300, 512, True), (2048, 512, False), (777, 512, True)]   # (a change of column width flushes)
    jobs = []
    for rows, cols, bias in shapes:
        X, dY = dev(rng.standard_normal((rows, cols)).astype(np.float32)), dev(rng.standard_normal((rows, cols)).astype(np.float32))
        w = dev(rng.uniform(0.5, 1.5, cols).astype(np.float32))
        std = torch.sqrt((X * X).mean(dim=1) + 1e-6).contiguous()
        jobs.append((rows, cols, bias, X, dY, w, std))

    def run(defer):
        outs = []
        if defer:
            call_hip_function("nnhipWeightGradDefer", 1, st)
        for rows, cols, bias, X, dY, w, std in jobs:
            dx = torch.empty_like(X)
            dw = torch.full((cols,), 123.0, device="cuda")
            db = torch.full((cols,), 321.0, device="cuda") if bias else None
            call_hip_function("nnhipRMSNormBackward", dY, X, w, std, None, dx, dw, db, rows, cols, st)
            outs.append((dx, dw, db))
        if defer:
            torch.cuda.synchronize()
            assert all(float(o[1][0]) == 123.0 for o in outs[1:]), "a deferred column sum ran before the flush"
            assert load_hip_function("nnhipWeightGradPending")() == 0          # (the GEMM queue's counter: column sums are not in it)
            call_hip_function("nnhipWeightGradFlush", st)
            call_hip_function("nnhipWeightGradDefer", 0, st)
        torch.cuda.synchronize()
        return outs

    a, b = run(True), run(False)
    for (dxa, dwa, dba), (dxb, dwb, dbb), (rows, cols, bias, X, dY, w, std) in zip(a, b, jobs):
        assert torch.equal(dxa, dxb) and torch.equal(dwa, dwb)
        if bias:
            assert torch.equal(dba, dbb)
        xn = host(X) / host(std)[:, None]
        np.testing.assert_allclose(host(dwa), (host(dY) * xn).sum(0), rtol=2e-4, atol=2e-3)


_colsum_job = {}


def _colsum_arena_job():
    """A 64 x 128 RMSNorm backward with dW: run(stream, deferred, out) issues it -- and with `deferred` the flush behind it -- on
    `stream` (a raw handle) into the fenced pair out = (dx, dw) with no synchronisation; its non-deferred bits, computed once."""
    from neunet_hip._lib import call_hip_function
    if not _colsum_job:
        rows, cols = 64, 128
        rng = np.random.default_rng(73)
        X, dY = dev(rng.standard_normal((rows, cols)).astype(np.float32)), dev(rng.standard_normal((rows, cols)).astype(np.float32))
        w = dev(rng.uniform(0.5, 1.5, cols).astype(np.float32))
        std = torch.sqrt((X * X).mean(dim=1) + 1e-6).contiguous()

        def run(stream, deferred, out):
            dx, dw = out
            if deferred:
                assert call_hip_function("nnhipWeightGradDefer", 1, stream) == 0
            try:
                assert call_hip_function("nnhipRMSNormBackward", dY, X, w, std, None, dx.view, dw.view, None, rows, cols, stream) == 0
                if deferred:
                    assert call_hip_function("nnhipWeightGradFlush", stream) == 0
            finally:
                if deferred:
                    call_hip_function("nnhipWeightGradDefer", 0, stream)

        ref = _colsum_outs()
        run(torch.cuda.current_stream().cuda_stream, False, ref)
        torch.cuda.synchronize()
        _colsum_job.update(run=run, ref=[ref[0].view.clone(), ref[1].view.clone()])
    return _colsum_job["run"], _colsum_job["ref"]


def _colsum_outs():
    """NaN-filled on torch's current stream, which a job on another stream would not wait for: synchronise before use."""
    from conv_child import FencedAt
    return FencedAt((64, 128)), FencedAt((128,))


def _same_as_plain(got, ref, what):
    for f, r, name in zip(got, ref, ("dX", "dW")):
        assert f.guards_intact() and torch.equal(f.view, r), f"{what}: {name} differs from the non-deferred call"


def test_colsum_queue_after_its_stream_is_destroyed(hip):
    """A column sum queued and flushed on a stream that is then synchronised and DESTROYED, the next one on the default stream: the
    arena's guard only compares the old handle (recording an event on it, or asking whether it is capturing, is undefined behaviour)."""
    import ctypes
    import gc
    run, ref = _colsum_arena_job()
    hiprt = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p()
    assert hiprt.hipStreamCreate(ctypes.byref(raw)) == 0
    st = torch.cuda.ExternalStream(raw.value)
    first, second = _colsum_outs(), _colsum_outs()
    torch.cuda.synchronize()
    run(raw.value, True, first)
    st.synchronize()
    del st
    gc.collect()
    assert hiprt.hipStreamDestroy(raw) == 0
    run(torch.cuda.current_stream().cuda_stream, True, second)                     # (run() asserts status 0 of every call)
    torch.cuda.synchronize()
    _same_as_plain(first, ref, "on the stream destroyed since")
    _same_as_plain(second, ref, "on the default stream behind it")


def test_colsum_arena_captured_then_eager_on_another_stream(hip):
    """The backward and its flush captured into a hipGraph and replayed once, then the same backward eagerly on a second stream with no
    host synchronisation: a capture leaves no event to wait for and the replay may still be reading the arena, so the eager
    reservation synchronises with the device."""
    run, ref = _colsum_arena_job()
    cap, other = torch.cuda.Stream(), torch.cuda.Stream()
    warm, graphed, eager = _colsum_outs(), _colsum_outs(), _colsum_outs()
    torch.cuda.synchronize()
    run(cap.cuda_stream, True, warm)                                               # the arena exists: it cannot grow inside a capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap, capture_error_mode="thread_local"):
        run(torch.cuda.current_stream().cuda_stream, True, graphed)
    assert bool(torch.isnan(graphed[1].view).all())                                # capturing runs nothing
    g.replay()
    run(other.cuda_stream, True, eager)
    torch.cuda.synchronize()
    _same_as_plain(graphed, ref, "graph replay")
    _same_as_plain(eager, ref, "eager on another stream behind the replay")


# ---------------------------------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("name", ["rmsnorm_2d", "rmsnorm_3d_bias"])
def test_rmsnorm_golden(hip, golden, name):
    g = golden(name)
    from neunet_hip.nn.experimental import HIPRMSNorm
    layer = HIPRMSNorm(g["X"].shape[-1], eps=float(g["eps"]), bias="b" in g)
    layer.weight.data.copy_(dev(g["w"]))
    if "b" in g:
        layer.bias.data.copy_(dev(g["b"]))
    x = T(hip, g["X"])
    y = layer(x)
    np.testing.assert_allclose(host(y.data), g["Y"], rtol=1e-5, atol=1e-5)
    y.backward(g["dY"])
    np.testing.assert_allclose(host(x.grad), g["dX"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(layer.weight.grad), g["dw"], rtol=1e-4, atol=1e-5)
    if "b" in g:
        np.testing.assert_allclose(host(layer.bias.grad), g["db"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shape,bias", [((32, 128), False), ((16, 256), False),   # tests/test_rmsnorm_cuda.py
                                        ((4, 64, 512), True), ((2100, 4096), True), ((9, 8192), False),
                                        ((5, 12000), True), ((7, 130), True), ((3, 6), False),
                                        ((16384, 512), False), ((4099, 512), True), ((37, 1000), True),   # C4 norm shape; ragged
                                        ((6, 20000), True), ((3, 16388), False), ((70, 16385), True)])   # looped (> 16384 cols)
def test_rmsnorm_vs_oracle(hip, shape, bias):
    from neunet_hip.nn.experimental import HIPRMSNorm
    rng = np.random.default_rng(42)
    X = rng.standard_normal(shape).astype(np.float32)
    w = rng.uniform(0.5, 1.5, shape[-1]).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, shape[-1]).astype(np.float32) if bias else None
    dY = rng.standard_normal(shape).astype(np.float32)
    layer = HIPRMSNorm(shape[-1], eps=1e-6, bias=bias)
    layer.weight.data.copy_(dev(w))
    if bias:
        layer.bias.data.copy_(dev(b))
    x = T(hip, X)
    y = layer(x)
    Yr, _, _ = O.rmsnorm_forward(X, w, b, 1e-6)
    np.testing.assert_allclose(host(y.data), Yr, **TOL)
    y.backward(dY)
    dX, dw, db = O.rmsnorm_backward(X, w, bias, dY, 1e-6)
    np.testing.assert_allclose(host(x.grad), dX, **TOL)
    rows = int(np.prod(shape[:-1]))
    assert_close_scaled(host(layer.weight.grad), dw)           # column sums over `rows` terms of either sign
    if bias:
        assert_close_scaled(host(layer.bias.grad), db)


# ------------------------------------------------------------------------------------ CrossEntropy
@pytest.mark.parametrize("name", ["ce_mean", "ce_sum", "ce_none", "ce_mean_ign", "ce_sum_ign", "ce_none_ign",
                                  "ce_mean_pad0", "ce_mean_small"])
@pytest.mark.parametrize("inplace", [False, True])
def test_cross_entropy_golden(hip, golden, name, inplace):
    g = golden(name)
    from neunet_hip.nn.experimental import HIPCrossEntropyLoss
    x = T(hip, g["logits"])
    y = T(hip, g["labels"], dtype=np.int32, requires_grad=False)
    loss = HIPCrossEntropyLoss(reduction=str(g["reduction"]), ignore_index=int(g["ignore_index"]), inplace=inplace)(x, y)
    np.testing.assert_allclose(host(loss.data).reshape(g["loss"].shape), g["loss"], rtol=1e-5, atol=1e-5)
    loss.backward()
    np.testing.assert_allclose(host(x.grad), g["dlogits"], rtol=1e-5, atol=1e-6)
    if not inplace:
        np.testing.assert_array_equal(host(x.data), g["logits"])  # CPU semantics: logits survive


@pytest.mark.parametrize("rows,C", [(32, 128), (16, 256), (8, 64),            # tests/test_crossentropyloss_cuda.py
                                    (32, 10), (64, 15000), (5, 4099), (3, 20001), (40, 1000)])
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_cross_entropy_vs_oracle(hip, rows, C, reduction):
    from neunet_hip.nn.experimental import HIPCrossEntropyLoss
    rng = np.random.default_rng(42)
    logits = (rng.standard_normal((rows, C)) * 3).astype(np.float32)
    labels = rng.integers(1, C, rows).astype(np.int32)
    labels[:: 5] = 0                      # PAD=0 is the ignored label (GPT config)
    x = T(hip, logits)
    loss = HIPCrossEntropyLoss(reduction=reduction, ignore_index=0)(x, T(hip, labels, dtype=np.int32, requires_grad=False))
    lr, dl = O.cross_entropy_forward_backward(logits, labels, None, 0, reduction)
    np.testing.assert_allclose(host(loss.data), lr, rtol=1e-5, atol=1e-5)
    loss.backward()
    assert_close_scaled(host(x.grad), dl)
    assert np.all(host(x.grad)[labels == 0] == 0)


@pytest.mark.parametrize("rows,C", [(32, 10), (200, 128), (64, 5000), (9, 15000), (3, 20001)])
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("ldtype", [np.int16, np.int32, np.int64])
def test_cross_entropy_class_weights_and_label_dtypes(hip, rows, C, reduction, ldtype):
    """neunet.nn.CrossEntropyLoss(weight=...) (losses.py:93-118: loss_i = -logp[y_i] w[y_i]; 'mean' divides by
    sum_i w[y_i] over the non-ignored rows) and the three label dtypes NLLLoss accepts (losses.py:100)."""
    import neunet_hip.nn as nn
    if np.iinfo(ldtype).max < C:
        pytest.skip("labels do not fit the dtype")
    rng = np.random.default_rng(7 + rows + C)
    logits = (rng.standard_normal((rows, C)) * 3).astype(np.float32)
    labels = rng.integers(1, C, rows).astype(ldtype)
    labels[::4] = 0
    w = rng.uniform(0.25, 2.0, C).astype(np.float32)
    for weight in (None, w):
        x = T(hip, logits)
        loss = nn.CrossEntropyLoss(weight=None if weight is None else hip.Tensor(weight), ignore_index=0,
                                   reduction=reduction)(x, T(hip, labels, dtype=ldtype, requires_grad=False))
        lr, dl = O.cross_entropy_forward_backward(logits, labels, weight, 0, reduction)
        np.testing.assert_allclose(host(loss.data), lr, rtol=1e-5, atol=1e-5)
        loss.backward()
        assert_close_scaled(host(x.grad), dl)
        assert np.all(host(x.grad)[labels == 0] == 0)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_cross_entropy_class_weights_golden(hip, golden, reduction):
    """neunet.nn.CrossEntropyLoss(weight=w, ignore_index=-100) of the reference, int64 labels (golden ce_weighted)."""
    import neunet_hip.nn as nn
    g = golden("ce_weighted")
    x = T(hip, g["logits"])
    y = T(hip, g["labels"], dtype=np.int64, requires_grad=False)
    loss = nn.CrossEntropyLoss(weight=hip.Tensor(g["weight"]), ignore_index=int(g["ignore_index"]), reduction=reduction)(x, y)
    np.testing.assert_allclose(host(loss.data).reshape(-1), g[f"loss_{reduction}"], rtol=1e-5, atol=1e-5)
    loss.backward()
    np.testing.assert_allclose(host(x.grad), g[f"dlogits_{reduction}"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("rows,C", [(16, 10), (300, 2000)])      # single-block kernel / persistent kernel
def test_cross_entropy_out_of_range_label_is_inert(hip, rows, C, inplace):
    """A label outside [0, C) that is not ignore_index (the reference would raise / Python-wrap it, losses.py:104 TODO):
    zero loss and zero gradient for that row, identically in the small and the large kernel (round-1 ADVICE: the small
    kernel read x[y] out of bounds)."""
    from neunet_hip.nn.experimental import HIPCrossEntropyLoss
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((rows, C)) * 2).astype(np.float32)
    labels = rng.integers(0, C, rows).astype(np.int32)
    bad = np.array([1, 5, rows - 1])
    labels[bad] = [-1, C, C + 7]
    labels[3] = -100
    good = np.ones(rows, bool)
    good[bad] = False
    good[3] = False
    for reduction in ("sum", "mean"):
        x = T(hip, logits)
        loss = HIPCrossEntropyLoss(reduction=reduction, ignore_index=-100, inplace=inplace)(
            x, T(hip, labels, dtype=np.int32, requires_grad=False))
        loss.backward()
        g = host(x.grad)
        assert np.all(g[~good] == 0)
        # an out-of-range row behaves exactly like an ignored one -- in the 'mean' denominator too (one predicate in the count
        # and in the rows kernels): the result is the oracle's on the valid rows alone
        lr, dl = O.cross_entropy_forward_backward(logits[good], labels[good], None, -100, reduction)
        np.testing.assert_allclose(loss.item(), float(lr), rtol=1e-5, atol=1e-5)
        assert_close_scaled(g[good], dl)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_cross_entropy_backward_with_an_upstream_gradient(hip, reduction):
    """loss.backward(g) with g != ones: the reference forms grad_y_pred * grad (cross_entropy.py:111-114) -- here on the library's
    own nnhipScaleRows (a device scalar for a reduced loss, one factor per row for reduction 'none'), against the oracle's
    `upstream` argument."""
    from neunet_hip.nn.experimental import HIPCrossEntropyLoss
    rng = np.random.default_rng(12)
    rows, C = 48, 130
    logits = (rng.standard_normal((rows, C)) * 2).astype(np.float32)
    labels = rng.integers(0, C, rows).astype(np.int32)
    labels[5] = 120
    up = rng.uniform(0.5, 2.0, rows).astype(np.float32) if reduction == "none" else np.float32(1.75)
    x = T(hip, logits)
    loss = HIPCrossEntropyLoss(reduction=reduction, ignore_index=120)(x, T(hip, labels, dtype=np.int32, requires_grad=False))
    loss.backward(dev(np.asarray(up, np.float32).reshape(-1) if reduction == "none" else np.asarray([up], np.float32)))
    lr, dl = O.cross_entropy_forward_backward(logits, labels, None, 120, reduction, upstream=up)
    np.testing.assert_allclose(host(loss.data).reshape(np.shape(lr)), lr, rtol=1e-5, atol=1e-6)
    assert_close_scaled(host(x.grad), dl)


def test_mse_backward_with_an_upstream_gradient(hip):
    """MSELoss.backward(g): dpred * g (neunet/nn/losses.py:9-22 through the tape) on nnhipScaleRows."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(13)
    P, Tt = rng.uniform(0, 1, (32, 10)).astype(np.float32), rng.uniform(0, 1, (32, 10)).astype(np.float32)
    p = T(hip, P)
    loss = nn.MSELoss()(p, T(hip, Tt, requires_grad=False))
    loss.backward(dev(np.asarray([0.25], np.float32)))
    _, dp = O.mse_forward_backward(P, Tt)
    np.testing.assert_allclose(host(p.grad), 0.25 * dp, rtol=1e-6, atol=1e-8)


def test_cross_entropy_tall_narrow_takes_the_two_launch_path(hip):
    """rows so many that a per-block label count would not be free (rows x blocks x 4 B > 64 MB): the denominator comes
    from its own small launch; results identical in kind."""
    from neunet_hip.nn.experimental import HIPCrossEntropyLoss
    rng = np.random.default_rng(11)
    rows, C = 300000, 1100
    logits = rng.standard_normal((rows, C)).astype(np.float32)
    labels = rng.integers(0, C, rows).astype(np.int32)
    labels[::7] = -100
    x = T(hip, logits)
    loss = HIPCrossEntropyLoss(reduction="mean")(x, T(hip, labels, dtype=np.int32, requires_grad=False))
    loss.backward()
    sel = rng.choice(rows, 64, replace=False)
    cnt = int((labels != -100).sum())
    lr, dl = O.cross_entropy_forward_backward(logits[sel], labels[sel], None, -100, "sum")
    np.testing.assert_allclose(host(x.grad[torch.from_numpy(sel).cuda()]), dl / cnt, rtol=1e-4, atol=1e-9)
    lse = np.log(np.exp(logits.astype(np.float64)).sum(1))
    ref = float(np.sum((lse - logits[np.arange(rows), np.maximum(labels, 0)])[labels != -100]) / cnt)
    assert abs(loss.item() - ref) < 1e-4


def test_masked_softmax_wide_rows_looped(hip):
    """nnhipMaskedSoftmaxForward/Backward for Tk > 16384 (round 1 returned EINVAL): looped kernels, same formulas."""
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    rng = np.random.default_rng(3)
    B, H, Tq, Tk = 2, 1, 3, 16500
    S = rng.standard_normal((B, H, Tq, Tk)).astype(np.float32)
    dY = rng.standard_normal((B, H, Tq, Tk)).astype(np.float32)
    kv = np.ones((B, Tk), np.int32)
    kv[1, -500:] = 0
    scale = 0.125
    s_d, dy_d, kv_d = dev(S), dev(dY), dev(kv)
    y_d, dx_d = torch.empty_like(s_d), torch.empty_like(s_d)
    call_hip_function("nnhipMaskedSoftmaxForward", y_d, s_d, kv_d, B, H, Tq, Tk, scale, 1, get_current_stream_ptr())
    call_hip_function("nnhipMaskedSoftmaxBackward", dx_d, dy_d, y_d, kv_d, B, H, Tq, Tk, scale, 1, get_current_stream_ptr())
    j, i = np.arange(Tk)[None, :], np.arange(Tq)[:, None]
    masked = (j > i + Tk - Tq)[None, None] | (kv == 0)[:, None, None, :]
    z = np.where(masked, np.float32(-1e9), S * np.float32(scale))
    yr = O.softmax_forward(z.astype(np.float32), -1)
    np.testing.assert_allclose(host(y_d), yr, rtol=1e-5, atol=1e-7)
    dz = O.softmax_backward(yr, dY, -1)
    np.testing.assert_allclose(host(dx_d), np.where(masked, 0, dz * scale), rtol=1e-4, atol=1e-7)


# ------------------------------------------------------------------------------------------- Conv2d
@pytest.mark.parametrize("name", ["conv2d_s2p1d2", "conv2d_s2_uncovered", "conv2d_pad4", "conv2d_c5_l1",
                                  "conv2d_c5_l2"])
def test_conv2d_golden(hip, golden, name):
    g = golden(name)
    from neunet_hip.nn.experimental import HIPConv2d
    Cout, Cin, kh, kw = g["W"].shape
    pad = tuple(int(p) for p in g["padding"])
    layer = HIPConv2d(Cin, Cout, (kh, kw), tuple(int(s) for s in g["stride"]), pad,
                      tuple(int(d) for d in g["dilation"]))
    assert tuple(layer.padding) == tuple(int(p) for p in g["padding4"])
    layer.weight.data.copy_(dev(g["W"]))
    layer.bias.data.copy_(dev(g["b"]))
    x = T(hip, g["X"])
    y = layer(x)
    assert y.shape == g["O"].shape
    np.testing.assert_allclose(host(y.data), g["O"], rtol=1e-5, atol=1e-5)
    y.backward(g["dO"])
    np.testing.assert_allclose(host(x.grad), g["dX"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(layer.weight.grad), g["dW"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(host(layer.bias.grad), g["db"], rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(host(layer.weight.data), g["W"])  # never mutated (Appendix A.2)


@pytest.mark.parametrize("xshape,cout,ks,stride,pad,dil", [
    ((16, 1, 28, 28), 8, 3, (1, 1), (1, 1), (1, 1)),       # C5 layer 1
    ((16, 8, 14, 14), 16, 3, (1, 1), (1, 1), (1, 1)),      # C5 layer 2
    ((3, 5, 17, 13), 40, (3, 2), (2, 1), (2, 0), (1, 2)),  # Cout > 32 (two m-tiles), odd everything
    ((2, 40, 9, 9), 6, 3, (1, 1), (0, 0), (1, 1)),         # Cin*kh*kw + 1 = 361 columns > 128 (3 n-groups)
    ((1, 1, 5, 5), 1, 1, (1, 1), (0, 0), (1, 1)),
    # implicit-GEMM kernel, 64- and 128-row block tiles (channels > 16), K not a multiple of the 16-deep k-tile, > 256 pixels per image
    ((2, 24, 19, 17), 48, 3, (1, 1), (1, 1), (1, 1)),      # forward M-tile 64, dgrad M-tile 32
    ((2, 72, 11, 9), 130, 3, (1, 1), (1, 1), (1, 1)),      # forward M-tile 128 (two tiles, the second nearly empty), dgrad 128
    ((2, 33, 14, 14), 20, (3, 2), (2, 2), (1, 0), (1, 2)), # dgrad with stride 2 (per-element division) and dilation, forward M-tile 32
    ((1, 20, 6, 40), 70, (1, 3), (1, 1), (0, 1), (1, 1)),  # 1 x 3 taps, one image narrower than a pixel tile
    # small channel counts take the direct (one pixel, all channels per thread) forward / dgrad kernels:
    ((3, 4, 17, 13), 3, (3, 2), (2, 1), (2, 0), (1, 2)),   # Cout <= 4 variant, strides, asymmetric everything
    ((2, 16, 9, 9), 16, 5, (1, 1), (2, 2), (1, 1)),        # 25 taps, 16 x 16 channels (the direct kernels' limits)
    ((2, 3, 12, 12), 12, 3, (2, 2), (1, 1), (2, 2)),       # stride 2 + dilation 2: inexact divisions in dgrad
    # 3x3, small channels: the 16x16x4-MFMA wgrad (padded image in LDS) with 4 / 10 column tiles, odd pixel counts, wide padding
    ((4, 7, 10, 15), 9, 3, (1, 1), (0, 2), (1, 1)),
    ((2, 16, 8, 8), 16, 3, (1, 1), (1, 1), (1, 1)),
    ((5, 2, 7, 5), 3, 3, (1, 2), (2, 2), (2, 1)),
    # 3x3, few positions: the "quad" direct kernels (four lanes per position, reduction channels split, DPP sum) -- also layer 2 above
    ((3, 5, 9, 11), 6, 3, (1, 1), (1, 1), (1, 1)),         # forward <8>, dgrad <8>, channel counts that are no multiple of four
    ((2, 4, 6, 7), 16, 3, (2, 1), (0, 1), (1, 2)),         # forward <16> with one channel per lane, dgrad <4>, stride + dilation
    ((1, 8, 3, 3), 13, 3, (1, 1), (2, 2), (1, 1)),         # nine positions: a block with a ragged last quad; padding wider than the image
])
def test_conv2d_vs_oracle(hip, xshape, cout, ks, stride, pad, dil):
    from neunet_hip.nn.experimental import HIPConv2d
    rng = np.random.default_rng(15)
    X = rng.uniform(-1, 1, xshape).astype(np.float32)
    layer = HIPConv2d(xshape[1], cout, ks, stride, pad, dil)
    W = host(layer.weight.data)
    b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    layer.bias.data.copy_(dev(b))
    x = T(hip, X)
    y = layer(x)
    Or = O.conv2d_forward(X, W, b, stride, pad, dil)
    assert y.shape == Or.shape
    np.testing.assert_allclose(host(y.data), Or, **TOL)
    dO = rng.uniform(-1, 1, Or.shape).astype(np.float32)
    y.backward(dO)
    dX, dW, db = O.conv2d_backward(X, W, True, dO, stride, pad, dil)
    np.testing.assert_allclose(host(x.grad), dX, **TOL)
    assert_close_scaled(host(layer.weight.grad), dW)       # sums over batch x pixels of either sign
    assert_close_scaled(host(layer.bias.grad), db)


def test_conv2d_igemm_random_geometries(hip):
    """The MFMA implicit-GEMM kernels of conv_mfma.hip (channels > 16: forward / dgrad with the tap outermost and repacked
    weights, 128 x 128 or 64 x 256 block tiles; wgrad over (image, pixel) k-tiles with (tap slot, channel) columns) on 24 random
    geometries -- kernel sizes 1..4, strides 1..3, dilations 1..2, asymmetric padding, channel counts on both sides of every tile
    edge, pixel counts that are and are not multiples of four (16-byte and dword dO loads) -- against the oracle."""
    from neunet_hip.nn.experimental import HIPConv2d
    rng = np.random.default_rng(77)
    done = 0
    while done < 24:
        cin, cout = int(rng.choice([17, 20, 31, 33, 48, 64, 65, 96, 130])), int(rng.choice([17, 24, 32, 40, 64, 72, 128, 129]))
        kh, kw = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        sh, sw = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        dh, dw = int(rng.integers(1, 3)), int(rng.integers(1, 3))
        ph, pw = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        H, W = int(rng.integers(5, 15)), int(rng.integers(5, 15))
        if H + 2 * ph < dh * (kh - 1) + 1 or W + 2 * pw < dw * (kw - 1) + 1:
            continue
        B = int(rng.integers(1, 4))
        X = rng.uniform(-1, 1, (B, cin, H, W)).astype(np.float32)
        layer = HIPConv2d(cin, cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw))
        Wt = host(layer.weight.data)
        b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
        layer.bias.data.copy_(dev(b))
        x = T(hip, X)
        y = layer(x)
        Or = O.conv2d_forward(X, Wt, b, (sh, sw), (ph, pw), (dh, dw))
        tag = f"cin {cin} cout {cout} k {kh}x{kw} s {sh},{sw} d {dh},{dw} p {ph},{pw} in {B}x{H}x{W}"
        assert y.shape == Or.shape, tag
        np.testing.assert_allclose(host(y.data), Or, err_msg=tag, **TOL)
        dO = rng.uniform(-1, 1, Or.shape).astype(np.float32)
        y.backward(dO)
        dX, dW, db = O.conv2d_backward(X, Wt, True, dO, (sh, sw), (ph, pw), (dh, dw))
        np.testing.assert_allclose(host(x.grad), dX, err_msg=tag, **TOL)
        assert_close_scaled(host(layer.weight.grad), dW, err_msg=tag)
        assert_close_scaled(host(layer.bias.grad), db, err_msg=tag)
        done += 1


@pytest.mark.parametrize("B,cin,H,W,cout,k,stride,pad,dil", [
    (3, 160, 20, 18, 96, 3, 1, 1, 1),      # 128-row tile; Cin > 128: two channel blocks per tap; even k-tiles per chunk; float4 dO loads
    (3, 160, 20, 17, 96, 3, 1, 1, 1),      # odd k-tiles per chunk (the pipeline's look-ahead tile must not enter db)
    (2, 300, 9, 11, 40, 3, 1, 1, 1),       # 64-row tile, 256-channel tap slots, two channel blocks; 99 pixels: dword dO loads
    (5, 64, 13, 13, 128, 3, 2, 1, 1),      # stride 2: dgrad's exact-division test per tap; 49 output pixels per image
    (2, 48, 16, 16, 80, (1, 5), 1, (0, 2), (1, 2)),   # 1 x 5 taps with dilation 2, Cin no multiple of the 32-deep k-tile
    (1, 32, 40, 40, 64, 1, 1, 0, 1),       # 1 x 1 convolution: one tap, TPT = 8 slots of which one is used; too few k-tiles to split
    (18, 32, 62, 62, 72, 3, 1, 1, 1),      # 541 pixel tiles: one whole round of 512 in the plain launch + 29 tiles in the split-K tail launch
])
def test_conv2d_mfma_kernels_through_the_c_abi(hip, B, cin, H, W, cout, k, stride, pad, dil):
    """nnhipConv2dForward / nnhipConv2dBackward on layers that take conv_mfma.hip, called with every output combination the ABI
    allows (dX only, dW only, db only, all three): each must equal the oracle (conv2d.py:297-355, 16-115), and the separately
    requested outputs must be bit-identical to the jointly requested ones (same kernels, same reduction order)."""
    import ctypes
    from neunet_hip._lib import Conv2dDesc, call_hip_function as call, get_current_stream_ptr
    kh, kw = (k, k) if isinstance(k, int) else k
    st2 = (stride, stride) if isinstance(stride, int) else stride
    pd2 = (pad, pad) if isinstance(pad, int) else pad
    dl2 = (dil, dil) if isinstance(dil, int) else dil
    rng = np.random.default_rng(B * 1000 + cin)
    X = rng.uniform(-1, 1, (B, cin, H, W)).astype(np.float32)
    Wt = (rng.uniform(-1, 1, (cout, cin, kh, kw)) / np.sqrt(cin * kh * kw)).astype(np.float32)
    bias = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    Or = O.conv2d_forward(X, Wt, bias, st2, pd2, dl2)
    dO = rng.uniform(-1, 1, Or.shape).astype(np.float32)
    dXr, dWr, dbr = O.conv2d_backward(X, Wt, True, dO, st2, pd2, dl2)
    d = Conv2dDesc(B, cin, H, W, cout, kh, kw, st2[0], st2[1], dl2[0], dl2[1], pd2[0], pd2[0], pd2[1], pd2[1])
    st = get_current_stream_ptr()
    x, w, b_, do = dev(X), dev(Wt), dev(bias), dev(dO)
    out = torch.empty(Or.shape, device="cuda")
    call("nnhipConv2dForward", x, w, b_, out, ctypes.byref(d), st)
    np.testing.assert_allclose(host(out), Or, **TOL)
    call("nnhipConv2dForward", x, w, None, out, ctypes.byref(d), st)                       # bias = NULL
    np.testing.assert_allclose(host(out), Or - bias[None, :, None, None], **TOL)
    dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b_)
    call("nnhipConv2dBackward", x, w, do, dx, dw, db, ctypes.byref(d), st)
    np.testing.assert_allclose(host(dx), dXr, **TOL)
    assert_close_scaled(host(dw), dWr)
    assert_close_scaled(host(db), dbr)
    dx2, dw2, db2 = torch.full_like(dx, 7.0), torch.full_like(dw, 7.0), torch.full_like(db, 7.0)
    call("nnhipConv2dBackward", x, w, do, dx2, None, None, ctypes.byref(d), st)
    call("nnhipConv2dBackward", x, w, do, None, dw2, None, ctypes.byref(d), st)
    call("nnhipConv2dBackward", x, w, do, None, None, db2, ctypes.byref(d), st)
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw) and torch.equal(db2, db)


def test_conv2d_mfma_full_size_samples(hip):
    """The MFMA conv kernels at the size the kernel bench quotes (Conv2d 64 -> 128 channels, 3x3, 56 x 56, batch 64: 29.6 GFLOP per
    pass; 1568 pixel tiles = three whole rounds + a split-K tail in one grid; wgrad in 102 K chunks) -- too large for the NumPy
    oracle's einsum, so sampled entries are recomputed in float64 straight from the definition (conv2d.py:297-355, 16-115):
    forward and dX entries as dot products over (ci, r, s) / (co, r, s), dW entries as sums over all 200 704 (b, ho, wo), db in full."""
    import ctypes
    from neunet_hip._lib import Conv2dDesc, call_hip_function as call, get_current_stream_ptr
    B, Cin, H, Cout = 64, 64, 56, 128
    rng = np.random.default_rng(2024)
    X = rng.uniform(-1, 1, (B, Cin, H, H)).astype(np.float32)
    Wt = (rng.uniform(-1, 1, (Cout, Cin, 3, 3)) / 24).astype(np.float32)
    bias = rng.uniform(-0.3, 0.3, Cout).astype(np.float32)
    dO = rng.uniform(-1, 1, (B, Cout, H, H)).astype(np.float32)
    d = Conv2dDesc(B, Cin, H, H, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
    st = get_current_stream_ptr()
    x, w, b_, do = dev(X), dev(Wt), dev(bias), dev(dO)
    out, dx, dw, db = torch.empty_like(do), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b_)
    call("nnhipConv2dForward", x, w, b_, out, ctypes.byref(d), st)
    call("nnhipConv2dBackward", x, w, do, dx, dw, db, ctypes.byref(d), st)
    out, dx, dw, db = host(out), host(dx), host(dw), host(db)
    Xp = np.pad(X, ((0, 0), (0, 0), (1, 1), (1, 1))).astype(np.float64)
    dOp = np.pad(dO, ((0, 0), (0, 0), (1, 1), (1, 1))).astype(np.float64)
    W64 = Wt.astype(np.float64)
    # forward: edge pixels, pixels of the last (split) tiles, random ones
    pts = [(0, 0, 0, 0), (B - 1, Cout - 1, H - 1, H - 1), (B - 1, 5, H - 1, 0), (B - 1, 77, 40, 55)]
    pts += [tuple(int(v) for v in (rng.integers(B), rng.integers(Cout), rng.integers(H), rng.integers(H))) for _ in range(60)]
    for (bb, co, y, xx) in pts:
        ref = float(np.sum(Xp[bb, :, y:y + 3, xx:xx + 3] * W64[co])) + float(bias[co])
        bound = 32 * U24 * float(np.sum(np.abs(Xp[bb, :, y:y + 3, xx:xx + 3] * W64[co]))) + 4 * U24 * abs(ref) + 1e-7
        assert abs(float(out[bb, co, y, xx]) - ref) <= bound, ("forward", bb, co, y, xx, out[bb, co, y, xx], ref)
    # dX[b, ci, y, x] = sum_{co, r, s} W[co, ci, r, s] dO[b, co, y + 1 - r, x + 1 - s]  (unit stride, padding 1)
    Wf = W64[:, :, ::-1, ::-1]
    for (bb, ci, y, xx) in [(0, 0, 0, 0), (B - 1, Cin - 1, H - 1, H - 1)] + [tuple(int(v) for v in (rng.integers(B), rng.integers(Cin), rng.integers(H), rng.integers(H))) for _ in range(60)]:
        terms = dOp[bb, :, y:y + 3, xx:xx + 3] * Wf[:, ci]
        ref = float(np.sum(terms))
        assert abs(float(dx[bb, ci, y, xx]) - ref) <= 32 * U24 * float(np.sum(np.abs(terms))) + 1e-7, ("dX", bb, ci, y, xx)
    # dW entries: sums over batch x pixels (K = 200 704)
    rms_dw = rms_of(dw)
    for (co, ci, r, s_) in [(0, 0, 0, 0), (Cout - 1, Cin - 1, 2, 2)] + [tuple(int(v) for v in (rng.integers(Cout), rng.integers(Cin), rng.integers(3), rng.integers(3))) for _ in range(24)]:
        ref = float(np.sum(Xp[:, ci, r:r + H, s_:s_ + H] * dO[:, co].astype(np.float64)))
        assert abs(float(dw[co, ci, r, s_]) - ref) <= 1e-4 * max(abs(ref), rms_dw), ("dW", co, ci, r, s_, dw[co, ci, r, s_], ref)
    assert_close_scaled(db, dO.astype(np.float64).sum(axis=(0, 2, 3)), err_msg="db")


# -------------------------------------------------------------------------------------- optimizers
@pytest.mark.parametrize("name", ["adam_wd0", "adam_wd1e-2", "adamw_wd0", "adamw_wd1e-2"])
@pytest.mark.parametrize("multi", [False, True])
def test_adam_golden(hip, golden, name, multi):
    g = golden(name)
    from neunet_hip.nn import Parameter
    from neunet_hip.optim import Adam, AdamW, HIPFusedAdamW
    n = int(g["n_tensors"])
    params = [Parameter(T(hip, g[f"p0_{i}"])) for i in range(n)]
    is_w = name.startswith("adamw")
    if multi:
        opt = (AdamW if is_w else Adam)(params, lr=float(g["lr"]), weight_decay=float(g["wd"]))
    else:
        opt = HIPFusedAdamW(params, lr=float(g["lr"]), weight_decay=float(g["wd"]))
        opt.decay_mode = 0 if is_w else 1
    for s in range(3):
        for i, p in enumerate(params):
            p.grad = dev(g[f"g{s}_{i}"])
        opt.step()
        for i, p in enumerate(params):
            np.testing.assert_allclose(host(p.data), g[f"p{s + 1}_{i}"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(host(opt.m[i]), g[f"m{s + 1}_{i}"], rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(host(opt.v[i]), g[f"v{s + 1}_{i}"], rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("shapes", [[(128, 256)], [(64, 128)] * 3, [(32, 64)] * 5, [(1000, 333), (7,), (16385,)]])
@pytest.mark.parametrize("wd", [1e-2, 0.0])
def test_fused_adamw_vs_oracle(hip, shapes, wd):
    """tests/test_fusedadamw_cuda.py: one step of both fused optimizers vs AdamW; then 2 more steps with
    some gradients missing (skipped params) and changing pointers."""
    from neunet_hip.nn import Parameter
    from neunet_hip.optim import HIPFusedAdamW, HIPFusedMultiTensorAdamW
    rng = np.random.default_rng(123)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    for cls in (HIPFusedAdamW, HIPFusedMultiTensorAdamW):
        params = [Parameter(T(hip, a)) for a in p0]
        opt = cls(params, lr=1e-3, weight_decay=wd)
        ref_p = [a.copy() for a in p0]
        ref_m = [np.zeros_like(a) for a in p0]
        ref_v = [np.zeros_like(a) for a in p0]
        for step in range(1, 4):
            gs = [rng.standard_normal(s).astype(np.float32) for s in shapes]
            for i, p in enumerate(params):
                skip = step == 2 and i == 0 and len(shapes) > 1
                p.grad = None if skip else dev(gs[i])
                if not skip:
                    ref_m[i], ref_v[i] = O.adamw_step(ref_p[i], gs[i], ref_m[i], ref_v[i], step, 1e-3,
                                                      (0.9, 0.999), 1e-8, wd)
            opt.step()
            for i, p in enumerate(params):
                assert_close_scaled(host(p.data), ref_p[i])


# ---------------------------------------------------------------------------- C1 end-to-end trajectory
def test_mlp_c1_trajectory_golden(hip, golden):
    """README quick-start loop on the HIP path vs the REAL reference's trajectory:
    losses, argmax (bit-exact), first-step grads, weights after 3 Adam steps."""
    g = golden("mlp_c1")
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam

    class MLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.l1 = nn.Linear(784, 128)
            self.relu = nn.ReLU()
            self.l2 = nn.Linear(128, 10)

        def forward(self, x):
            return self.l2(self.relu(self.l1(x)))

    model = MLP()
    model.l1.weight.data.copy_(dev(g["W1"]))
    model.l1.bias.data.copy_(dev(g["b1"]))
    model.l2.weight.data.copy_(dev(g["W2"]))
    model.l2.bias.data.copy_(dev(g["b2"]))
    opt = Adam(model.parameters(), lr=1e-3)
    loss_fn = nn.CrossEntropyLoss()
    for s in range(3):
        opt.zero_grad()
        out = model(T(hip, g["X"][s], requires_grad=False))
        loss = loss_fn(out, T(hip, g["Y"][s], dtype=np.int32, requires_grad=False))
        loss.backward()
        if s == 0:
            ps = model.parameters()
            assert_close_scaled(host(ps[0].grad)[::8], g["dW1_step0_rows"])
            assert_close_scaled(host(ps[1].grad), g["db1_step0"])
            assert_close_scaled(host(ps[2].grad), g["dW2_step0"])
            assert_close_scaled(host(ps[3].grad), g["db2_step0"])
        opt.step()
        assert abs(loss.item() - g["losses"][s]) < 1e-4
        np.testing.assert_array_equal(host(hip.argmax(out, axis=1).data), g["argmax"][s])
    np.testing.assert_allclose(host(model.l1.weight.data)[::8], g["W1_final_rows"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(model.l1.bias.data), g["b1_final"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(model.l2.weight.data), g["W2_final"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(model.l2.bias.data), g["b2_final"], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------- full-size, size-independent properties
def test_linear_c2_full_size_properties(hip):
    """BASELINE C2 (4096x4096x4096) is too slow for the oracle; check sampled rows against float64 dot
    products and linearity:  L(x1 + x2) - b = (L(x1) - b) + (L(x2) - b)."""
    from neunet_hip.nn.experimental import HIPLinear
    rng = np.random.default_rng(1002)
    n = 4096
    X = rng.uniform(-1, 1, (n, n)).astype(np.float32)
    layer = HIPLinear(n, n)
    W, b = host(layer.weight.data), host(layer.bias.data)
    x = T(hip, X)
    out = layer(x)
    o = host(out.data)
    rows = rng.choice(n, 16, replace=False)
    ref = X[rows].astype(np.float64) @ W.T.astype(np.float64) + b
    np.testing.assert_allclose(o[rows], ref, rtol=1e-4, atol=1e-4)
    dO = rng.uniform(-1, 1, (n, n)).astype(np.float32)
    out.backward(dO)
    dX, dW, db = host(x.grad), host(layer.weight.grad), host(layer.bias.grad)
    np.testing.assert_allclose(dX[rows], dO[rows].astype(np.float64) @ W.astype(np.float64), rtol=1e-4, atol=1e-4)
    assert_close_scaled(dW[rows], dO[:, rows].T.astype(np.float64) @ X.astype(np.float64))
    assert_close_scaled(db[0], dO.astype(np.float64).sum(0))
    X2 = rng.uniform(-1, 1, (n, n)).astype(np.float32)
    o2 = host(layer(T(hip, X2)).data)
    o12 = host(layer(T(hip, X + X2)).data)
    assert_close_scaled(o12 - b, (o - b) + (o2 - b))


def test_fused_c3_full_size_properties(hip):
    """C3 sizes (8192 x 4096): softmax rows sum to 1 / grads sum to 0; RMSNorm output has unit RMS;
    CE gradient rows sum to 0 and sum(loss)/count == mean; Swish matches the oracle on a row sample."""
    from neunet_hip.nn.experimental import HIPCrossEntropyLoss, HIPRMSNorm, HIPSoftmax, HIPSwish
    rng = np.random.default_rng(1003)
    R, D = 8192, 4096
    X = rng.standard_normal((R, D)).astype(np.float32)
    x = T(hip, X)
    y = HIPSoftmax(axis=-1)(x)
    s = y.data.sum(dim=1)
    assert torch.allclose(s, torch.ones_like(s), atol=1e-5)
    dYs = rng.standard_normal((R, D)).astype(np.float32)
    y.backward(dYs)
    assert float(x.grad.sum(dim=1).abs().max()) < 1e-4
    rows = rng.choice(R, 8, replace=False)
    ys_rows = O.softmax_forward(X[rows], -1)
    np.testing.assert_allclose(host(y.data)[rows], ys_rows, rtol=1e-5, atol=1e-7)
    # backward on the same 8-row sample against the oracle (activations.py:437-446: dx = (dy - sum(dy y)) y, row-local) --
    # the row-sum property above would also hold for a wrong inner product (round-3 review)
    np.testing.assert_allclose(host(x.grad)[rows], O.softmax_backward(ys_rows, dYs[rows], -1), rtol=1e-4, atol=1e-7)

    # RMSNorm with a NON-trivial weight and a bias (w = 1 makes "unit RMS" blind to a misplaced eps or a wrong dw): forward and
    # dx on the row sample vs the oracle (rmsnorm.py:84-94, 43-59: row-local given w), dw / db -- sums over all 8192 rows --
    # against a float64 pass over the full tensor
    wn = rng.uniform(0.5, 1.5, D).astype(np.float32)
    bn_ = rng.uniform(-0.5, 0.5, D).astype(np.float32)
    norm = HIPRMSNorm(D, bias=True)
    norm.weight.data.copy_(dev(wn))
    norm.bias.data.copy_(dev(bn_))
    x = T(hip, X)
    yn = norm(x)
    yr, _, _ = O.rmsnorm_forward(X[rows], wn, bn_)
    np.testing.assert_allclose(host(yn.data)[rows], yr, rtol=1e-5, atol=1e-6)
    yn.backward(dYs)
    dxr, _, _ = O.rmsnorm_backward(X[rows], wn, True, dYs[rows])
    np.testing.assert_allclose(host(x.grad)[rows], dxr, rtol=1e-4, atol=1e-6)
    X64, dY64 = X.astype(np.float64), dYs.astype(np.float64)
    xn64 = X64 / np.sqrt(np.mean(X64 ** 2, -1, keepdims=True) + 1e-6)
    assert_close_scaled(host(norm.weight.grad).reshape(-1), np.sum(dY64 * xn64, axis=0), err_msg="rmsnorm dw at C3 size")
    assert_close_scaled(host(norm.bias.grad).reshape(-1), np.sum(dY64, axis=0), err_msg="rmsnorm db at C3 size")
    del X64, dY64, xn64, norm, yn
    x = T(hip, X)
    yn = HIPRMSNorm(D)(x)
    rms = (yn.data ** 2).mean(dim=1).sqrt()
    assert torch.allclose(rms, torch.ones_like(rms), atol=1e-4)

    x = T(hip, X)
    ys = HIPSwish(1.0)(x)
    np.testing.assert_allclose(host(ys.data)[rows], O.swish_forward(X[rows], 1.0), rtol=1e-5, atol=1e-6)

    labels = rng.integers(1, D, R).astype(np.int32)
    labels[::10] = 0
    x = T(hip, X)
    loss = HIPCrossEntropyLoss(reduction="mean", ignore_index=0)(x, T(hip, labels, dtype=np.int32, requires_grad=False))
    loss.backward()
    assert float(x.grad.sum(dim=1).abs().max()) < 1e-6
    lr, dl = O.cross_entropy_forward_backward(X[rows], labels[rows], None, 0, "sum")
    cnt = int((labels != 0).sum())
    np.testing.assert_allclose(host(x.grad)[rows], dl / cnt, rtol=1e-4, atol=1e-9)
    ref_mean = O.cross_entropy_forward_backward(X, labels, None, 0, "mean")[0]
    assert abs(loss.item() - float(ref_mean)) < 1e-4

    # fused Linear->Swish 8192 x 4096 -> 4096 (C3's MFMA-bound op): sampled rows vs float64; z saved; backward rows
    from neunet_hip.nn.experimental import HIPFusedSwishAndMul, HIPLinearSwish
    ls = HIPLinearSwish(D, D, swish_beta=1.0, save_preactivation=True)
    W, b = host(ls.weight.data).astype(np.float64), host(ls.bias.data).astype(np.float64)
    x = T(hip, X)
    yl = ls(x)
    z64 = X[rows].astype(np.float64) @ W.T + b
    np.testing.assert_allclose(host(yl.data)[rows], z64 / (1 + np.exp(-z64)), rtol=1e-4, atol=1e-4)
    dYl = rng.standard_normal((R, D)).astype(np.float32)
    yl.backward(dYl)
    sg = 1 / (1 + np.exp(-z64))
    dz64 = dYl[rows].astype(np.float64) * (sg + z64 * sg * (1 - sg))
    assert_close_scaled(host(x.grad)[rows], dz64 @ W)
    assert bool(torch.isfinite(ls.weight.grad).all())
    del ls, yl, x

    # SwiGLU gate 8192 x (2 x 2048)
    x = T(hip, X)
    yg = HIPFusedSwishAndMul(1.0)(x)
    np.testing.assert_allclose(host(yg.data)[rows], O.swiglu_forward(X[rows], 1.0), rtol=1e-5, atol=1e-6)
    dG = rng.standard_normal((R, D // 2)).astype(np.float32)
    yg.backward(dG)
    np.testing.assert_allclose(host(x.grad)[rows], O.swiglu_backward(X[rows], dG[rows], 1.0), rtol=1e-5, atol=1e-5)

    # multi-tensor AdamW over 200 x (512, 1024) (scripts/profile_adam.py:11-14): 3 steps vs the oracle on sampled tensors
    from neunet_hip.nn import Parameter
    from neunet_hip.optim import HIPFusedMultiTensorAdamW
    ps, refs = [], {}
    for i in range(200):
        a = rng.standard_normal((512, 1024)).astype(np.float32)
        ps.append(Parameter(hip.Tensor(a, device="cuda")))
        if i % 37 == 0:
            refs[i] = [a.copy(), np.zeros_like(a), np.zeros_like(a)]
    opt = HIPFusedMultiTensorAdamW(ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for step in range(1, 4):
        for i, p in enumerate(ps):
            gnp = rng.standard_normal((512, 1024)).astype(np.float32) if i in refs else None
            p.grad = dev(gnp) if gnp is not None else torch.randn(512, 1024, device="cuda")
            if i in refs:
                refs[i][1], refs[i][2] = O.adamw_step(refs[i][0], gnp, refs[i][1], refs[i][2], step, 1e-3, (0.9, 0.999), 1e-8, 1e-2)
        opt.step()
    for i, (pr, _, _) in refs.items():
        np.testing.assert_allclose(host(ps[i].data), pr, rtol=1e-5, atol=1e-6)


# =============================================================================================================
# Embedding (last-write-wins gradient), attention (strided-batched GEMM + fused masked softmax),
# GPT-tiny training step -- against golden vectors produced by EXECUTING the notebook's own model cells.
# =============================================================================================================
def test_embedding_golden(hip, golden):
    g = golden("embedding")
    import neunet_hip.nn as nn
    emb = nn.Embedding(*g["W"].shape)
    emb.weight.data.copy_(dev(g["W"]))
    out = emb(T(hip, g["ids"], dtype=np.int32, requires_grad=False))
    np.testing.assert_array_equal(host(out.data), g["out"])
    out.backward(g["grad"])
    np.testing.assert_array_equal(host(emb.weight.grad), g["dW"])      # bit-exact: it is a row copy


def test_embedding_scale_pe_vs_oracle(hip):
    import neunet_hip.nn as nn
    rng = np.random.default_rng(3)
    V, D, B, Tn = 97, 48, 5, 33
    emb = nn.Embedding(V, D)
    pe = nn.PositionalEncoding(D, max_len=64)
    W = host(emb.weight.data)
    ids = rng.integers(0, V, (B, Tn)).astype(np.int32)
    ids[:, 5] = ids[:, 4]
    out = emb(T(hip, ids, dtype=np.int32, requires_grad=False), scale=np.sqrt(D), pe=pe.table)
    ref = O.embedding_forward(W, ids) * np.float32(np.sqrt(D)) + O.positional_encoding(64, D)[None, :Tn]
    np.testing.assert_allclose(host(out.data), ref, rtol=1e-6, atol=1e-6)
    gr = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(gr)
    np.testing.assert_allclose(host(emb.weight.grad), O.embedding_backward(W.shape, ids, gr * np.float32(np.sqrt(D))),
                               rtol=1e-6, atol=1e-6)


def test_mha_golden(hip, golden):
    g = golden("mha")
    import neunet_hip.nn as nn
    B, Tn, D = g["X"].shape
    mha = nn.MultiHeadAttention(D, int(g["n_heads"]))
    for name, lin in zip("qkvo", [mha.wq, mha.wk, mha.wv, mha.fc]):
        lin.weight.data.copy_(dev(g[f"W{name}"]))
        lin.bias.data.copy_(dev(g[f"b{name}"]))
    x = T(hip, g["X"])
    y, attn = mha(x, x, x, dev(g["key_valid"]), causal=True)
    np.testing.assert_allclose(host(attn), g["attn"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(y.data), g["Y"], rtol=1e-4, atol=1e-5)
    y.backward(g["dY"])
    np.testing.assert_allclose(host(x.grad), g["dX"], rtol=1e-4, atol=1e-5)
    for name, lin in zip("qkvo", [mha.wq, mha.wk, mha.wv, mha.fc]):
        np.testing.assert_allclose(host(lin.weight.grad), g[f"dW{name}"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(host(lin.bias.grad), g[f"db{name}"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,Tn,D,H", [(3, 100, 64, 4), (2, 256, 512, 8), (1, 7, 24, 3)])
def test_mha_vs_oracle(hip, B, Tn, D, H):
    import neunet_hip.nn as nn
    rng = np.random.default_rng(B * Tn)
    mha = nn.MultiHeadAttention(D, H)
    ps = []
    for lin in (mha.wq, mha.wk, mha.wv, mha.fc):
        ps += [host(lin.weight.data), host(lin.bias.data)]
    X = rng.standard_normal((B, Tn, D)).astype(np.float32)
    tok = rng.integers(1, 9, (B, Tn))
    tok[0, -max(1, Tn // 5):] = 0
    mask = O.attention_mask(tok, 0)
    ref = O.MHA(*ps, n_heads=H)
    yr, ar = ref.forward(X, mask)
    x = T(hip, X)
    y, attn = mha(x, x, x, dev((tok != 0).astype(np.int32)), causal=True)
    assert_close_scaled(host(attn), ar)
    np.testing.assert_allclose(host(y.data), yr, **TOL)
    dY = rng.standard_normal(yr.shape).astype(np.float32)
    y.backward(dY)
    dxr, gr = ref.backward(dY)
    assert_close_scaled(host(x.grad), dxr)
    for lin, dW, db in zip((mha.wq, mha.wk, mha.wv, mha.fc), gr[0::2], gr[1::2]):
        assert_close_scaled(host(lin.weight.grad), dW)
        assert_close_scaled(host(lin.bias.grad), db, scale=rms_of(dW))


@pytest.mark.parametrize("B,Tn,D,H,causal", [(2, 256, 512, 8, True), (3, 100, 256, 4, True), (1, 7, 64, 1, True),
                                              (2, 130, 128, 2, True), (2, 257, 128, 2, False), (1, 64, 64, 1, True)])
def test_fused_attention_vs_oracle(hip, B, Tn, D, H, causal):
    """need_weights=False takes nnhipAttentionForward/Backward (flash-style, head_dim 64): same output and
    gradients as the oracle MHA (and therefore as the GEMM + masked-softmax path), incl. padded keys."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(B * Tn + D)
    mha = nn.MultiHeadAttention(D, H)
    ps = []
    for lin in (mha.wq, mha.wk, mha.wv, mha.fc):
        lin.weight.data.mul_(3.0)          # sharper softmax than the default init gives
        ps += [host(lin.weight.data), host(lin.bias.data)]
    X = rng.standard_normal((B, Tn, D)).astype(np.float32)
    tok = rng.integers(1, 9, (B, Tn))
    tok[0, -max(1, Tn // 5):] = 0
    tok[-1, Tn // 2] = 0
    mask = O.attention_mask(tok, 0) if causal else np.broadcast_to((tok != 0)[:, None, :], (B, Tn, Tn)).astype(np.int32)
    ref = O.MHA(*ps, n_heads=H)
    yr, _ = ref.forward(X, mask)
    x = T(hip, X)
    y, attn = mha(x, x, x, dev((tok != 0).astype(np.int32)), causal=causal, need_weights=False)
    assert attn is None
    np.testing.assert_allclose(host(y.data), yr, **TOL)
    dY = rng.standard_normal(yr.shape).astype(np.float32)
    y.backward(dY)
    dxr, gr = ref.backward(dY)
    assert_close_scaled(host(x.grad), dxr)
    for lin, dW, db in zip((mha.wq, mha.wk, mha.wv, mha.fc), gr[0::2], gr[1::2]):
        assert_close_scaled(host(lin.weight.grad), dW)
        assert_close_scaled(host(lin.bias.grad), db, scale=rms_of(dW))


@pytest.mark.parametrize("B,Tn,D,H", [(2, 50, 64, 4), (2, 128, 128, 2)])
def test_mha_attention_dropout(hip, B, Tn, D, H):
    """cell 2's `self.dropout(softmax(scores))` with an injected mask (the reference draws it with the host NumPy RNG):
    output, returned map and every gradient equal the oracle's; p > 0 in training mode draws a device mask (runs, finite,
    different from p = 0), eval mode is the identity."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(B * Tn + 5)
    mha = nn.MultiHeadAttention(D, H, dropout=0.25)
    ps = []
    for lin in (mha.wq, mha.wk, mha.wv, mha.fc):
        ps += [host(lin.weight.data), host(lin.bias.data)]
    X = rng.standard_normal((B, Tn, D)).astype(np.float32)
    tok = rng.integers(1, 9, (B, Tn))
    tok[0, -5:] = 0
    drop = ((rng.random((B, H, Tn, Tn)) >= 0.25) / 0.75).astype(np.float32)
    ref = O.MHA(*ps, n_heads=H)
    yr, ar = ref.forward(X, O.attention_mask(tok, 0), drop_mask=drop)
    kv = dev((tok != 0).astype(np.int32))
    x = T(hip, X)
    y, attn = mha(x, x, x, kv, causal=True, drop_mask=dev(drop))
    assert_close_scaled(host(attn), ar)
    np.testing.assert_allclose(host(y.data), yr, **TOL)
    dY = rng.standard_normal(yr.shape).astype(np.float32)
    y.backward(dY)
    dxr, gr = ref.backward(dY)
    assert_close_scaled(host(x.grad), dxr)
    for lin, dW, db in zip((mha.wq, mha.wk, mha.wv, mha.fc), gr[0::2], gr[1::2]):
        assert_close_scaled(host(lin.weight.grad), dW)
        assert_close_scaled(host(lin.bias.grad), db, scale=rms_of(dW))
    # device RNG in training mode; identity in eval mode (fused kernels again when need_weights=False)
    x2 = T(hip, X)
    y_train, a_train = mha(x2, x2, x2, kv, causal=True, need_weights=True)
    assert a_train is not None and np.isfinite(host(y_train.data)).all()
    assert (host(a_train) == 0).mean() > 0.5          # causal zeros + ~25 % dropped
    y_fused, a_fused = mha(x2, x2, x2, kv, causal=True, need_weights=False)   # dropout inside the fused kernels (hash RNG)
    assert (a_fused is None) == (D // H in (32, 64, 128)) and np.isfinite(host(y_fused.data)).all()
    assert not np.allclose(host(y_fused.data), yr, atol=1e-3)
    y_train.backward(dY)
    assert np.isfinite(host(x2.grad)).all()
    mha.dropout.eval()
    y_eval, _ = mha(x2, x2, x2, kv, causal=True)
    ref0 = O.MHA(*ps, n_heads=H)
    np.testing.assert_allclose(host(y_eval.data), ref0.forward(X, O.attention_mask(tok, 0))[0], **TOL)


@pytest.mark.parametrize("dh,H,Tq,Tk,causal", [(32, 4, 150, 150, True), (32, 2, 64, 200, False), (128, 2, 200, 200, True),
                                                (128, 1, 70, 130, False), (64, 3, 257, 257, True)])
def test_fused_attention_head_dims(hip, dh, H, Tq, Tk, causal):
    """The fused kernels at head_dim 32 / 64 / 128 (round 1: 64 only) against the GEMM + masked-softmax path, forward and
    all three gradients, with padded keys and (causal case) leading padding -> fully masked rows."""
    from neunet_hip.nn.experimental import attention as A
    rng = np.random.default_rng(dh + Tq)
    B, D = 2, H * dh
    q = dev(rng.standard_normal((B, Tq, D)).astype(np.float32) * 1.5)
    k = dev(rng.standard_normal((B, Tk, D)).astype(np.float32) * 1.5)
    v = dev(rng.standard_normal((B, Tk, D)).astype(np.float32))
    do = dev(rng.standard_normal((B, Tq, D)).astype(np.float32))
    kvh = (rng.random((B, Tk)) > 0.15).astype(np.int32)
    if causal:
        kvh[0, :9] = 0
    kv = dev(kvh)
    scale = float(np.sqrt(D))
    ctx_u, attn, _ = A.attention_forward(q, k, v, kv, H, scale, causal)
    gu = A.attention_backward(q, k, v, attn, kv, H, scale, causal, do)
    ctx_f, lse = A.fused_attention_forward(q, k, v, kv, H, scale, causal)
    gf = A.fused_attention_backward(q, k, v, kv, ctx_f, lse, H, scale, causal, do)
    np.testing.assert_allclose(host(ctx_f), host(ctx_u), rtol=1e-4, atol=2e-5)
    for a, b, n in zip(gf, gu, "qkv"):
        np.testing.assert_allclose(host(a), host(b), rtol=1e-4, atol=5e-5, err_msg="d" + n)


@pytest.mark.parametrize("dh,H,Tn", [(64, 2, 130), (32, 3, 70), (128, 1, 96)])
def test_fused_attention_dropout_injected_and_hash(hip, dh, H, Tn):
    """Attention dropout inside the fused kernels.  (1) an injected [B,H,T,T] mask: output and gradients equal the GEMM +
    masked-softmax path given the same mask (which test_mha_attention_dropout pins to the oracle).  (2) the hash RNG:
    identical to injecting the mask nnhipAttentionDropoutMask writes for the same (p, seed); about p of the entries are
    dropped; another seed -- host side or through the device-side seed offset -- gives another mask."""
    from neunet_hip.nn.experimental import attention as A
    rng = np.random.default_rng(dh * 7 + Tn)
    B, D, p = 2, H * dh, 0.3
    q, k, v, do = [dev(rng.standard_normal((B, Tn, D)).astype(np.float32)) for _ in range(4)]
    kvh = np.ones((B, Tn), np.int32)
    kvh[1, -11:] = 0
    kv = dev(kvh)
    scale = float(np.sqrt(D))
    drop = dev(((rng.random((B, H, Tn, Tn)) >= p) / (1 - p)).astype(np.float32))
    ctx_u, attn, used = A.attention_forward(q, k, v, kv, H, scale, True, drop)
    gu = A.attention_backward(q, k, v, attn, kv, H, scale, True, do, drop_mask=drop, attn_used=used)
    o1 = A.FusedAttentionOptions(dropout_mask=drop)
    ctx_f, lse = A.fused_attention_forward(q, k, v, kv, H, scale, True, o1)
    gf = A.fused_attention_backward(q, k, v, kv, ctx_f, lse, H, scale, True, do, opts=o1)
    np.testing.assert_allclose(host(ctx_f), host(ctx_u), rtol=1e-4, atol=2e-5)
    for a, b, n in zip(gf, gu, "qkv"):
        np.testing.assert_allclose(host(a), host(b), rtol=1e-4, atol=5e-5, err_msg="injected d" + n)
    # hash RNG == its own materialised mask
    seed = 12345
    hmask = A.attention_dropout_mask(B, H, Tn, Tn, p, seed)
    hm = host(hmask)
    assert set(np.unique(hm)).issubset({0.0, np.float32(1 / (1 - p))})
    assert abs((hm == 0).mean() - p) < 0.02
    o2, o3 = A.FusedAttentionOptions(dropout_p=p, seed=seed), A.FusedAttentionOptions(dropout_mask=hmask)
    c2, l2 = A.fused_attention_forward(q, k, v, kv, H, scale, True, o2)
    c3, l3 = A.fused_attention_forward(q, k, v, kv, H, scale, True, o3)
    np.testing.assert_array_equal(host(c2), host(c3))
    g2 = A.fused_attention_backward(q, k, v, kv, c2, l2, H, scale, True, do, opts=o2)
    g3 = A.fused_attention_backward(q, k, v, kv, c3, l3, H, scale, True, do, opts=o3)
    for a, b in zip(g2, g3):
        np.testing.assert_array_equal(host(a), host(b))
    # a different seed, and the same seed shifted by a device-side counter
    c4, _ = A.fused_attention_forward(q, k, v, kv, H, scale, True, A.FusedAttentionOptions(dropout_p=p, seed=seed + 1))
    assert not np.array_equal(host(c4), host(c2))
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    c5, _ = A.fused_attention_forward(q, k, v, kv, H, scale, True, A.FusedAttentionOptions(dropout_p=p, seed=seed, seed_dev=one))
    np.testing.assert_array_equal(host(c5), host(c4))


@pytest.mark.parametrize("D,H,Tn", [(128, 2, 150), (64, 2, 64), (256, 2, 97)])
def test_fused_attention_dense_mask(hip, D, H, Tn):
    """The notebook hands MultiHeadAttention a DENSE mask (cell 7: get_pad_mask(x) & get_sub_mask(x)).  (1) that very mask,
    packed into bits, gives the same output and gradients as its (key_valid, causal) form; (2) an arbitrary random dense
    mask -- including rows with no visible key, which the reference turns into a uniform distribution over ALL keys --
    matches the oracle MHA given the same mask; dropout on top still matches the unfused formula."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(D + Tn)
    B = 2
    mha = nn.MultiHeadAttention(D, H)
    ps = []
    for lin in (mha.wq, mha.wk, mha.wv, mha.fc):
        lin.weight.data.mul_(2.0)
        ps += [host(lin.weight.data), host(lin.bias.data)]
    X = rng.standard_normal((B, Tn, D)).astype(np.float32)
    dY = rng.standard_normal((B, Tn, D)).astype(np.float32)
    tok = rng.integers(1, 9, (B, Tn))
    tok[0, -7:] = 0
    tok[1, :3] = 0
    pc = O.attention_mask(tok, 0)                                  # [B,T,T] pad & causal
    masks = [pc]
    rnd = (rng.random((B, Tn, Tn)) > 0.4).astype(np.int32)
    rnd[0, 5, :] = 0                                               # rows that see nothing
    rnd[1, Tn - 1, :] = 0
    rnd[1, :, 64:] = 0 if Tn > 64 else rnd[1, :, 64:]              # whole key tiles invisible to a batch (tile skipping)
    masks.append(rnd)
    for mi, mask in enumerate(masks):
        ref = O.MHA(*ps, n_heads=H)
        yr, _ = ref.forward(X, mask)
        dxr, gr = ref.backward(dY)
        for lin in (mha.wq, mha.wk, mha.wv, mha.fc):
            lin.weight.grad = lin.bias.grad = None
        x = T(hip, X)
        y, attn = mha(x, x, x, need_weights=False, mask=T(hip, mask[:, None], dtype=np.int32, requires_grad=False))
        assert attn is None
        np.testing.assert_allclose(host(y.data), yr, **TOL)
        y.backward(dY)
        assert_close_scaled(host(x.grad), dxr, err_msg=f"mask {mi}")
        for lin, dW, db in zip((mha.wq, mha.wk, mha.wv, mha.fc), gr[0::2], gr[1::2]):
            assert_close_scaled(host(lin.weight.grad), dW)
            assert_close_scaled(host(lin.bias.grad), db, scale=rms_of(dW))
        # the GEMM + masked-softmax path (returns the attention map) takes the dense mask too
        for lin in (mha.wq, mha.wk, mha.wv, mha.fc):
            lin.weight.grad = lin.bias.grad = None
        xu = T(hip, X)
        yu, au = mha(xu, xu, xu, need_weights=True, mask=dev(mask))
        np.testing.assert_allclose(host(yu.data), yr, **TOL)
        assert_close_scaled(host(au), ref.attn)
        yu.backward(dY)
        assert_close_scaled(host(xu.grad), dxr)
        if mi == 0:   # identical to the (key_valid, causal) form of the same mask
            x2 = T(hip, X)
            y2, _ = mha(x2, x2, x2, dev((tok != 0).astype(np.int32)), causal=True, need_weights=False)
            np.testing.assert_allclose(host(y.data), host(y2.data), rtol=1e-5, atol=1e-6)
    # dense mask + injected dropout mask vs the oracle
    drop = ((rng.random((B, H, Tn, Tn)) >= 0.2) / 0.8).astype(np.float32)
    ref = O.MHA(*ps, n_heads=H)
    yr, _ = ref.forward(X, rnd, drop_mask=drop)
    dxr, _ = ref.backward(dY)
    x = T(hip, X)
    y, _ = mha(x, x, x, need_weights=False, mask=dev(rnd), drop_mask=dev(drop))
    np.testing.assert_allclose(host(y.data), yr, **TOL)
    y.backward(dY)
    assert_close_scaled(host(x.grad), dxr)


def test_fused_attention_fully_masked_rows(hip):
    """Queries whose every visible key is padding: the reference's where(mask, scores, -1e9) makes their softmax
    uniform over ALL keys (incl. future ones) -- the fused kernels must reproduce that and its gradient, so the
    causal tile skipping is disabled for such blocks."""
    from neunet_hip.nn.experimental import attention as A
    import torch
    rng = np.random.default_rng(3)
    B, Tn, H, D = 2, 200, 2, 128
    q, k, v, do = [dev(rng.standard_normal((B, Tn, D)).astype(np.float32)) for _ in range(4)]
    kvh = np.ones((B, Tn), np.int32)
    kvh[0, :70] = 0            # leading padding: queries 0..69 of batch 0 see no valid key
    kvh[1, 5:9] = 0
    kv = dev(kvh)
    scale = float(np.sqrt(D))
    ctx_u, attn, _ = A.attention_forward(q, k, v, kv, H, scale, True)
    dq_u, dk_u, dv_u = A.attention_backward(q, k, v, attn, kv, H, scale, True, do)
    ctx_f, lse = A.fused_attention_forward(q, k, v, kv, H, scale, True)
    dq_f, dk_f, dv_f = A.fused_attention_backward(q, k, v, kv, ctx_f, lse, H, scale, True, do)
    for a, b, name in ((ctx_f, ctx_u, "ctx"), (dq_f, dq_u, "dq"), (dk_f, dk_u, "dk"), (dv_f, dv_u, "dv")):
        np.testing.assert_allclose(host(a), host(b), rtol=1e-4, atol=1e-5, err_msg=name)


@pytest.mark.parametrize("B,Tq,Tk,H,causal,ld3", [(2, 96, 200, 2, True, False), (1, 200, 96, 1, True, False),
                                                   (2, 130, 257, 2, False, True), (3, 64, 64, 4, True, True)])
def test_fused_attention_rectangular_and_strided(hip, B, Tq, Tk, H, causal, ld3):
    """Tq != Tk (the causal diagonal is shifted by Tk - Tq, as nnhipMaskedSoftmax does) and q/k/v given as column blocks
    of one wider buffer (row stride 3D, the fused q|k|v projection layout): forward and all three gradients equal the
    GEMM + masked-softmax path."""
    from neunet_hip.nn.experimental import attention as A
    import torch
    rng = np.random.default_rng(Tq + Tk)
    D = H * 64
    kvh = np.ones((B, Tk), np.int32)
    kvh[0, -Tk // 4:] = 0
    kv = dev(kvh)
    scale = float(np.sqrt(D))
    qc = dev(rng.standard_normal((B, Tq, D)).astype(np.float32))
    kc = dev(rng.standard_normal((B, Tk, D)).astype(np.float32))
    vc = dev(rng.standard_normal((B, Tk, D)).astype(np.float32))
    do = dev(rng.standard_normal((B, Tq, D)).astype(np.float32))
    ctx_u, attn, _ = A.attention_forward(qc, kc, vc, kv, H, scale, causal)
    dq_u, dk_u, dv_u = A.attention_backward(qc, kc, vc, attn, kv, H, scale, causal, do)
    q, k, v = qc, kc, vc
    if ld3:   # column blocks of [B,T,3D] buffers: one common row stride, batch stride = rows * stride
        qbuf, kbuf = torch.zeros((B, Tq, 3 * D), device="cuda"), torch.zeros((B, Tk, 3 * D), device="cuda")
        qbuf[:, :, 0:D].copy_(qc)
        kbuf[:, :, D:2 * D].copy_(kc)
        kbuf[:, :, 2 * D:].copy_(vc)
        q, k, v = qbuf[:, :, 0:D], kbuf[:, :, D:2 * D], kbuf[:, :, 2 * D:]
    ctx_f, lse = A.fused_attention_forward(q, k, v, kv, H, scale, causal)
    out = None
    if ld3:
        gq, gk = torch.zeros((B, Tq, 3 * D), device="cuda"), torch.zeros((B, Tk, 3 * D), device="cuda")
        out = (gq[:, :, 0:D], gk[:, :, D:2 * D], gk[:, :, 2 * D:])
    dq_f, dk_f, dv_f = A.fused_attention_backward(q, k, v, kv, ctx_f, lse, H, scale, causal, do, out=out)
    for a, b, name in ((ctx_f, ctx_u, "ctx"), (dq_f, dq_u, "dq"), (dk_f, dk_u, "dk"), (dv_f, dv_u, "dv")):
        np.testing.assert_allclose(host(a.contiguous()), host(b), rtol=1e-4, atol=2e-5, err_msg=name)


def test_fused_attention_fuzz(hip):
    """25 random (B, H, Tq, Tk, causal, padding pattern) cases: the fused kernels against the GEMM + masked-softmax path
    (itself pinned to the oracle and the notebook goldens), forward and all three gradients."""
    from neunet_hip.nn.experimental import attention as A
    rng = np.random.default_rng(77)
    for case in range(25):
        B, H = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        Tq = int(rng.choice([1, 5, 31, 32, 33, 64, 100, 128, 129, 200, 256, 300, 385]))
        Tk = Tq if case % 3 else int(rng.choice([1, 17, 64, 130, 256, 320]))
        causal = bool(case % 2)
        D = H * 64
        q = dev(rng.standard_normal((B, Tq, D)).astype(np.float32) * 2)
        k = dev(rng.standard_normal((B, Tk, D)).astype(np.float32) * 2)
        v = dev(rng.standard_normal((B, Tk, D)).astype(np.float32))
        do = dev(rng.standard_normal((B, Tq, D)).astype(np.float32))
        kvh = (rng.random((B, Tk)) > (0.0 if case % 4 == 0 else 0.2)).astype(np.int32)
        if case % 5 == 1:
            kvh[0, : Tk // 2 + 1] = 0                       # leading padding: fully-masked query rows under the causal mask
        kv = None if case % 7 == 3 else dev(kvh)
        scale = float(np.sqrt(D))
        ctx_u, attn, _ = A.attention_forward(q, k, v, kv, H, scale, causal)
        gu = A.attention_backward(q, k, v, attn, kv, H, scale, causal, do)
        ctx_f, lse = A.fused_attention_forward(q, k, v, kv, H, scale, causal)
        gf = A.fused_attention_backward(q, k, v, kv, ctx_f, lse, H, scale, causal, do)
        tag = f"case {case}: B{B} H{H} Tq{Tq} Tk{Tk} causal={causal}"
        np.testing.assert_allclose(host(ctx_f), host(ctx_u), rtol=1e-4, atol=2e-5, err_msg=tag + " ctx")
        for a, b, n in zip(gf, gu, "qkv"):
            np.testing.assert_allclose(host(a), host(b), rtol=1e-4, atol=5e-5, err_msg=tag + " d" + n)


@pytest.mark.parametrize("B,H,ld3", [(1, 1, False), (1, 3, True), (3, 8, True), (5, 2, False)])
def test_attention_balanced_t256_kernels(hip, monkeypatch, B, H, ld3):
    """csrc/attention_sb.hip (causal T = 256, head dim 64: the C4 shape) against the GEMM + masked-softmax path AND the tiled
    kernels it replaces there (NNHIP_ATTN_SB=0), forward and all three gradients, for every padding pattern the reference's
    where(mask == 0, -1e9) semantics distinguishes (none, trailing, holes, leading padding = fully-masked rows, both); an odd
    number of (batch, head) slices (the last block has no second slice); q / k / v as column blocks of one [B,T,3D] buffer; the
    single-pass backward is deterministic (dQ contributions are added in a fixed order, no atomics)."""
    from neunet_hip.nn.experimental import attention as A
    Tn, D = 256, H * 64
    rng = np.random.default_rng(B * 100 + H)
    scale = float(np.sqrt(D))
    pats = {"none": None}
    kv = np.ones((B, Tn), np.int32); kv[0, -Tn // 5:] = 0; pats["trailing"] = kv
    pats["holes"] = (rng.random((B, Tn)) > 0.2).astype(np.int32)
    kv = np.ones((B, Tn), np.int32); kv[0, :70] = 0; kv[-1, 3:9] = 0; pats["leading"] = kv
    kv = (rng.random((B, Tn)) > 0.3).astype(np.int32); kv[0, :140] = 0; pats["leading+holes"] = kv
    for name, kvh in pats.items():
        kvd = None if kvh is None else dev(kvh)
        if ld3:
            buf = dev(rng.standard_normal((B, Tn, 3 * D)).astype(np.float32) * 1.5)
            q, k, v = buf[..., 0:D], buf[..., D:2 * D], buf[..., 2 * D:]
        else:
            q, k, v = [dev(rng.standard_normal((B, Tn, D)).astype(np.float32) * 1.5) for _ in range(3)]
        do = dev(rng.standard_normal((B, Tn, D)).astype(np.float32))
        ctx_u, attn, _ = A.attention_forward(q.contiguous(), k.contiguous(), v.contiguous(), kvd, H, scale, True)
        g_u = A.attention_backward(q.contiguous(), k.contiguous(), v.contiguous(), attn, kvd, H, scale, True, do)

        def grads(ctx, lse):
            out = None
            if ld3:
                gb = torch.zeros((B, Tn, 3 * D), device="cuda")
                out = (gb[..., 0:D], gb[..., D:2 * D], gb[..., 2 * D:])
            return [t.clone() for t in A.fused_attention_backward(q, k, v, kvd, ctx, lse, H, scale, True, do, out=out)]
        monkeypatch.setenv("NNHIP_ATTN_SB", "1")
        ctx_s, lse_s = A.fused_attention_forward(q, k, v, kvd, H, scale, True)
        g_s, g_s2 = grads(ctx_s, lse_s), grads(ctx_s, lse_s)
        monkeypatch.setenv("NNHIP_ATTN_SB", "0")
        ctx_t, lse_t = A.fused_attention_forward(q, k, v, kvd, H, scale, True)
        g_t = grads(ctx_t, lse_t)
        g_ts = grads(ctx_s, lse_s)      # the tiled backward on the balanced forward's (lazy maximum, log2 sum) pair: a consistent pair
        monkeypatch.setenv("NNHIP_ATTN_SB", "1")
        tag = f"B{B} H{H} {name}"
        np.testing.assert_allclose(host(ctx_s), host(ctx_u), rtol=1e-4, atol=2e-5, err_msg=tag + " ctx")
        np.testing.assert_allclose(host(ctx_s), host(ctx_t), rtol=1e-4, atol=2e-5, err_msg=tag + " ctx vs tiled")
        for a, a2, b, c, d, n in zip(g_s, g_s2, g_u, g_t, g_ts, "qkv"):
            assert torch.equal(a, a2), tag + f" d{n}: two launches differ"
            assert_close_scaled(host(a), host(b), err_msg=tag + " d" + n)
            assert_close_scaled(host(c), host(b), err_msg=tag + " tiled d" + n)
            assert_close_scaled(host(d), host(b), err_msg=tag + " tiled backward on the balanced forward's statistics, d" + n)


def test_attention_sb_counted_waits_match_full_drain(hip):
    """csrc/attention_sb.hip orders its operand stream with hand-counted `s_waitcnt vmcnt(N)` around inline-asm buffer loads that
    hipcc does not count -- correct today, one edit away from a silent race (round-5 review).  The -DSB_CHECK build
    (lib/libneunet_hip.sbcheck.so, built by __graft_entry__.build()) replaces every counted wait by vmcnt(0): whatever the
    default build computes with its counts must be what the fully drained build computes, BIT FOR BIT -- forward output, row
    statistics and all three gradients, at the C4 shape (three launches), odd slice counts and the padding patterns
    (tools/attn_sb_digest.py, one process per library)."""
    import json
    import subprocess
    import sys
    from neunet_hip import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    chk = os.path.join(os.path.dirname(_lib.DEFAULT_LIB), "libneunet_hip.sbcheck.so")
    assert os.path.exists(chk), f"{chk} is missing: python -c 'import __graft_entry__ as g; g.build()' builds it"

    def run(lib):
        env = dict(os.environ)
        env.pop(_lib.LIB_ENV, None)
        if lib:
            env[_lib.LIB_ENV] = lib
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "attn_sb_digest.py")], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    a, b = run(None), run(chk)
    assert a.pop("lib") == "libneunet_hip.so" and b.pop("lib") == "libneunet_hip.sbcheck.so"
    assert a.keys() == b.keys() and len(a) >= 20
    bad = [k for k in a if a[k] != b[k]]
    assert not bad, f"counted waits and full drains disagree: {bad}"


def test_attention_sb_forward_wave_private_tiles_variant(hip):
    """Round 6: NNHIP_ATTN_SB_FWD=pw runs the balanced forward with its K / V operands parked in wave-private LDS tiles (whole-row
    loads one unit ahead) instead of streamed into the MFMA registers -- measured 5-8 % slower on MI355X and therefore not the
    default, but kept as a switch: same key-group order, same arithmetic, so everything the forward writes -- and with it every
    gradient of the backward that consumes its statistics -- must be BIT-IDENTICAL to the default, padding patterns and odd slice
    counts included (tools/attn_sb_digest.py, one process per setting: the switch is read once)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(mode):
        env = dict(os.environ)
        env.pop("NNHIP_ATTN_SB_FWD", None)
        if mode:
            env["NNHIP_ATTN_SB_FWD"] = mode
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "attn_sb_digest.py")], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    a, b = run(None), run("pw")
    assert a.keys() == b.keys() and len(a) >= 20
    bad = [k for k in a if a[k] != b[k]]
    assert not bad, f"the wave-private-tile forward differs from the streamed one: {bad}"


def test_argmax_integer_tensors_and_upstream_broadcast(hip):
    """neunet.argmax takes labels / ids / masks as well (np.argmax, neunet/__init__.py:132-139): integer device tensors give
    np.argmax's indices bit for bit; loss.backward(g) broadcasts g by SHAPE (a (D,) gradient against a (B, D) 'none' loss runs
    along the last axis also when B == D)."""
    import neunet_hip
    from neunet_hip.nn.experimental.utils import times_upstream
    rng = np.random.default_rng(4)
    for dt in (np.int32, np.int16, np.int64):
        a = rng.integers(-50, 50, (7, 33)).astype(dt)
        for ax in (None, 0, 1, -1):
            got = neunet_hip.argmax(neunet_hip.Tensor(a, dtype=dt, device="cuda", requires_grad=False), axis=ax)
            np.testing.assert_array_equal(host(got.data), np.argmax(a, axis=ax).astype(np.int32))
    big = np.array([[1 << 30, (1 << 30) + 1, 5]], np.int64)                        # beyond fp32's exact integers
    got = neunet_hip.argmax(neunet_hip.Tensor(big, dtype=np.int64, device="cuda", requires_grad=False), axis=1)
    np.testing.assert_array_equal(host(got.data), np.argmax(big, axis=1).astype(np.int32))
    lg = rng.standard_normal((6, 6)).astype(np.float32)
    for g in (rng.standard_normal(6).astype(np.float32), rng.standard_normal((6, 1)).astype(np.float32),
              np.float32(1.5), rng.standard_normal((6, 6)).astype(np.float32), rng.standard_normal((1, 6)).astype(np.float32)):
        np.testing.assert_allclose(host(times_upstream(dev(lg), dev(np.asarray(g)))), lg * g, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        times_upstream(dev(lg), dev(rng.standard_normal(5).astype(np.float32)))
    lg1 = rng.standard_normal(9).astype(np.float32)                                # a 1-D 'none' loss: one value per row
    g1 = rng.standard_normal(9).astype(np.float32)
    np.testing.assert_allclose(host(times_upstream(dev(lg1), dev(g1))), lg1 * g1, rtol=1e-6, atol=0)


def test_shared_state_guard_survives_a_destroyed_stream(hip):
    """The CrossEntropy / fused-MLP launches share one set of ticket words per process; a call that arrives on another stream than
    the previous one is ordered behind it.  The previous caller's stream may be GONE by then (CuPy destroys streams on garbage
    collection; round-4 advisor): the guard must neither fail nor poison later calls."""
    import gc
    from neunet_hip.nn.experimental.losses import cross_entropy_forward_backward
    rng = np.random.default_rng(9)
    x = rng.standard_normal((300, 70)).astype(np.float32)
    y = rng.integers(0, 70, 300).astype(np.int32)
    ref_rows, _ = O.cross_entropy_forward_backward(x, y, ignore_index=-100, reduction="none")
    import ctypes
    hiprt = ctypes.CDLL("libamdhip64.so")
    for _ in range(3):
        raw = ctypes.c_void_p()
        assert hiprt.hipStreamCreate(ctypes.byref(raw)) == 0
        st = torch.cuda.ExternalStream(raw.value)
        with torch.cuda.stream(st):
            rows, _ = cross_entropy_forward_backward(dev(x), dev(y), "none", -100)
            st.synchronize()
        np.testing.assert_allclose(host(rows), ref_rows, rtol=1e-5, atol=1e-5)
        del st
        gc.collect()
        assert hiprt.hipStreamDestroy(raw) == 0                                    # the previous caller's stream no longer exists
        rows, _ = cross_entropy_forward_backward(dev(x), dev(y), "none", -100)     # back on the default stream
        torch.cuda.synchronize()
        np.testing.assert_allclose(host(rows), ref_rows, rtol=1e-5, atol=1e-5)
    # round 6: a stream change waits for the previous user's EVENT (recorded behind its launches), not for the whole device.  Two live
    # streams taking turns on the shared ticket words and loss partials, no host synchronisation in between: every 'mean' loss must
    # be the reference's (an unordered pair of launches would mix their partial sums and tickets)
    ref_mean, _ = O.cross_entropy_forward_backward(x, y, ignore_index=-100, reduction="mean")
    big_x = dev(np.tile(x, (40, 1)))                                               # 12000 rows: long enough to overlap if unordered
    big_y = dev(np.tile(y, 40))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    losses = []
    for k in range(12):
        with torch.cuda.stream(s1 if k % 2 == 0 else s2):
            loss, _ = cross_entropy_forward_backward(big_x, big_y, "mean", -100)
            losses.append(loss)
    torch.cuda.synchronize()
    for l_ in losses:
        np.testing.assert_allclose(float(host(l_).reshape(-1)[0]), float(ref_mean), rtol=2e-5)


def test_gpt_step_fused_attention_equals_unfused(hip):
    """A GPT step (d 128, 2 heads of 64) with the fused attention kernels gives the same loss and gradients as
    the GEMM + masked-softmax path (which the gpt_tiny golden pins to the reference)."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    V, D, H, F, L, B, Tn = 97, 128, 2, 256, 2, 3, 70
    rng = np.random.default_rng(11)
    batch = rng.integers(1, V, (B, Tn + 1)).astype(np.int32)
    batch[0, -9:] = 0
    grads, losses = [], []
    for fa in (False, True):
        np.random.seed(21)
        model = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=128, fused=True, fused_attention=fa)
        loss_fn = nn.CrossEntropyLoss(ignore_index=0)
        out, attn = model.forward(batch[:, :-1])
        assert (attn is None) == fa
        loss = loss_fn(out.reshape(B * Tn, V), T(hip, np.ascontiguousarray(batch[:, 1:]).reshape(-1), dtype=np.int32,
                                                 requires_grad=False))
        loss.backward()
        losses.append(loss.item())
        grads.append([None if p.grad is None else host(p.grad) for p in model.parameters()])
    assert abs(losses[0] - losses[1]) < 1e-5
    for i, (a, b) in enumerate(zip(*grads)):
        assert (a is None) == (b is None)
        if a is not None:
            assert_close_scaled(b, a, err_msg=f"grad {i}", scale=grad_list_scale(grads[0]))


@pytest.mark.parametrize("fused", [False, True])
def test_gpt_tiny_step_golden(hip, golden, fused):
    """One full training step of the notebook's GPT (2 layers, d 32, 4 heads, vocab 50, repeated ids, PAD tail):
    logits, loss, every gradient (incl. None for the never-called cross_attn) and every parameter after Adam."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    g = golden("gpt_tiny")
    V, D, H, F, L = [int(v) for v in g["cfg"]]
    model = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=64, fused=fused)
    params = model.parameters()
    assert len(params) == int(g["n_params"])
    for i, p in enumerate(params):
        assert tuple(p.shape) == g[f"p{i}"].shape, (i, p.shape, g[f"p{i}"].shape)
        p.data.copy_(dev(g[f"p{i}"]))
    opt = Adam(params, lr=1.5e-4, betas=(0.9, 0.98), eps=1e-9)
    loss_fn = nn.CrossEntropyLoss(ignore_index=0)
    batch = g["batch"]
    output, _ = model.forward(batch[:, :-1])
    np.testing.assert_allclose(host(output.data), g["logits"], rtol=1e-4, atol=1e-4)
    out2 = output.reshape(output.shape[0] * output.shape[1], output.shape[2])
    loss = loss_fn(out2, T(hip, np.ascontiguousarray(batch[:, 1:]).reshape(-1), dtype=np.int32, requires_grad=False))
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    gscale = grad_list_scale([g[f"g{i}"] for i in range(len(params)) if bool(g[f"has_grad{i}"])])
    for i, p in enumerate(params):
        if bool(g[f"has_grad{i}"]):
            assert_close_scaled(host(p.grad), g[f"g{i}"], err_msg=f"grad {i}", scale=gscale)
        else:
            assert p.grad is None, i
    our_grads = [None if p.grad is None else host(p.grad) for p in params]
    opt.step()
    for i, p in enumerate(params):
        got = host(p.data)
        if not bool(g[f"has_grad{i}"]):
            np.testing.assert_array_equal(got, g[f"p{i}"], err_msg=f"param {i} (no grad -> untouched)")
            continue
        # (1) the fused Adam applied to OUR gradient == the oracle's Adam on the same gradient, everywhere
        ref = g[f"p{i}"].copy()
        O.adam_step(ref, our_grads[i], np.zeros_like(ref), np.zeros_like(ref), 1, 1.5e-4, (0.9, 0.98), 1e-9, 0.0)
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6, err_msg=f"param {i} vs oracle Adam")
        # (2) against the reference's own post-step parameters wherever the gradient is above rounding noise
        #     (Adam's first step moves by lr*sign(g): a ~1e-9 gradient such as wk.bias -- mathematically zero,
        #     softmax is shift-invariant -- turns rounding noise into a full +-lr step in BOTH implementations)
        sig = np.abs(g[f"g{i}"]) > 1e-5
        np.testing.assert_allclose(got[sig], g[f"p_after{i}"][sig], rtol=1e-4, atol=2e-5, err_msg=f"param {i}")


@pytest.mark.parametrize("fused", [False, True])
def test_reference_checkpoint_loads_and_reproduces_the_reference_logits(hip, golden, fused, tmp_path):
    """a checkpoint written BY THE REFERENCE (neunet.save(model.state_dict()) -> pickle of an OrderedDict of
    NumPy arrays, neunet/__init__.py:26-29, nn/modules.py:76-86; tests/golden/gpt_tiny_state.pkl) loads through
    neunet_hip.load + Module.load_state_dict and the HIP forward reproduces the reference's logits; our own
    save(state_dict()) round-trips to the identical dictionary (same keys, same order, same arrays)."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    from conftest import GOLDEN
    g = golden("gpt_tiny")
    V, D, H, F, L = [int(v) for v in g["cfg"]]
    np.random.seed(99)                                           # a different init: everything must come from the file
    model = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=64, fused=fused)
    sd = hip.load(os.path.join(GOLDEN, "gpt_tiny_state.pkl"))
    assert list(model.state_dict()) == list(sd)                  # the reference's key names, in its order
    model.load_state_dict(sd)
    out, _ = model.forward(g["batch"][:, :-1])
    np.testing.assert_allclose(host(out.data), g["logits"], rtol=1e-4, atol=1e-4)
    path = str(tmp_path / "ours.pkl")
    hip.save(model.state_dict(), path)
    back = hip.load(path)
    assert list(back) == list(sd)
    for k in sd:
        assert isinstance(back[k], np.ndarray) and back[k].dtype == sd[k].dtype
        np.testing.assert_array_equal(back[k], sd[k], err_msg=k)


@pytest.mark.parametrize("dropout,fused", [(0.0, True), (0.1, True), (0.0, False)])
def test_gpt_tiny_learns(hip, dropout, fused):
    """End to end: the notebook's GPT on a deterministic next-token task -- the loss falls from ~ln(V) to well under a
    third of it in 150 Adam steps, through the fused kernels (flash attention, fused q|k|v, epilogue fusions), through
    the plain ones, and with the notebook's dropout 0.1 (device-RNG masks, attention dropout included)."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    np.random.seed(3)
    V, D, H, L, B, Tn = 96, 128, 2, 2, 16, 32
    model = gpt_tiny.build_gpt(V, D, H, 2 * D, L, pad_idx=0, max_len=Tn + 1, fused=fused, dropout=dropout)
    opt = Adam(model.parameters(), lr=2e-3, betas=(0.9, 0.98), eps=1e-9)
    loss_fn = nn.CrossEntropyLoss(ignore_index=0)
    losses = [gpt_tiny.train_step(model, opt, loss_fn, b).item() for b in gpt_tiny.synthetic_batches(V, B, Tn, 150, seed=1)]
    assert np.isfinite(losses).all()
    assert losses[0] > 0.8 * np.log(V - 1)
    assert np.mean(losses[-10:]) < 0.3 * losses[0], (losses[0], losses[-10:])


@pytest.mark.parametrize("rows,inf,classes,reduction", [(32, 128, 10, "mean"), (200, 784, 10, "sum"), (256, 2048, 32, "none"),
                                                         (7, 50, 3, "mean"), (64, 33, 1, "mean")])
def test_linear_cross_entropy_fused(hip, rows, inf, classes, reduction):
    """nnhipLinearCrossEntropyLoss (a small classifier head and its loss in one launch): logits, loss, d(logits) against the
    oracle, and bit-identical to nnhipLinearModuleForward followed by nnhipCrossEntropyLossEx; ignored and out-of-range labels,
    class weights.  Module level: CrossEntropyLoss applied to a pending Linear output takes the fused entry and the backward pass
    gives the gradients of the unfused tape."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    import neunet_hip.nn as nn
    import torch
    rng = np.random.default_rng(rows + inf + classes)
    st = get_current_stream_ptr()
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    W = (rng.standard_normal((classes, inf)) / np.sqrt(inf)).astype(np.float32)
    b = rng.standard_normal((1, classes)).astype(np.float32)
    IGN = 0                                                    # an in-range ignore_index: the oracle gathers weight[label] first
    Y = rng.integers(0, classes, rows).astype(np.int32)
    Y[::5] = IGN
    cw = rng.uniform(0.5, 2.0, classes).astype(np.float32)
    red = {"mean": b"m", "sum": b"s", "none": b"n"}[reduction]
    x, w, bb, y, cwd = dev(X), dev(W), dev(b), dev(Y), dev(cw)

    def run(fused, weight):
        logits = torch.full((rows, classes), float("nan"), device="cuda")
        dl = torch.full((rows, classes), float("nan"), device="cuda")
        lr, lse = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
        loss = torch.full((), float("nan"), device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        if fused:
            call("nnhipLinearCrossEntropyLoss", x, w, bb, logits, dl, lr, lse, y, 4, weight, IGN, rows, inf, classes, red,
                 None if reduction == "none" else loss, cnt if reduction == "mean" else None, st)
        else:
            call("nnhipLinearModuleForward", x, w, bb, logits, rows, inf, classes, st)
            call("nnhipCrossEntropyLossEx", logits, dl, lr, lse, y, 4, weight, classes, IGN, rows, classes, red,
                 None if reduction == "none" else loss, cnt if reduction == "mean" else None, st)
        return logits, dl, lr, lse, loss, cnt

    for weight in (None, cwd):
        f, u = run(True, weight), run(False, weight)
        assert torch.equal(f[0], u[0])                         # the logits: same tile code, same wave split
        for name, a, c in zip(("dlogits", "loss_rows", "lse"), f[1:4], u[1:4]):   # same formulas, a 512- vs 1024-thread block
            np.testing.assert_allclose(host(a), host(c), rtol=2e-6, atol=1e-7, err_msg=name)
        if reduction != "none":
            np.testing.assert_allclose(host(f[4]), host(u[4]), rtol=2e-6, atol=1e-7)
        if reduction == "mean":
            assert int(f[5].item()) == int(u[5].item())
        z = O.linear_forward(X, W, b)
        np.testing.assert_allclose(host(f[0]), z, **TOL)
        if classes > 1:                                        # (one class, every label ignored: 0/0 in the oracle's mean)
            want_loss, want_grad = O.cross_entropy_forward_backward(z, Y, None if weight is None else cw, IGN, reduction)
            got_loss = host(f[2]) if reduction == "none" else host(f[4])
            np.testing.assert_allclose(got_loss, want_loss, rtol=1e-4, atol=1e-5)
            assert_close_scaled(host(f[1]), want_grad)

    # module level: the tape with and without the fusion
    def tape(fuse):
        np.random.seed(9)
        lin = nn.Linear(inf, classes)
        xt = T(hip, X)
        out = lin(xt)
        if not fuse:
            out.data                                           # materialise the Linear first: the two-launch path
        loss = nn.CrossEntropyLoss(reduction=reduction, ignore_index=IGN)(out, hip.Tensor(Y, dtype=np.int32, device="cuda", requires_grad=False))
        if reduction == "none":
            loss.backward(dev(np.ones(rows, np.float32)))
        else:
            loss.backward()
        return host(loss.data), host(out.data), host(xt.grad), host(lin.weight.grad), host(lin.bias.grad)

    for a, c in zip(tape(True), tape(False)):
        np.testing.assert_allclose(a, c, rtol=1e-5, atol=1e-6)


def test_graphed_step_unrolled(hip):
    """GraphedTrainStep(unroll=U): U consecutive training steps captured into one graph (each reading its own static batch
    slot) leave exactly the parameters of U single-step replays and of the eager loop -- README quick-start MLP, Adam with
    its device-side step counter and cached bias corrections, 3 replays of 4 steps."""
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    U, R, B = 4, 3, 32
    rng = np.random.default_rng(11)
    data = [(rng.uniform(-1, 1, (B, 784)).astype(np.float32), rng.integers(0, 10, B).astype(np.int32)) for _ in range(2 + U * R)]

    class MLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.l1, self.relu, self.l2 = nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)

        def forward(self, x):
            return self.l2(self.relu(self.l1(x)))

    def make(unroll):
        np.random.seed(42)
        model = MLP()
        xs = [hip.Tensor(data[0][0], device="cuda", requires_grad=False) for _ in range(unroll)]
        ys = [hip.Tensor(data[0][1], dtype=np.int32, device="cuda", requires_grad=False) for _ in range(unroll)]
        loss_fn = nn.CrossEntropyLoss()

        def fb(k=0):
            loss = loss_fn(model(xs[k]), ys[k])
            loss.backward()
            return loss

        opt = Adam(model.parameters(), lr=1e-3)
        return model, xs, ys, fb, opt, GradBucket(model.parameters())

    def feed(xs, ys, k, item):
        xs[k].data.copy_(dev(item[0]))
        ys[k].data.copy_(dev(item[1]))

    # eager reference: 2 warm-up steps on item 0 / 1 (what the graphed objects run before capture), then U*R steps
    m0, xs0, ys0, fb0, opt0, bk0 = make(1)
    for item in data:
        feed(xs0, ys0, 0, item)
        opt0.zero_grad()
        fb0()
        opt0.step()
    want = [host(p.data) for p in m0.parameters()]

    for unroll in (1, U):
        m, xs, ys, fb, opt, bk = make(unroll)
        warm = iter(data[:2])

        def fb_warm(k=0, fb=fb, xs=xs, ys=ys, warm=warm):
            item = next(warm, None)
            if item is not None:                         # the two eager warm-up steps read items 0 and 1 through slot 0
                feed(xs, ys, 0, item)
            return fb(k)

        g = GraphedTrainStep(fb_warm, opt, bk, warmup=2, unroll=unroll)
        rest = data[2:]
        for r in range(len(rest) // unroll):
            for k in range(unroll):
                feed(xs, ys, k, rest[r * unroll + k])
            g()
        got = [host(p.data) for p in m.parameters()]
        g.release()
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)


def test_graphed_conv_classifier_equals_eager(hip):
    """The conv classifier's step with every round-3 shortcut on (deferred conv launches, conv + LeakyReLU + MaxPool forward as one
    kernel per layer, first-layer weight gradient off the pool's gradient, the layers' reduces queued and launched as one grid out
    of their own arena) captured into hipGraphs -- one step per graph and four -- leaves exactly the parameters of the eager
    loop: nothing the capture bakes in (arena and workspace addresses, queue state) differs between replays."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import conv_classifier
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    U, R, B = 4, 2, 176                                   # 176 x 14 x 14 windows: enough for the first layer's one-thread-per-window kernel
    rng = np.random.default_rng(12)
    data = [(rng.uniform(-1, 1, (B, 1, 28, 28)).astype(np.float32), np.eye(10, dtype=np.float32)[rng.integers(0, 10, B)])
            for _ in range(2 + U * R)]

    def make(unroll):
        np.random.seed(43)
        model = conv_classifier.Conv2dClassifier()
        xs = [hip.Tensor(data[0][0], device="cuda", requires_grad=False) for _ in range(unroll)]
        ts = [hip.Tensor(data[0][1], device="cuda", requires_grad=False) for _ in range(unroll)]
        loss_fn = nn.MSELoss()

        def fb(k=0):
            loss = loss_fn(model(xs[k]), ts[k])
            loss.backward()
            return loss

        opt = Adam(model.parameters(), lr=1e-3)
        return model, xs, ts, fb, opt, GradBucket(model.parameters())

    def feed(xs, ts, k, item):
        xs[k].data.copy_(dev(item[0]))
        ts[k].data.copy_(dev(item[1]))

    m0, xs0, ts0, fb0, opt0, _ = make(1)
    for item in data:
        feed(xs0, ts0, 0, item)
        opt0.zero_grad()
        fb0()
        opt0.step()
    want = [host(p.data) for p in m0.parameters()]
    for unroll in (1, U):
        m, xs, ts, fb, opt, bk = make(unroll)
        warm = iter(data[:2])

        def fb_warm(k=0, fb=fb, xs=xs, ts=ts, warm=warm):
            item = next(warm, None)
            if item is not None:
                feed(xs, ts, 0, item)
            return fb(k)

        g = GraphedTrainStep(fb_warm, opt, bk, warmup=2, unroll=unroll)
        rest = data[2:]
        for r in range(len(rest) // unroll):
            for k in range(unroll):
                feed(xs, ts, k, rest[r * unroll + k])
            g()
        got = [host(p.data) for p in m.parameters()]
        g.release()
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)


def test_graphed_step_equals_eager(hip):
    """A hipGraph-replayed GPT step (neunet_hip.graph.GraphedTrainStep, device-side Adam step counter) produces
    the same parameters as the eager step, step after step, with fresh data copied into the static buffers."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    V, D, H, F, L, B, Tn = 61, 32, 4, 64, 2, 3, 12
    rng = np.random.default_rng(77)
    batches = [rng.integers(1, V, (B, Tn + 1)).astype(np.int32) for _ in range(6)]
    for b in batches:
        b[0, -3:] = 0

    def make():
        np.random.seed(5)
        model = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=32)
        ids = hip.Tensor(batches[0][:, :-1], dtype=np.int32, requires_grad=False, device="cuda")
        tgt = hip.Tensor(np.ascontiguousarray(batches[0][:, 1:]).reshape(-1), dtype=np.int32, requires_grad=False, device="cuda")
        loss_fn = nn.CrossEntropyLoss(ignore_index=0)

        def fb():
            out, _ = model.forward(ids)
            loss = loss_fn(out.reshape(B * Tn, V), tgt)
            loss.backward()
            return loss

        fb()
        active = [p for p in model.parameters() if p.grad is not None]
        for p in model.parameters():
            p.grad = None
        opt = Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
        return model, ids, tgt, fb, opt, GradBucket(active)

    def feed(ids, tgt, b):
        ids.data.copy_(dev(np.ascontiguousarray(b[:, :-1])))
        tgt.data.copy_(dev(np.ascontiguousarray(b[:, 1:]).reshape(-1)))

    m1, ids1, tgt1, fb1, opt1, bk1 = make()
    losses1 = []
    for b in [batches[0], batches[0]] + batches:      # the graphed run warms up twice on batch 0 first
        feed(ids1, tgt1, b)
        opt1.zero_grad()
        losses1.append(fb1().item())
        bk1.all_reduce()
        opt1.step()

    m2, ids2, tgt2, fb2, opt2, bk2 = make()
    feed(ids2, tgt2, batches[0])
    g = GraphedTrainStep(fb2, opt2, bk2, warmup=2)       # warm-up (eager) grows the workspace / uploads the plan
    losses2 = []
    for b in batches:
        feed(ids2, tgt2, b)
        losses2.append(g().item())
    np.testing.assert_allclose(losses2, losses1[2:], rtol=1e-5, atol=1e-6)
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        np.testing.assert_allclose(host(p2.data), host(p1.data), rtol=1e-5, atol=1e-6)
    # an LR schedule between replays takes effect (lr lives in the optimizer's device state, not in the captured arguments)
    opt1.lr = opt2.lr = 3e-4
    feed(ids1, tgt1, batches[1])
    opt1.zero_grad()
    fb1()
    bk1.all_reduce()
    opt1.step()
    feed(ids2, tgt2, batches[1])
    g()
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        np.testing.assert_allclose(host(p2.data), host(p1.data), rtol=1e-5, atol=1e-6)
    # moving a parameter after capture is detected instead of silently training on stale memory
    first = m2.parameters()[0]
    first.data = first.data.clone()
    g._calls = 0
    with pytest.raises(RuntimeError, match="moved since capture"):
        g()
    g.release()


def _c4_batch(rng, B, Tn, vocab):
    ids = rng.integers(3, vocab, (B, Tn + 1)).astype(np.int32)
    for r in rng.choice(B, max(1, B // 10), replace=False):      # ~10 % of rows PAD-tailed (bench.py's c4_batch)
        ids[r, -int(rng.integers(8, Tn // 4)):] = 0
    return ids


def test_gpt_c4_full_size_properties(hip):
    """BASELINE C4 at FULL size (B 64 x T 256, d 512, 6 layers, 8 heads, d_ff 2048, vocab 15000 -> 16384 x 15000 logits,
    983 MB): the shapes only this configuration reaches -- the 16384x512->15000 head GEMM (N not a tile multiple), the
    1024-thread CrossEntropy tile at 15000 columns, the split-K dW with a 16384-long reduction, db inside the dW GEMM --
    checked through properties the oracle can afford: sampled rows/columns against float64 dot products, per-row losses
    against the float64 log-sum-exp, gradient rows summing to zero, ignored rows exactly zero, fused == unfused
    attention, Adam step against the oracle's Adam on our gradient."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    from neunet_hip.nn.experimental.losses import cross_entropy_forward_backward
    from neunet_hip.optim import Adam
    V, D, H, F, L, B, Tn = 15000, 512, 8, 2048, 6, 64, 256
    rng = np.random.default_rng(1004)
    batch = _c4_batch(rng, B, Tn, V)
    ids_np, tgt_np = np.ascontiguousarray(batch[:, :-1]), np.ascontiguousarray(batch[:, 1:]).reshape(-1)
    rows = B * Tn
    np.random.seed(1004)
    model = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=1024, fused=True)
    params = model.parameters()
    opt = Adam(params, lr=1.5e-4, betas=(0.9, 0.98), eps=1e-9)
    loss_fn = nn.CrossEntropyLoss(ignore_index=0)
    tgt = T(hip, tgt_np, dtype=np.int32, requires_grad=False)
    out, attn = model.forward(ids_np)
    assert attn is None and tuple(out.shape) == (B, Tn, V)
    fc_out = model.decoder.fc_out
    xf = out.args[0]                                             # the Linear node's input: final hidden states [B,T,D]
    Xf = host(xf.data).reshape(rows, D).astype(np.float64)
    Wf, bf = host(fc_out.weight.data).astype(np.float64), host(fc_out.bias.data).astype(np.float64)
    logits = out.data.reshape(rows, V)
    # (1) head GEMM 16384x512 -> 15000: sampled rows against float64 dot products
    sel = np.sort(rng.choice(rows, 24, replace=False))
    sel_d = torch.from_numpy(sel).cuda()
    lg = host(logits[sel_d])
    np.testing.assert_allclose(lg, Xf[sel] @ Wf.T + bf, rtol=1e-4, atol=1e-4)
    # (2) CrossEntropy at 16384 x 15000: per-row loss vs float64 log-sum-exp on the sample; mean == sum / count
    loss_rows, dl_none = cross_entropy_forward_backward(logits, tgt.data, "none", 0)
    lg64 = lg.astype(np.float64)
    lse = np.log(np.exp(lg64 - lg64.max(1, keepdims=True)).sum(1)) + lg64.max(1)
    ref_rows = np.where(tgt_np[sel] != 0, lse - lg64[np.arange(len(sel)), tgt_np[sel]], 0.0)
    np.testing.assert_allclose(host(loss_rows[sel_d]), ref_rows, rtol=1e-5, atol=1e-5)
    del dl_none
    loss = loss_fn(out.reshape(rows, V), tgt)
    cnt = int((tgt_np != 0).sum())
    assert abs(loss.item() - float(loss_rows.double().sum().item()) / cnt) < 1e-5
    loss.backward()
    # (3) dlogits: softmax - onehot rows sum to zero, ignored rows are exactly zero, sampled rows vs float64
    dlog = out.grad.reshape(rows, V)
    assert float(dlog.sum(dim=1).abs().max()) < 1e-8
    ign = torch.from_numpy(np.nonzero(tgt_np == 0)[0]).cuda()
    assert ign.numel() > 0 and float(dlog[ign].abs().max()) == 0.0
    p64 = np.exp(lg64 - lse[:, None])
    p64[np.arange(len(sel)), tgt_np[sel]] -= 1.0
    p64[tgt_np[sel] == 0] = 0.0
    np.testing.assert_allclose(host(dlog[sel_d]), p64 / cnt, rtol=1e-4, atol=1e-10)
    # (4) fc_out.weight.grad rows (split over a 16384-long reduction) and db, sampled vocabulary rows vs float64
    vsel = np.sort(rng.choice(V, 12, replace=False))
    vsel_d = torch.from_numpy(vsel).cuda()
    dcols = host(dlog[:, vsel_d]).astype(np.float64)             # [rows, 12]
    np.testing.assert_allclose(host(fc_out.weight.grad[vsel_d]), dcols.T @ Xf, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(host(fc_out.bias.grad)[0, vsel], dcols.sum(0), rtol=1e-4, atol=1e-7)
    # dX of the head GEMM (K = 15000): sampled rows
    np.testing.assert_allclose(host(xf.grad.reshape(rows, D)[sel_d]), host(dlog[sel_d]).astype(np.float64) @ Wf,
                               rtol=1e-4, atol=1e-8)
    # (5) never-called cross_attn parameters have no gradient; everything else does and is finite
    n_none = sum(p.grad is None for p in params)
    assert n_none == 8 * L
    for p in params:
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all())
    # (6) Adam on every parameter == the oracle's Adam on our gradient (sampled slices)
    before = [host(p.data.reshape(-1)[:4096]).copy() for p in params]
    grads = [None if p.grad is None else host(p.grad.reshape(-1)[:4096]).copy() for p in params]
    opt.step()
    for p, b0, g0 in zip(params, before, grads):
        got = host(p.data.reshape(-1)[:4096])
        if g0 is None:
            np.testing.assert_array_equal(got, b0)
            continue
        ref = b0.copy()
        O.adam_step(ref, g0, np.zeros_like(ref), np.zeros_like(ref), 1, 1.5e-4, (0.9, 0.98), 1e-9, 0.0)
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)
    # (7) the same model with the GEMM + masked-softmax attention path (the one the golden pins to the reference)
    sd = model.state_dict()
    first_loss = loss.item()
    first_logits = lg
    del model, out, loss, dlog, logits, loss_rows, opt
    torch.cuda.empty_cache()
    np.random.seed(1004)
    m2 = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=1024, fused=True, fused_attention=False)
    # undo the Adam step in the copied weights: reload the pre-step values is not possible -> compare forward on the
    # POST-step weights of both paths instead (fused path recomputed below on the same weights)
    m2.load_state_dict(sd)
    out2, attn2 = m2.forward(ids_np)
    assert attn2 is not None
    lg2 = host(out2.data.reshape(rows, V)[sel_d])
    np.random.seed(1004)
    m3 = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=1024, fused=True, fused_attention=True)
    m3.load_state_dict(sd)
    out3, _ = m3.forward(ids_np)
    lg3 = host(out3.data.reshape(rows, V)[sel_d])
    assert_close_scaled(lg3, lg2)
    assert np.abs(lg3 - first_logits).max() > 0                   # the Adam step did change the weights
    assert np.isfinite(first_loss)


_C4_ORACLE = {}


def _c4_oracle_step(params_host, ids_in, targets, H, L):
    """ONE step of the oracle's GPT (examples/gpt.ipynb cells 2-12 restated in oracle/neunet_oracle.py:459) at the full C4 size on
    the given weights: ~20 s of host time, computed once per session (both attention paths start from the same seeded weights)."""
    key = (ids_in.tobytes()[:64], float(params_host[1].reshape(-1)[0]))
    if key not in _C4_ORACLE:
        P = lambda i: params_host[i]  # noqa: E731
        layers, idx = [], 1
        for _ in range(L):
            layers.append({"attn": [P(idx + j) for j in range(8)], "ffn": [P(idx + 16 + j) for j in range(4)],
                           "norm1": P(idx + 20), "norm2": P(idx + 21), "base": idx})
            idx += 22
        ref = O.GPTTiny(P(0), layers, P(idx), P(idx + 1), H, pad_idx=0, max_len=1024)
        loss, logits, grads = ref.forward_backward(ids_in, targets)
        flat = {0: grads["emb"], idx: grads["Wout"], idx + 1: grads["bout"]}
        for Ly, gl in zip(layers, grads["layers"]):
            b = Ly["base"]
            for j in range(8):
                flat[b + j] = gl["attn"][j]
            for j in range(4):
                flat[b + 16 + j] = gl["ffn"][j]
            flat[b + 20], flat[b + 21] = gl["norm1"], gl["norm2"]
        _C4_ORACLE.clear()
        _C4_ORACLE[key] = (float(loss), logits.reshape(-1, logits.shape[-1]), flat)
    return _C4_ORACLE[key]


@pytest.mark.parametrize("fused_attention", [True, False])
def test_gpt_c4_full_size_whole_step_vs_oracle(hip, fused_attention):
    """BASELINE C4 at FULL size against the reference algorithm's WHOLE step (round-4 review, item 2): the oracle's GPT
    (/root/reference/examples/gpt.ipynb cells 2-12 -> oracle GPTTiny; loss: neunet/nn/losses.py:59-126) runs forward and backward
    on the same seeded weights and the same 64 x 256 batch; loss (1e-4), sampled logits rows, and EVERY parameter gradient --
    embedding, the six decoder layers' projections / FFN / norms at 16384 rows, the vocabulary head -- are compared
    (assert_close_scaled, 1e-4).  fused_attention=True runs the balanced T = 256 kernels of csrc/attention_sb.hip (single-pass
    backward), False the GEMM + masked-softmax path."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    V, D, H, F, L, B, Tn = 15000, 512, 8, 2048, 6, 64, 256
    rng = np.random.default_rng(1004)
    batch = _c4_batch(rng, B, Tn, V)
    ids_np, tgt_np = np.ascontiguousarray(batch[:, :-1]), np.ascontiguousarray(batch[:, 1:])
    rows = B * Tn
    np.random.seed(1004)
    model = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=1024, fused=True, fused_attention=fused_attention)
    params = model.parameters()
    assert len(params) == 1 + 22 * L + 2
    params_host = [host(p.data).copy() for p in params]
    ref_loss, ref_logits, ref_grads = _c4_oracle_step(params_host, ids_np, tgt_np, H, L)
    loss_fn = nn.CrossEntropyLoss(ignore_index=0)
    tgt = T(hip, tgt_np.reshape(-1), dtype=np.int32, requires_grad=False)
    out, attn = model.forward(ids_np)
    assert (attn is None) == fused_attention
    sel = np.sort(rng.choice(rows, 64, replace=False))
    lg = host(out.data.reshape(rows, V)[torch.from_numpy(sel).cuda()])
    np.testing.assert_allclose(lg, ref_logits[sel], rtol=1e-4, atol=1e-4)
    loss = loss_fn(out.reshape(rows, V), tgt)
    assert abs(loss.item() - ref_loss) < 1e-4, (loss.item(), ref_loss)
    loss.backward()
    zscale = grad_list_scale(list(ref_grads.values()))
    n_checked = 0
    for i, p in enumerate(params):
        if i not in ref_grads:
            assert p.grad is None, f"param {i} (cross attention, never called) has a gradient"
            continue
        assert p.grad is not None, f"param {i} has no gradient"
        ref = np.asarray(ref_grads[i]).reshape(tuple(p.grad.shape))
        # the key projection's bias gradient is mathematically zero (softmax is shift invariant): both sides hold rounding noise
        assert_close_scaled(host(p.grad), ref, err_msg=f"gradient of parameter {i} {tuple(p.grad.shape)}", scale=zscale if rms_of(ref) < 1e-3 * zscale else 0.0)
        n_checked += 1
    assert n_checked == 1 + 14 * L + 2


def test_gpt_c4_full_size_graphed_equals_eager(hip):
    """The BASELINE C4 step replayed as a hipGraph (what bench.py times) == the eager step, two steps, full size."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    V, D, H, F, L, B, Tn = 15000, 512, 8, 2048, 6, 64, 256
    rng = np.random.default_rng(1004)
    batches = [_c4_batch(rng, B, Tn, V) for _ in range(2)]

    def make():
        np.random.seed(1004)
        model = gpt_tiny.build_gpt(V, D, H, F, L, pad_idx=0, max_len=1024, fused=True)
        ids = hip.Tensor(np.ascontiguousarray(batches[0][:, :-1]), dtype=np.int32, requires_grad=False, device="cuda")
        tgt = hip.Tensor(np.ascontiguousarray(batches[0][:, 1:]).reshape(-1), dtype=np.int32, requires_grad=False, device="cuda")
        loss_fn = nn.CrossEntropyLoss(ignore_index=0)

        def fb():
            out, _ = model.forward(ids)
            loss = loss_fn(out.reshape(B * Tn, V), tgt)
            loss.backward()
            return loss

        fb()
        active = [p for p in model.parameters() if p.grad is not None]
        for p in model.parameters():
            p.grad = None
        opt = Adam(model.parameters(), lr=1.5e-4, betas=(0.9, 0.98), eps=1e-9)
        return model, ids, tgt, fb, opt, GradBucket(active)

    def feed(ids, tgt, b):
        ids.data.copy_(dev(np.ascontiguousarray(b[:, :-1])))
        tgt.data.copy_(dev(np.ascontiguousarray(b[:, 1:]).reshape(-1)))

    m1, ids1, tgt1, fb1, opt1, bk1 = make()
    losses1 = []
    for b in [batches[0]] + batches:                   # the graphed run warms up once on batch 0 first
        feed(ids1, tgt1, b)
        opt1.zero_grad()
        losses1.append(fb1().item())
        bk1.all_reduce()
        opt1.step()
    samples1 = [host(p.data.reshape(-1)[:8192]) for p in m1.parameters()]
    del m1, fb1, opt1, bk1
    torch.cuda.empty_cache()
    m2, ids2, tgt2, fb2, opt2, bk2 = make()
    feed(ids2, tgt2, batches[0])
    g = GraphedTrainStep(fb2, opt2, bk2, warmup=1)
    losses2 = []
    for b in batches:
        feed(ids2, tgt2, b)
        losses2.append(g().item())
    np.testing.assert_allclose(losses2, losses1[1:], rtol=1e-6, atol=1e-6)
    for s1, p2 in zip(samples1, m2.parameters()):
        np.testing.assert_allclose(host(p2.data.reshape(-1)[:8192]), s1, rtol=1e-6, atol=1e-7)
    g.release()


# =============================================================================================================
# LeakyReLU / Sigmoid / MaxPool2d / BatchNorm2d / MSELoss and the full config-5 classifier step
# =============================================================================================================
def test_vision_ops_golden(hip, golden):
    g = golden("vision_ops")
    import neunet_hip.nn as nn
    X = g["X"]
    for name, mod in [("leaky", nn.LeakyReLU(0.01)), ("sigmoid", nn.Sigmoid())]:
        x = T(hip, X)
        y = mod(x)
        np.testing.assert_allclose(host(y.data), g[f"{name}_Y"], rtol=1e-5, atol=1e-6)
        y.backward(g[f"{name}_dY"])
        np.testing.assert_allclose(host(x.grad), g[f"{name}_dX"], rtol=1e-5, atol=1e-6)
    for tag in ("pool22", "pool32p1", "pool21_overlap"):
        ks, st, pad = [int(v) for v in g[f"{tag}_cfg"]]
        x = T(hip, X)
        y = nn.MaxPool2d(ks, st, pad)(x)
        np.testing.assert_array_equal(host(y.data), g[f"{tag}_Y"])
        y.backward(g[f"{tag}_dY"])
        np.testing.assert_allclose(host(x.grad), g[f"{tag}_dX"], rtol=1e-6, atol=1e-6)
    bn = nn.BatchNorm2d(3)
    bn.weight.data.copy_(dev(g["bn_w"]))
    bn.bias.data.copy_(dev(g["bn_b"]))
    x = T(hip, X)
    y = bn(x)
    np.testing.assert_allclose(host(y.data), g["bn_Y"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(bn.running_mean.data), g["bn_rm"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(bn.running_var.data), g["bn_rv"], rtol=1e-5, atol=1e-6)
    y.backward(g["bn_dY"])
    np.testing.assert_allclose(host(x.grad), g["bn_dX"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(bn.weight.grad), g["bn_dw"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(host(bn.bias.grad), g["bn_db"], rtol=1e-5, atol=1e-5)
    bn.eval()
    np.testing.assert_allclose(host(bn(T(hip, X)).data), g["bn_Yeval"], rtol=1e-5, atol=1e-5)
    bn2 = nn.BatchNorm2d(3, affine=False)
    x = T(hip, X)
    y = bn2(x)
    np.testing.assert_allclose(host(y.data), g["bn_noaffine_Y"], rtol=1e-5, atol=1e-5)
    y.backward(g["bn_noaffine_dY"])
    np.testing.assert_allclose(host(x.grad), g["bn_noaffine_dX"], rtol=1e-4, atol=1e-5)
    p = T(hip, g["mse_P"])
    loss = nn.MSELoss()(p, T(hip, g["mse_T"], requires_grad=False))
    assert abs(loss.item() - float(g["mse_loss"])) < 1e-6
    loss.backward()
    np.testing.assert_allclose(host(p.grad), g["mse_dP"], rtol=1e-5, atol=1e-7)


def test_maxpool_dilated_golden(hip, golden):
    """MaxPool2d with dilation (the in-row gap of round 2): reference fixtures + an oracle case the reference's own backward
    cannot run (non-square dilated window, asymmetric padding)."""
    import neunet_hip.nn as nn
    g = golden("maxpool_dilated")
    X = g["X"]
    for tag in ("k2s1p0d2", "k3s2p2d2", "k2s2p1d3"):
        ks, st, pad, dil = [int(v) for v in g[f"{tag}_cfg"]]
        x = T(hip, X)
        y = nn.MaxPool2d(ks, st, pad, dil)(x)
        np.testing.assert_array_equal(host(y.data), g[f"{tag}_Y"])
        y.backward(g[f"{tag}_dY"])
        np.testing.assert_allclose(host(x.grad), g[f"{tag}_dX"], rtol=1e-6, atol=1e-6)
    rng = np.random.default_rng(3)
    X2 = rng.standard_normal((3, 2, 13, 10)).astype(np.float32)
    x = T(hip, X2)
    y = nn.MaxPool2d((3, 2), (2, 1), (2, 1), (2, 3))(x)
    yr, arg = O.maxpool2d_forward(X2, (3, 2), (2, 1), (2, 1), (2, 3))
    np.testing.assert_array_equal(host(y.data), yr)
    dY = rng.standard_normal(yr.shape).astype(np.float32)
    y.backward(dY)
    np.testing.assert_allclose(host(x.grad), O.maxpool2d_backward(X2.shape, arg, dY, (3, 2), (2, 1), (2, 1), (2, 3)),
                               rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError):
        nn.MaxPool2d(2, 2, 0, 0)


def _skip_if_switched_off(*names):
    """The fusion tests assert that the fused path RUNS: with its developer switch off in the environment there is nothing to test."""
    off = [n for n in names if os.environ.get(n) == "0"]
    if off:
        pytest.skip("switched off in the environment: " + ", ".join(off))


@pytest.mark.parametrize("xshape,cout,pool,leaky", [((16, 1, 28, 28), 8, (2, 2), True),      # C5 layer 1 (one column tile)
                                                    ((5, 3, 12, 18), 16, (2, 3), True),       # 28 columns, non-square windows
                                                    ((4, 7, 8, 8), 9, (2, 2), False),         # no activation in between, 64 columns
                                                    ((3, 2, 6, 6), 4, (3, 3), True),
                                                    ((2, 4, 5, 7), 6, (1, 1), True)])         # 1x1 "pool": every cell routed
def test_conv_pooled_weight_grad(hip, xshape, cout, pool, leaky):
    """Conv2d -> [LeakyReLU ->] MaxPool2d with a conv input that needs no gradient: the pool's backward hands dW, db to the conv
    straight from its own gradient (nnhipConv2dWeightGradPooled; the conv-output gradient is never written, the conv node's
    backward is skipped).  Bit-identical to the unfused chain (the same values meet the same MFMAs in the same order), equal to
    the oracle chain within the conv tolerance; with an input that DOES need a gradient the fused path must not run."""
    _skip_if_switched_off("NNHIP_VISION_FUSION", "NNHIP_CONV_POOLED_WGRAD", "NNHIP_CONV_WGRAD_MFMA")
    import neunet_hip
    import neunet_hip.nn as nn
    from neunet_hip.nn.experimental import HIPConv2d, vision
    rng = np.random.default_rng(sum(xshape) + cout)
    X = rng.uniform(-1, 1, xshape).astype(np.float32)
    conv = HIPConv2d(xshape[1], cout, 3, (1, 1), (1, 1))
    conv.bias.data.copy_(dev(rng.uniform(-0.3, 0.3, cout).astype(np.float32)))
    act, mp = nn.LeakyReLU(0.01), nn.MaxPool2d(pool, pool)
    Hq, Wq = xshape[2] // pool[0], xshape[3] // pool[1]
    dY = rng.standard_normal((xshape[0], cout, Hq, Wq)).astype(np.float32)
    res = {}
    for fused in (True, False):
        old, vision._FUSE = vision._FUSE, fused
        try:
            conv.weight.grad = conv.bias.grad = None
            x = neunet_hip.Tensor(X, device="cuda", requires_grad=False)
            c = conv(x)
            y = mp(act(c) if leaky else c)
            y.backward(dY)
            res[fused] = (host(conv.weight.grad), host(conv.bias.grad), host(y.data))
            assert (c.grad is None) == fused                  # fused: the conv-output gradient was never materialised
        finally:
            vision._FUSE = old
    for a, b in zip(res[True], res[False]):
        np.testing.assert_array_equal(a, b)
    W, b = host(conv.weight.data), host(conv.bias.data)
    Oc = O.conv2d_forward(X, W, b, (1, 1), (1, 1), (1, 1))
    A = O.leaky_relu_forward(Oc, 0.01) if leaky else Oc
    Yr, arg = O.maxpool2d_forward(A, pool, pool)
    np.testing.assert_allclose(res[True][2], Yr, **TOL)
    dA = O.maxpool2d_backward(A.shape, arg, dY, pool, pool)
    dOc = O.leaky_relu_backward(A, dA, 0.01) if leaky else dA
    _, dW, db = O.conv2d_backward(X, W, True, dOc, (1, 1), (1, 1), (1, 1))
    assert_close_scaled(res[True][0], dW)
    assert_close_scaled(res[True][1], db)
    # an input that needs its gradient: the ordinary path (the conv node runs its own backward)
    conv.weight.grad = conv.bias.grad = None
    x = T(hip, X)
    c = conv(x)
    (mp(act(c) if leaky else c)).backward(dY)
    assert c.grad is not None
    np.testing.assert_array_equal(host(conv.weight.grad), res[True][0])
    dX, _, _ = O.conv2d_backward(X, W, True, dOc, (1, 1), (1, 1), (1, 1))
    np.testing.assert_allclose(host(x.grad), dX, **TOL)


@pytest.mark.parametrize("xshape,cout,leaky,pad,need_dx", [((170, 1, 28, 28), 8, True, 1, False),      # C5 layer 1 (smaller batch)
                                                           ((64, 3, 46, 46), 16, True, 1, True),        # <16>, three input channels
                                                           ((40, 2, 62, 60), 5, False, 0, True),        # no activation, unpadded conv
                                                           ((150, 4, 32, 28), 7, True, 2, False),       # padding 2: patches past every edge
                                                           # few positions, >= 4 input channels: the quad kernel, sixteen lanes per window
                                                           ((16, 8, 14, 14), 16, True, 1, True),        # C5 layer 2
                                                           ((3, 5, 10, 14), 7, False, 1, True),         # <8>, channel counts off the fours, no activation
                                                           ((2, 16, 6, 6), 12, True, 2, False)])        # sixteen input channels, wide padding
def test_conv_leaky_pool_forward_fusion(hip, xshape, cout, leaky, pad, need_dx):
    """Conv2d -> [LeakyReLU ->] MaxPool2d(2, 2) with the conv launch deferred: one kernel computes the pooled output and the arg-max
    and never writes the conv output (nnhipConv2dLeakyMaxPoolForward).  Pooled values and gradients against the three-module
    chain and the oracle; the conv output materialises (identically) only if somebody reads it afterwards."""
    _skip_if_switched_off("NNHIP_VISION_FUSION", "NNHIP_LAZY_CONV", "NNHIP_CONV_POOL_FWD", "NNHIP_CONV_QUAD")
    import neunet_hip
    import neunet_hip.nn as nn
    from neunet_hip.nn.experimental import HIPConv2d, vision
    rng = np.random.default_rng(sum(xshape) + cout)
    X = rng.uniform(-1, 1, xshape).astype(np.float32)
    conv = HIPConv2d(xshape[1], cout, 3, (1, 1), (pad, pad))
    conv.bias.data.copy_(dev(rng.uniform(-0.3, 0.3, cout).astype(np.float32)))
    act, mp = nn.LeakyReLU(0.01), nn.MaxPool2d(2, 2)
    Ho, Wo = xshape[2] + 2 * pad - 2, xshape[3] + 2 * pad - 2
    dY = rng.standard_normal((xshape[0], cout, Ho // 2, Wo // 2)).astype(np.float32)
    res = {}
    for fused in (True, False):
        old, vision._FUSE = vision._FUSE, fused
        try:
            conv.weight.grad = conv.bias.grad = None
            x = neunet_hip.Tensor(X, device="cuda", requires_grad=need_dx)
            c = conv(x)
            y = mp(act(c) if leaky else c)
            assert c.pending() == fused                        # fused: the conv kernel never ran
            y.backward(dY)
            assert c.pending() == fused
            res[fused] = [host(y.data), host(conv.weight.grad), host(conv.bias.grad)] + ([host(x.grad)] if need_dx else []) + [host(c.data)]
        finally:
            vision._FUSE = old
    # the fused kernel and conv_direct_fwd_kernel run the same products in the same order, but the compiler contracts them into
    # fused multiply-adds differently: pooled values agree to an ulp or two, not bit for bit (so do the gradients routed by them)
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-6, atol=1e-6)
    for a, b in zip(res[True][1:-1], res[False][1:-1]):
        assert_close_scaled(a, b)
    np.testing.assert_array_equal(res[True][-1], res[False][-1])        # the conv output, once somebody asks for it: the same kernel
    W, b = host(conv.weight.data), host(conv.bias.data)
    Oc = O.conv2d_forward(X, W, b, (1, 1), (pad, pad), (1, 1))
    A = O.leaky_relu_forward(Oc, 0.01) if leaky else Oc
    Yr, arg = O.maxpool2d_forward(A, (2, 2), (2, 2))
    np.testing.assert_allclose(res[True][0], Yr, **TOL)
    dA = O.maxpool2d_backward(A.shape, arg, dY, (2, 2), (2, 2))
    dOc = O.leaky_relu_backward(A, dA, 0.01) if leaky else dA
    dX, dW, db = O.conv2d_backward(X, W, True, dOc, (1, 1), (pad, pad), (1, 1))
    assert_close_scaled(res[True][1], dW)
    assert_close_scaled(res[True][2], db)
    if need_dx:
        np.testing.assert_allclose(res[True][3], dX, rtol=1e-4, atol=2e-4)
    # ... but not after an optimizer step: the deferred launch would see updated weights (the deferred Linear's rule)
    from neunet_hip.optim import Adam
    x = neunet_hip.Tensor(X, device="cuda", requires_grad=False)
    c = conv(x)
    y = mp(act(c) if leaky else c)
    y.backward(dY)
    assert c.pending()
    Adam(conv.parameters(), lr=1e-3).step()
    with pytest.raises(RuntimeError, match="never materialised"):
        c.data


def test_conv_weight_grad_reduces_deferred(hip):
    """Inside Tensor.backward() the reduces of the small-channel convs' per-image partial weight gradients are queued and launched
    as one grid (conv_wgrad_reduce_group_kernel; partials in an arena of their own).  Five stacked 3x3 convs -- more than the
    queue holds, so it is flushed when full and again at the end -- plus a second backward that ACCUMULATES into the existing
    gradients (the flush must come before the add): bit-identical to the same steps with deferral switched off."""
    import neunet_hip
    from neunet_hip import _lib
    from neunet_hip.nn.experimental import HIPConv2d
    rng = np.random.default_rng(321)
    X = rng.uniform(-1, 1, (6, 1, 12, 10)).astype(np.float32)
    np.random.seed(99)
    chans = [1, 8, 16, 5, 12, 3]
    convs = [HIPConv2d(chans[i], chans[i + 1], 3, (1, 1), (1, 1)) for i in range(5)]
    dY = rng.standard_normal((6, 3, 12, 10)).astype(np.float32)
    res = {}
    for group in (8, 1):                                      # 1: wgrad_begin() declines, every reduce is launched where it is asked for
        old, _lib._wgrad["group"] = _lib._wgrad["group"], group
        try:
            for c in convs:
                c.weight.grad = c.bias.grad = None
            for _ in range(2):
                h = neunet_hip.Tensor(X, device="cuda", requires_grad=False)
                for c in convs:
                    h = c(h)
                h.backward(dY)
            res[group] = [host(c.weight.grad) for c in convs] + [host(c.bias.grad) for c in convs]
        finally:
            _lib._wgrad["group"] = old
    for a, b in zip(res[8], res[1]):
        np.testing.assert_array_equal(a, b)
    # and against the oracle chain (one backward = half of the accumulated gradient)
    acts, Ws = [X], [host(c.weight.data) for c in convs]
    for c, W in zip(convs, Ws):
        acts.append(O.conv2d_forward(acts[-1], W, host(c.bias.data), (1, 1), (1, 1), (1, 1)))
    d = dY
    for i in reversed(range(5)):
        dX, dW, db = O.conv2d_backward(acts[i], Ws[i], True, d, (1, 1), (1, 1), (1, 1))
        assert_close_scaled(res[8][i], 2 * dW)
        assert_close_scaled(res[8][5 + i], 2 * db)
        d = dX


@pytest.mark.parametrize("ks,st,pad,shape", [(2, 2, 0, (3, 4, 12, 12)), (3, 2, 1, (2, 3, 11, 9)), (2, 1, 0, (2, 2, 7, 7)),
                                              (2, 2, 0, (256, 8, 28, 28))])
def test_leaky_relu_maxpool_fusion(hip, ks, st, pad, shape):
    """MaxPool2d(LeakyReLU(x)): the deferred LeakyReLU is absorbed by the pool (nnhipMaxPool2dLeakyForward / Backward, one
    launch per direction) -- output, arg-max routing and the gradient of x must equal the two-module path exactly
    (bit-for-bit: the same activation values enter the same comparisons), also with overlapping windows, padding and when
    the activation output is ALSO read by someone else."""
    import neunet_hip.nn as nn
    from neunet_hip.nn.experimental import vision
    rng = np.random.default_rng(ks * 100 + st * 10 + pad)
    X = rng.standard_normal(shape).astype(np.float32)
    X.flat[:: 7] = 0.0                                        # zeros: the f <= 0 branch of the gradient
    Ho = (shape[2] + 2 * pad - ks) // st + 1
    Wo = (shape[3] + 2 * pad - ks) // st + 1
    dY = rng.standard_normal(shape[:2] + (Ho, Wo)).astype(np.float32)
    act, pool = nn.LeakyReLU(0.01), nn.MaxPool2d(ks, st, pad)
    res = {}
    for lazy in (True, False):
        old, vision._FUSE = vision._FUSE, lazy
        try:
            x = T(hip, X)
            h = act(x)
            assert h.pending() == lazy
            y = pool(h)
            assert h.pending() == lazy                        # absorbed, not materialised
            y.backward(dY)
            res[lazy] = (host(y.data), host(x.grad))
        finally:
            vision._FUSE = old
    np.testing.assert_array_equal(res[True][0], res[False][0])
    np.testing.assert_array_equal(res[True][1], res[False][1])
    ref = np.where(X <= 0, np.float32(0.01) * X, X)
    # the activation output read by someone else: AFTER the pool absorbed it (it materialises then, the pool's result and
    # backward are unaffected) and BEFORE (the pool then sees a plain tensor and takes the two-launch path)
    for read_first in (False, True):
        x = T(hip, X)
        h = act(x)
        if read_first:
            np.testing.assert_array_equal(host(h.data), ref)
        y = pool(h)
        if not read_first:
            np.testing.assert_array_equal(host(h.data), ref)
        assert not h.pending()
        y.backward(dY)
        np.testing.assert_array_equal(host(y.data), res[False][0])
        np.testing.assert_array_equal(host(x.grad), res[False][1])


def test_conv_classifier_golden(hip, golden):
    """Config-5 model (notebook cell 2) on the HIP path vs the REAL reference: step-1 outputs / loss / every gradient
    tight; step 2 (after one Adam update) to the +-lr noise level explained in test_oracle_golden.py."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import conv_classifier
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    g = golden("conv_classifier")
    model = conv_classifier.Conv2dClassifier()
    params = model.parameters()
    assert len(params) == int(g["n_params"])
    for i, p in enumerate(params):
        assert tuple(p.shape) == g[f"p{i}"].shape
        p.data.copy_(dev(g[f"p{i}"]))
    opt = Adam(params, lr=0.001)
    for s in range(2):
        opt.zero_grad()
        rm_before, rv_before = host(model.bnorm.running_mean.data).copy(), host(model.bnorm.running_var.data).copy()
        out = model(T(hip, g["X"][s]))
        loss = nn.MSELoss()(out, T(hip, g["T"][s], requires_grad=False))
        loss.backward()
        assert abs(loss.item() - g["losses"][s]) < (1e-6 if s == 0 else 2e-4)
        # step 2 against the reference's own trajectory: Adam's first update moves EVERY element by lr * sign(gradient), so an
        # element whose gradient is rounding noise lands lr = 1e-3 away from the reference's -- an Adam-trajectory floor of
        # lr * steps, not a kernel tolerance.  The kernels' step-2 arithmetic is held to the tight bound right below, against the
        # oracle evaluated at the SAME (HIP-updated) parameters.
        np.testing.assert_allclose(host(out.data), g["outs"][s], rtol=1e-4, atol=1e-5 if s == 0 else 1e-3)
        if s == 1:
            same = O.ConvClassifier([host(p.data) for p in params])
            same.rm, same.rv = rm_before.reshape(1, -1).copy(), rv_before.reshape(1, -1).copy()
            sl, so, sg = same.forward_backward(g["X"][s], g["T"][s])
            assert abs(loss.item() - float(sl)) < 1e-6
            np.testing.assert_allclose(host(out.data), so, rtol=1e-4, atol=1e-5)
            gs2 = grad_list_scale(sg)
            for i, p in enumerate(params):
                assert_close_scaled(host(p.grad), np.asarray(sg[i]).reshape(tuple(p.shape)), err_msg=f"step-2 grad {i}", scale=gs2)
        if s == 0:
            gscale = grad_list_scale([g[f"g{i}"] for i in range(len(params))])
            for i, p in enumerate(params):
                # conv biases in front of a BatchNorm have a mathematically zero gradient (the norm removes the mean)
                assert_close_scaled(host(p.grad), g[f"g{i}"], err_msg=f"grad {i}", scale=gscale)
        opt.step()
    # After Adam steps two correct fp32 implementations may differ by up to lr per step in any parameter whose gradient
    # is rounding noise (the update is lr * m / (sqrt(v) + eps): the noise's SIGN decides it) -- here lr = 1e-3, 2 steps;
    # the running mean is an average of activations of those parameters.
    np.testing.assert_allclose(host(model.bnorm.running_mean.data), g["rm"], rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("tail_one_launch", [False, True])
def test_conv_classifier_c5_batch_vs_oracle(hip, monkeypatch, tail_one_launch):
    """Batch 256 (BASELINE config 5) forward+backward against the oracle; also with the opt-in one-launch tail
    (NNHIP_BN_HEAD_FUSION=1: conv2's launch leaves partial batch statistics, BatchNorm + fc1 + Sigmoid + MSE are one kernel)."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import conv_classifier
    import neunet_hip.nn as nn
    import neunet_hip.nn.experimental.vision as V
    monkeypatch.setattr(V, "_FUSE_TAIL", tail_one_launch)
    rng = np.random.default_rng(1005)
    np.random.seed(1005)                       # the layers draw their initial weights from the global NumPy RNG
    model = conv_classifier.Conv2dClassifier()
    params = model.parameters()
    model.conv1.bias.data.copy_(dev(rng.uniform(-0.1, 0.1, 8).astype(np.float32)))
    ref = O.ConvClassifier([host(p.data) for p in params])
    X = rng.uniform(-1, 1, (256, 1, 28, 28)).astype(np.float32)
    Tt = np.eye(10, dtype=np.float32)[rng.integers(0, 10, 256)]
    out = model(T(hip, X))
    assert getattr(out, "pending", lambda: False)() == tail_one_launch
    loss = nn.MSELoss()(out, T(hip, Tt, requires_grad=False))
    loss.backward()
    rl, ro, rg = ref.forward_backward(X, Tt)
    assert abs(loss.item() - float(rl)) < 1e-5
    np.testing.assert_allclose(host(out.data), ro, rtol=1e-4, atol=1e-5)
    # The gradients are judged against a FLOAT64 pass of the same oracle (round-3 review: two fp32 sums compared loosely prove
    # little).  conv1.weight's gradient is 72 sums of 200 704 products: against float64 every entry must be within 1e-4 of
    # max(|its value|, the tensor's rms) -- the bound every other gradient tensor in this file holds.
    ref64 = O.ConvClassifier([host(p.data).astype(np.float64) for p in params])
    ref64.rm, ref64.rv = ref64.rm.astype(np.float64), ref64.rv.astype(np.float64)
    _, ro64, rg64 = ref64.forward_backward(X.astype(np.float64), Tt.astype(np.float64))
    np.testing.assert_allclose(host(out.data), ro64, rtol=1e-4, atol=1e-5)
    for i, p in enumerate(params):
        assert_close_scaled(host(p.grad), np.asarray(rg64[i]).reshape(tuple(p.shape)), tol=1e-4, err_msg=f"grad {i} vs float64")


@pytest.mark.parametrize("B,C,HW,N,affine,nstat", [(256, 16, 49, 10, True, 196), (37, 5, 12, 3, True, 4), (16, 3, 64, 16, False, 1024),
                                                   (2, 2, 2, 1, True, 1), (300, 16, 4, 7, True, 25)])
def test_batchnorm_linear_sigmoid_mse_entry(hip, B, C, HW, N, affine, nstat):
    """nnhipBatchNorm2dLinearSigmoidMSE (round 5): BatchNorm2d(training) -> flatten -> Linear -> Sigmoid -> MSELoss in one launch, the
    batch statistics combined from (mean, M2) pairs of `nstat` groups of values per channel.  Against the oracle's chain
    (batchnorm2d.py:84-100, linear.py:48-58, activations.py:19-28, losses.py:9-22) and against the library's own step-by-step entries."""
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr, load_hip_function
    rng = np.random.default_rng(90 + B)
    X = (rng.standard_normal((B, C, HW)) * 1.7 + 0.3 + 3.0 * rng.standard_normal((1, C, 1))).astype(np.float32)
    Tt = rng.uniform(0, 1, (B, N)).astype(np.float32)
    W = rng.uniform(-0.2, 0.2, (N, C * HW)).astype(np.float32)
    bl = rng.uniform(-0.2, 0.2, N).astype(np.float32)
    g = rng.uniform(0.5, 1.5, C).astype(np.float32) if affine else None
    be = rng.uniform(-0.5, 0.5, C).astype(np.float32) if affine else None
    assert load_hip_function("nnhipBatchNorm2dLinearSigmoidMSEFits")(B, C, HW, N) == 1
    count = B * HW // nstat
    assert nstat * count == B * HW
    groups = X.transpose(1, 0, 2).reshape(C, nstat, count).astype(np.float64)     # any partition of a channel's values will do
    gm = groups.mean(axis=2)
    stats = np.stack([gm, ((groups - gm[:, :, None]) ** 2).sum(axis=2)], axis=-1).transpose(1, 0, 2).astype(np.float32)   # [nstat][C][2]
    Xd, Y = dev(X), torch.empty(B, C, HW, device="cuda")
    sm, si = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    rm, rv = dev(np.full(C, 0.25, np.float32)), dev(np.full(C, 2.0, np.float32))
    pred, dz, loss = torch.empty(B, N, device="cuda"), torch.empty(B, N, device="cuda"), torch.empty((), device="cuda")
    for rep in range(2):                                     # twice: the ticket words are left clean
        call_hip_function("nnhipBatchNorm2dLinearSigmoidMSE", Xd, dev(stats), nstat, count, dev(g) if affine else None,
                          dev(be) if affine else None, Y, sm, si, rm if rep == 0 else None, rv if rep == 0 else None, B, C, HW, 1e-5, 0.1,
                          dev(W), dev(bl), N, dev(Tt), pred, dz, loss, get_current_stream_ptr())
    mean = X.astype(np.float64).mean(axis=(0, 2))
    var = X.astype(np.float64).var(axis=(0, 2))
    yo = (X - mean[None, :, None]) / np.sqrt(var[None, :, None] + 1e-5)
    if affine:
        yo = yo * g[None, :, None] + be[None, :, None]
    z = yo.reshape(B, -1) @ W.T.astype(np.float64) + bl
    po = 1.0 / (1.0 + np.exp(-z))
    np.testing.assert_allclose(host(sm), mean, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(si), 1.0 / np.sqrt(var + 1e-5), rtol=2e-5)
    np.testing.assert_allclose(host(rm), 0.1 * 0.25 + 0.9 * mean, rtol=1e-5, atol=1e-6)       # momentum * running + (1 - momentum) * stat
    np.testing.assert_allclose(host(rv), 0.1 * 2.0 + 0.9 * var, rtol=2e-5)
    np.testing.assert_allclose(host(Y), yo, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(host(pred), po, rtol=1e-4, atol=1e-5)
    assert abs(loss.item() - float(((po - Tt) ** 2).mean())) < 1e-5
    np.testing.assert_allclose(host(dz), 2 * (po - Tt) / (B * N) * po * (1 - po), rtol=1e-3, atol=1e-7)
    # the step-by-step entries on the same buffers
    Y2, sm2, si2 = torch.empty_like(Y), torch.empty_like(sm), torch.empty_like(si)
    call_hip_function("nnhipBatchNorm2dForward", Xd, dev(g) if affine else None, dev(be) if affine else None, Y2, sm2, si2, None, None, B, C,
                      HW, 1e-5, 0.1, 1, get_current_stream_ptr())
    np.testing.assert_allclose(host(Y), host(Y2), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(host(sm), host(sm2), rtol=1e-5, atol=1e-6)


def _conv_tail_model(nn, cin=8, cout=16, feat=7 * 7 * 16, n_out=10):
    class Tail(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.act, self.pool = nn.Conv2d(cin, cout, 3, 1, 1), nn.LeakyReLU(), nn.MaxPool2d(2, 2)
            self.bnorm, self.fc, self.sig = nn.BatchNorm2d(cout), nn.Linear(feat, n_out), nn.Sigmoid()

        def forward(self, x):
            self.y = self.bnorm(self.pool(self.act(self.conv(x))))
            return self.sig(self.fc(self.y.reshape(x.shape[0], -1)))

    return Tail()


def test_conv_classifier_tail_one_launch_vs_step_by_step(hip, monkeypatch):
    """conv2 -> LeakyReLU -> MaxPool -> BatchNorm2d -> flatten -> fc1 -> Sigmoid -> MSELoss (C5's second half): with the tail fusion the
    conv + pool launch leaves partial batch statistics and the rest is ONE launch; NNHIP_BN_HEAD_FUSION=0 launches module by module.
    Prediction, loss, the BatchNorm output / statistics and every gradient agree to rounding; the pending links are really pending."""
    import neunet_hip.nn as nn
    import neunet_hip.nn.experimental.vision as V
    from neunet_hip._lib import load_hip_function
    rng = np.random.default_rng(77)
    X = rng.uniform(-1, 1, (64, 8, 14, 14)).astype(np.float32)
    Tt = np.eye(10, dtype=np.float32)[rng.integers(0, 10, 64)]

    def run(fuse):
        monkeypatch.setattr(V, "_FUSE_TAIL", fuse)
        np.random.seed(12)
        m = _conv_tail_model(nn)
        m.bnorm.weight.data.copy_(dev(np.linspace(0.5, 1.5, 16, dtype=np.float32).reshape(1, 16)))
        x = T(hip, X)
        out = m(x)
        assert m.y.pending() == fuse and getattr(out, "pending", lambda: False)() == fuse
        loss = nn.MSELoss()(out, T(hip, Tt, requires_grad=False))
        assert not m.y.pending() and m.bnorm._pending_out is None
        loss.backward()
        res = {"y": host(m.y.data), "pred": host(out.data), "loss": np.float32(loss.item()), "dx": host(x.grad),
               "rm": host(m.bnorm.running_mean.data), "rv": host(m.bnorm.running_var.data)}
        for i, p_ in enumerate(m.parameters()):
            res[f"g{i}"] = host(p_.grad)
        return res

    a, r = run(True), run(False)
    for k in a:
        if k.startswith("g") or k == "dx":
            assert_close_scaled(a[k], r[k], err_msg=k, tol=2e-4)
        else:
            np.testing.assert_allclose(a[k], r[k], rtol=1e-4, atol=2e-5, err_msg=k)


def test_pending_batchnorm_is_unobservable(hip, monkeypatch):
    """A deferred BatchNorm2d launch must not be observable: a forward pass whose result is dropped still updates the running
    statistics before anyone can read them (batchnorm2d.py:84-100), a reader of the output in the middle of the chain gets the
    step-by-step launches, eval mode and inputs without producer statistics never defer."""
    import neunet_hip.nn as nn
    import neunet_hip.nn.experimental.vision as V
    monkeypatch.setattr(V, "_FUSE_TAIL", True)               # NNHIP_BN_HEAD_FUSION=1
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, (64, 8, 14, 14)).astype(np.float32)
    np.random.seed(3)
    m = _conv_tail_model(nn)
    bn = m.bnorm

    def pooled(x):
        return m.pool(m.act(m.conv(T(hip, x))))

    P = pooled(X)
    assert P._chan_stats is not None
    ref_mean = host(P.data).mean(axis=(0, 2, 3))
    out = bn(P)
    assert out.pending()
    del out                                                  # nobody ever reads it
    np.testing.assert_allclose(host(bn.running_mean.data).ravel(), 0.9 * ref_mean, rtol=1e-4, atol=1e-6)   # momentum 0.1: 0.1 * 0 + 0.9 * mean
    assert bn._pending_out is None
    sd = bn.state_dict()
    assert set(sd) == {"running_mean", "running_var", "weight", "bias"} and len(bn.parameters()) == 2
    # two forwards in a row: the first is launched before the second reads the running statistics
    o1 = bn(pooled(X))
    o2 = bn(pooled(2 * X))
    assert not o1.pending() and o2.pending()
    bn.eval()
    assert not o2.pending()
    assert not getattr(bn(pooled(X)), "pending", lambda: False)()
    bn.train()
    assert not getattr(bn(T(hip, host(P.data))), "pending", lambda: False)()        # no producer statistics: launched at once
    # a reader in the middle of the chain
    y = bn(pooled(X))
    flat = y.reshape(64, -1)
    z = m.fc(flat)
    zz = host(z.data)                                         # reads the Linear output: BatchNorm + GEMM launch now
    assert not y.pending() and not flat.pending()
    np.testing.assert_allclose(zz, O.linear_forward(host(y.data).reshape(64, -1), host(m.fc.weight.data), host(m.fc.bias.data)), rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):
        bn(pooled(X)).reshape(7, 11)


# =============================================================================================================
# Edge cases: empty inputs, > 2^31 elements (64-bit indexing), NULL-skipped outputs, error statuses on the GPU
# =============================================================================================================
def test_empty_inputs(hip):
    import neunet_hip.nn as nn
    lin = nn.Linear(8, 4)
    x = T(hip, np.zeros((0, 8), np.float32))
    y = lin(x)
    assert y.shape == (0, 4)
    y.backward(np.zeros((0, 4), np.float32))
    assert float(lin.weight.grad.abs().sum()) == 0.0 and tuple(lin.weight.grad.shape) == (4, 8)
    assert float(lin.bias.grad.abs().sum()) == 0.0
    for mod in (nn.Swish(), nn.ReLU(), nn.Softmax(axis=-1), nn.RMSNorm(8)):
        out = mod(T(hip, np.zeros((0, 8), np.float32)))
        assert out.shape == (0, 8)


def test_more_than_2_31_elements(hip):
    """64-bit indexing: elementwise over 2^31 + 4096 + 3 floats (the reference's `int size` would overflow)."""
    from neunet_hip.nn.experimental.activations import hip_swish_forward
    n = (1 << 31) + 4096 + 3
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    x.fill_(0.5)
    idx = torch.tensor([0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 4097, n - 1], device="cuda")
    vals = torch.tensor([-2.0, 3.0, 1.5, -0.25, 4.0, -1.0], device="cuda")
    x[idx] = vals
    y = torch.empty_like(x)
    hip_swish_forward(x, y, 1.0)
    got = host(y[idx])
    np.testing.assert_allclose(got, O.swish_forward(host(vals), 1.0), rtol=1e-6, atol=1e-7)
    mid = host(y[(1 << 31) - 8: (1 << 31) + 8])
    assert np.isfinite(mid).all()
    del x, y


def test_null_outputs_are_skipped(hip):
    """dX / dW / db may be NULL in nnhipLinearModuleBackward: only the requested gradients are produced."""
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    rng = np.random.default_rng(1)
    X, W, dO = [dev(rng.standard_normal(s).astype(np.float32)) for s in ((96, 40), (24, 40), (96, 24))]
    dW = torch.full((24, 40), 7.0, device="cuda")
    call_hip_function("nnhipLinearModuleBackward", X, W, dO, None, dW, None, 96, 40, 24, get_current_stream_ptr())
    np.testing.assert_allclose(host(dW), host(dO).T @ host(X), rtol=1e-4, atol=1e-4)


def test_error_status_not_exit(hip):
    from neunet_hip._lib import NeunetHipError, call_hip_function, get_current_stream_ptr
    a = torch.zeros(16, device="cuda")
    with pytest.raises(NeunetHipError, match="multiple of hidden"):
        call_hip_function("nnhipFusedSwishAndMul", a, a, 1.0, 3, 16, get_current_stream_ptr())
    with pytest.raises(NeunetHipError, match="negative size"):
        call_hip_function("nnhipRMSNormForward", a, a, None, a, a, None, -1, 16, 1e-6, get_current_stream_ptr())
    with pytest.raises(NeunetHipError, match="int16, int32 or int64"):
        call_hip_function("nnhipCrossEntropyLossEx", a, None, a, a, a, 3, None, 4, -100, 4, 4, b"n", None, None,
                          get_current_stream_ptr())
    # the library is still usable afterwards
    call_hip_function("nnhipScale", a, 2.0, 16, get_current_stream_ptr())


def test_device_error_word_is_a_sticky_status_not_a_trap(hip):
    """ABI 210 (round-5 review, hygiene): a kernel that finds the device state broken raises the library's device error word
    (pinned host memory) and ends normally -- no __builtin_trap(), the context survives.  The word is read without synchronising;
    nnhipDeviceError(), the optimizer step and the optimizer-in-backward entry answer NNHIP_EDEVICE (-5) until
    nnhipClearDeviceError().  The reference's convention for a failure inside its CUDA path is printf + exit(1)
    (linear_cublaslt_no_manual_mem.cu:91-94)."""
    import neunet_hip.nn as nn
    from neunet_hip._lib import NeunetHipError, call_hip_function, get_current_stream_ptr, load_hip_function
    from neunet_hip.optim import Adam
    assert load_hip_function("nnhipDeviceError")() == 0
    np.random.seed(1)
    lin = nn.Linear(64, 64)
    opt = Adam(lin.parameters(), lr=1e-3)
    x = T(hip, np.ones((128, 64), np.float32), requires_grad=False)
    lin(x).backward(np.ones((128, 64), np.float32))
    opt.step()                                               # fine
    before = [host(p.data).copy() for p in lin.parameters()]
    call_hip_function("nnhipRaiseDeviceErrorForTest", 1, get_current_stream_ptr())
    torch.cuda.synchronize()                                 # (only so that the test knows the store has landed)
    try:
        assert load_hip_function("nnhipDeviceError")() == -5
        with pytest.raises(NeunetHipError, match="device error 1"):
            call_hip_function("nnhipDeviceError")
        lin(x).backward(np.ones((128, 64), np.float32))
        with pytest.raises(NeunetHipError, match="status -5"):
            opt.step()
        for a, p_ in zip(before, lin.parameters()):          # the refused step touched nothing
            np.testing.assert_array_equal(a, host(p_.data))
    finally:
        load_hip_function("nnhipClearDeviceError")()
    assert load_hip_function("nnhipDeviceError")() == 0
    opt.zero_grad()
    lin(x).backward(np.ones((128, 64), np.float32))
    opt.step()                                               # the context is alive and the library usable
    assert np.isfinite(host(lin.parameters()[0].data)).all()


def test_dropout_mask_and_rng(hip):
    """Dropout: identity at p=0/eval; an injected mask reproduces dropout.py:17-37; the device RNG keeps ~(1-p)."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(2)
    X = rng.standard_normal((64, 256)).astype(np.float32)
    d0 = nn.Dropout(0.0)
    x = T(hip, X)
    assert d0(x) is x
    d = nn.Dropout(0.25)
    mask = (rng.random(X.shape) >= 0.25).astype(np.float32) / 0.75
    x = T(hip, X)
    y = d(x, mask=dev(mask))
    np.testing.assert_allclose(host(y.data), X * mask, rtol=1e-6, atol=1e-7)
    g = rng.standard_normal(X.shape).astype(np.float32)
    y.backward(g)
    np.testing.assert_allclose(host(x.grad), g * mask, rtol=1e-6, atol=1e-7)
    y2 = d(T(hip, np.ones_like(X)))
    kept = float((y2.data != 0).float().mean())
    assert abs(kept - 0.75) < 0.03
    assert abs(float(y2.data.max()) - 1 / 0.75) < 1e-6
    d.eval()
    x = T(hip, X)
    assert d(x) is x


# ------------------------------------------------------------------------------------------ Dropout (device hash RNG)
def test_dropout_hash_mask_statistics_and_backward(hip):
    """HIPDropout with p > 0 (neunet/nn/layers/dropout.py:17-37): the mask is a counter hash of (seed, index), never stored.
    Checked: every output is 0 or x/(1-p); the keep rate is 1-p within 4 sigma; the backward pass regenerates the SAME mask
    (dx == dy * y/x); two calls draw different masks; a device seed word changes the mask without a new launch argument;
    eval mode and p = 0 are the identity."""
    import neunet_hip.nn as nn
    rng = np.random.default_rng(12)
    n, p = 1 << 18, 0.1
    X = (rng.uniform(1.0, 2.0, (512, n // 512))).astype(np.float32)          # no zeros: y/x identifies the mask
    dY = rng.standard_normal(X.shape).astype(np.float32)
    drop = nn.Dropout(p)
    x = T(hip, X)
    y = drop(x)
    Y = host(y.data)
    m = Y / X
    keep = m != 0
    np.testing.assert_allclose(m[keep], 1.0 / (1.0 - p), rtol=1e-6)
    rate = keep.mean()
    assert abs(rate - (1 - p)) < 4 * np.sqrt(p * (1 - p) / n), rate
    y.backward(dY)
    np.testing.assert_allclose(host(x.grad), dY * m, rtol=1e-6, atol=0)
    m2 = host(drop(T(hip, X)).data) / X
    assert 0.15 < np.mean((m2 != 0) != keep) < 0.21                           # independent masks differ on 2 p (1-p) = 18 %
    # rows of the mask are not copies of each other (the index enters the hash, not the column alone)
    assert np.mean(keep[0] != keep[1]) > 0.1
    seed = torch.zeros(1, dtype=torch.int32, device="cuda")
    drop.seed_dev = seed
    drop._calls = 100
    a = host(drop(T(hip, X)).data)
    drop._calls = 100                                                          # same host seed ...
    seed.fill_(7)                                                              # ... different device word
    b = host(drop(T(hip, X)).data)
    assert 0.15 < np.mean((a != 0) != (b != 0)) < 0.21
    drop.eval()
    assert drop(x) is x
    assert nn.Dropout(0.0)(x) is x


def test_graphed_step_draws_fresh_dropout_masks(hip):
    """A captured training step with dropout: GraphedTrainStep(step_seed=attach_step_seed(model)) advances the device seed
    word before every replay, so two replays on the same input differ (a captured host seed alone would replay one mask)."""
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep, attach_step_seed
    from neunet_hip.optim import Adam

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.l1 = nn.Linear(32, 64)
            self.drop = nn.Dropout(0.5)
            self.l2 = nn.Linear(64, 8)

        def forward(self, x):
            self.h = self.drop(self.l1(x))
            return self.l2(self.h)

    np.random.seed(3)
    model = Net()
    seed = attach_step_seed(model)
    assert model.drop.seed_dev is seed
    opt = Adam(model.parameters(), lr=0.0)                                     # lr 0: the parameters stay put, only the mask changes
    xs = T(hip, np.random.default_rng(1).uniform(1, 2, (16, 32)).astype(np.float32), requires_grad=False)
    ys = T(hip, np.zeros(16, np.int32), dtype=np.int32, requires_grad=False)
    loss_fn = nn.CrossEntropyLoss()

    def fb():
        loss = loss_fn(model(xs), ys)
        loss.backward()
        return loss

    step = GraphedTrainStep(fb, opt, GradBucket(model.parameters()), warmup=1, step_seed=seed)
    step()
    h1 = host(model.h.data).copy()
    step()
    h2 = host(model.h.data).copy()
    step.release()
    assert 0.3 < np.mean((h1 != 0) != (h2 != 0)) < 0.7


# ------------------------------------------------------------------------------------------- deferred parameter gradients
def _wgrad_problem(rows, inf, outf, seed, bias=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.rand(rows, inf, device="cuda", generator=g) * 2 - 1
    W = (torch.rand(outf, inf, device="cuda", generator=g) * 2 - 1) / 16
    dO = torch.rand(rows, outf, device="cuda", generator=g) * 2 - 1
    dW, db = torch.empty(outf, inf, device="cuda"), (torch.empty(outf, device="cuda") if bias else None)
    return X, W, dO, dW, db


@pytest.mark.gpu
def test_deferred_weight_grads_grouped_launch(hip):
    """nnhipWeightGradDefer / Flush: the dW (+db) GEMMs of several Linear backward calls leave as ONE grid + ONE reduce.  Checked
    against float64 at the dot-product bound, against the undeferred calls, and for the contract's corners: a job's bits do not
    depend on its company (alone == in a group of four), small layers are not queued, dX is produced by the call itself."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    st = get_current_stream_ptr()
    shapes = [(4096, 512, 512), (4104, 260, 388), (8192, 256, 384), (5000, 2048, 516)]   # rows, in, out (two of them ragged: partial tiles, a partial last k-chunk)
    probs = [_wgrad_problem(*s, seed=i, bias=(i != 2)) for i, s in enumerate(shapes)]
    ref = []
    for (X, W, dO, dW, db), (r, i, o) in zip(probs, shapes):
        call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, r, i, o, st)
        ref.append((dW.clone(), None if db is None else db.clone()))
        dW.fill_(float("nan"))
        if db is not None:
            db.fill_(float("nan"))
    before = call("nnhipGemmLaunchCount", 0)
    call("nnhipWeightGradDefer", 1, st)
    try:
        dXs = []
        for (X, W, dO, dW, db), (r, i, o) in zip(probs, shapes):
            dX = torch.empty(r, i, device="cuda")
            call("nnhipLinearModuleBackward", X, W, dO, dX, dW, db, r, i, o, st)
            dXs.append(dX)
        assert call("nnhipWeightGradPending") == 4
        assert bool(torch.isnan(probs[0][3]).all()), "a queued dW was written before the flush"
        # a layer that is too small for the queue is served at once
        Xs, Ws, dOs, dWs, dbs = _wgrad_problem(64, 32, 16, seed=9)
        call("nnhipLinearModuleBackward", Xs, Ws, dOs, None, dWs, dbs, 64, 32, 16, st)
        assert call("nnhipWeightGradPending") == 4
        np.testing.assert_allclose(host(dWs), host(dOs).astype(np.float64).T @ host(Xs).astype(np.float64), rtol=1e-5, atol=1e-5)
        call("nnhipWeightGradFlush", st)
        assert call("nnhipWeightGradPending") == 0
    finally:
        call("nnhipWeightGradDefer", 0, st)
    assert call("nnhipGemmLaunchCount", 0) - before >= 4 + 4       # 4 dX GEMMs + 4 grouped jobs
    for (X, W, dO, dW, db), (rW, rb), dX, (r, i, o) in zip(probs, ref, dXs, shapes):
        assert_dot_close(host(dW), host(dO).T, host(X), err_msg=f"grouped dW {r}x{i}->{o}")
        assert_close_scaled(host(dW), host(rW), err_msg="grouped dW vs the undeferred call")
        assert_dot_close(host(dX), host(dO), host(W), err_msg="dX next to a queued dW")
        if db is not None:
            assert_within(host(db), host(dO).astype(np.float64).sum(0), 32 * U24 * np.abs(host(dO)).astype(np.float64).sum(0), "grouped db")
    # alone == in company
    X, W, dO, dW, db = probs[1]
    grouped = (dW.clone(), db.clone())
    dW.zero_(); db.zero_()
    call("nnhipWeightGradDefer", 1, st)
    try:
        call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, *shapes[1], st)
        assert call("nnhipWeightGradPending") == 1
    finally:
        call("nnhipWeightGradDefer", 0, st)       # switching off flushes
    assert call("nnhipWeightGradPending") == 0
    assert torch.equal(dW, grouped[0]) and torch.equal(db, grouped[1])


@pytest.mark.gpu
def test_deferred_weight_grads_grouped_slabs_across_streams(hip):
    """The slabs of the grouped launch are one block per process.  Two queued jobs leave with nnhipWeightGradFlushGemms on a side stream
    that is still busy with a few milliseconds of matrix products; two more are queued on the main stream at once and leave with
    nnhipWeightGradFlush, no synchronisation in between: the library orders the second launch behind the first one's reduce (it did
    not: the second launch's slabs overwrote the first's before they were summed).  All four dW / db: the bits of the same calls and
    flushes made on ONE stream.  Not the bits of the non-deferred call (no kernel changed here): the grouped launch cuts K = 4096 into four
    chunks of 1024 and the call's own GEMM splits it differently, so the two differ in the last bits (MI355X: dW by at most 7.5e-5
    at |dW| up to 88, db by at most 2.5e-5; printed below) -- the non-deferred call is held to assert_close_scaled here, as in
    test_deferred_weight_grads_grouped_launch, and a race shows against either."""
    from conv_child import FencedAt
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    st = get_current_stream_ptr()
    rows, inf, outf = 4096, 64, 64                                               # the smallest job the grouped launch takes: K = 4096, M = N = 64
    probs = [_wgrad_problem(rows, inf, outf, seed=40 + k) for k in range(4)]
    plain = []
    for X, W, dO, dW, db in probs:
        call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, rows, inf, outf, st)
        plain.append((dW.clone(), db.clone()))
    a = torch.ones(4096, 4096, device="cuda")
    side = torch.cuda.Stream()

    def run(first):
        """Jobs 0, 1 queued and launched by nnhipWeightGradFlushGemms on `first` behind a few milliseconds of matrix products there,
        jobs 2, 3 queued at once and launched by nnhipWeightGradFlush on the main stream."""
        outs = [(FencedAt((outf, inf)), FencedAt((outf,))) for _ in probs]
        torch.cuda.synchronize()

        def queue(k):
            X, W, dO, _, _ = probs[k]
            call("nnhipLinearModuleBackward", X, W, dO, None, outs[k][0].view, outs[k][1].view, rows, inf, outf, st)

        call("nnhipWeightGradDefer", 1, st)
        try:
            queue(0), queue(1)
            assert call("nnhipWeightGradPending") == 2
            with torch.cuda.stream(first):
                keep = [a @ a for _ in range(4)]
            call("nnhipWeightGradFlushGemms", first.cuda_stream)
            queue(2), queue(3)
            assert call("nnhipWeightGradPending") == 2
            call("nnhipWeightGradFlush", st)
        finally:
            call("nnhipWeightGradDefer", 0, st)
        torch.cuda.synchronize()
        del keep
        assert all(f.guards_intact() for o in outs for f in o)
        return outs

    ref, outs = run(torch.cuda.current_stream()), run(side)
    for k, ((fw, fb), (rW, rb), (pW, pb)) in enumerate(zip(outs, ref, plain)):
        print(f"\n[grouped slabs across streams, job {k}] one stream vs the non-deferred call: largest |dW difference| "
              f"{float((rW.view - pW).abs().max()):.3e} at largest |dW| {float(pW.abs().max()):.3e}, |db difference| {float((rb.view - pb).abs().max()):.3e}")
        assert torch.equal(fw.view, rW.view) and torch.equal(fb.view, rb.view), f"job {k}: differs from the same calls on one stream"
        assert_close_scaled(host(fw.view), host(pW), err_msg=f"job {k}: dW vs the non-deferred call")
        assert_close_scaled(host(fb.view), host(pb), err_msg=f"job {k}: db vs the non-deferred call")


@pytest.mark.gpu
def test_deferred_weight_grads_in_backward(hip, monkeypatch):
    """Tensor.backward() with the queue on (default, groups of four) == with it off, on a model whose layers qualify (4096 rows):
    every parameter gradient and the input gradient, within the gradient tolerance; torch's allocator is given every chance to
    recycle a queued job's dO (fresh temporaries between the layers), so a missing keep-alive shows up as garbage."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    from neunet_hip import _lib
    rng = np.random.default_rng(5)
    B, Tn, V = 16, 256, 1000
    ids = rng.integers(1, V, (B, Tn)).astype(np.int32)
    tgt = rng.integers(1, V, (B * Tn,)).astype(np.int32)
    init = None

    def run(group):
        nonlocal init
        monkeypatch.setitem(_lib._wgrad, "group", group)
        model = gpt_tiny.build_gpt(V, 256, 4, 1024, 2, pad_idx=0, max_len=Tn, fused=True)
        params = model.parameters()
        if init is None:
            init = [p.data.clone() for p in params]
        for p, v in zip(params, init):
            p.data.copy_(v)
        loss_fn = nn.CrossEntropyLoss(ignore_index=0)
        before = _lib.call_hip_function("nnhipGemmLaunchCount", 0)
        out, _ = model.forward(ids)
        loss = loss_fn(out.reshape(B * Tn, V), T(hip, tgt, dtype=np.int32, requires_grad=False))
        loss.backward()
        assert _lib.call_hip_function("nnhipWeightGradPending") == 0 and not _lib._wgrad["on"] and not _lib._wgrad["keep"]
        return [None if p.grad is None else host(p.grad) for p in params], loss.item(), \
            _lib.call_hip_function("nnhipGemmLaunchCount", 0) - before

    g_on, l_on, n_on = run(4)
    g_off, l_off, n_off = run(0)
    assert l_on == l_off and n_on == n_off
    # round 6, opt-in NNHIP_WGRAD_STREAM=1: the grouped launches on a side stream (fork at the flush, join at the end of backward();
    # measured SLOWER on the C4 step -- EXPERIMENTS.md -- and kept as a tested switch): same kernels, same bits
    monkeypatch.setattr(_lib, "_WGRAD_SIDE", True)
    g_side, l_side, n_side = run(4)
    monkeypatch.setattr(_lib, "_WGRAD_SIDE", False)
    assert l_side == l_on and n_side == n_on and not _lib._side["busy"] and not _lib._side["keep"]
    for a, b in zip(g_side, g_on):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, b)
    scale = grad_list_scale([a for a in g_off if a is not None])
    for k, (a, b) in enumerate(zip(g_on, g_off)):
        assert (a is None) == (b is None)
        if a is not None:
            assert_close_scaled(a, b, err_msg=f"parameter {k}", scale=scale)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,inf,outf,bias", [(4096, 512, 8320, True), (4096, 512, 15000, True), (8192, 384, 11000, False)])
def test_linear_dw_uneven_split(hip, rows, inf, outf, bias):
    """A dW GEMM whose tiles make ONE under-filled generation (256 < tiles <= 496; the GPT-tiny head has 472) is cut unevenly
    along the reduction: long blocks first, the short remainders through the idle slots, two slabs, one reduce.  dW and db against
    float64 at the dot-product bound -- including the ragged last tile row (15000 = 117 x 128 + 24)."""
    from neunet_hip._lib import call_hip_function as call, get_current_stream_ptr
    X, W, dO, dW, db = _wgrad_problem(rows, inf, outf, seed=rows + outf, bias=bias)
    dW.fill_(float("nan"))
    call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, rows, inf, outf, get_current_stream_ptr())
    assert_dot_close(host(dW), host(dO).T, host(X), err_msg="uneven-split dW")
    if bias:
        assert_within(host(db), host(dO).astype(np.float64).sum(0), 32 * U24 * np.abs(host(dO)).astype(np.float64).sum(0), "db")


@pytest.mark.gpu
def test_deferred_weight_grads_accumulate_across_backward_calls(hip, monkeypatch):
    """Two backward() calls without zero_grad(): the second call's parameter gradients are ADDED to the first's
    (neunet/autograd.py:85-93).  With the queue on, that addition must not read a gradient that is still a queued GEMM
    (`_finish_param` flushes first): same sums as with the queue off."""
    from neunet_hip import _lib
    from neunet_hip.nn.experimental import HIPLinear
    rng = np.random.default_rng(11)
    rows, inf, hid = 4096, 256, 384
    x1, x2 = (rng.standard_normal((rows, inf)) * 0.5).astype(np.float32), (rng.standard_normal((rows, inf)) * 0.5).astype(np.float32)
    g1, g2 = rng.standard_normal((rows, inf)).astype(np.float32), rng.standard_normal((rows, inf)).astype(np.float32)
    init = None

    def run(group):
        nonlocal init
        monkeypatch.setitem(_lib._wgrad, "group", group)
        l1, l2 = HIPLinear(inf, hid), HIPLinear(hid, inf)
        params = [l1.weight, l1.bias, l2.weight, l2.bias]
        if init is None:
            init = [p.data.clone() for p in params]
        for p, v in zip(params, init):
            p.data.copy_(v)
        for x, g in ((x1, g1), (x2, g2)):
            out = l2(l1(T(hip, x)))
            out.backward(g)
        return [host(p.grad) for p in params]

    on, off = run(4), run(0)
    for k, (a, b) in enumerate(zip(on, off)):
        assert_close_scaled(a, b, err_msg=f"accumulated gradient {k}")
    # and against float64 for the last layer's weight: dW2 = sum over both passes of dO^T h
    W1, b1 = host(init[0]).astype(np.float64), host(init[1]).astype(np.float64)
    ref = sum(g.astype(np.float64).T @ (x.astype(np.float64) @ W1.T + b1) for x, g in ((x1, g1), (x2, g2)))
    assert_close_scaled(on[2], ref, err_msg="accumulated dW2 vs float64")


# ------------------------------------------------------------------------------------------- argmax (own kernel, round 4)
@pytest.mark.parametrize("shape,axis", [((32, 10), 1), ((32, 10), 0), ((7, 5, 9), 1), ((7, 5, 9), -1), ((7, 5, 9), 0),
                                         ((3, 4100), 1), ((2, 70000), -1), ((300000,), None), ((64, 15000), 1),
                                         ((5, 1, 3), 1), ((6, 4, 5, 3), 2)])
def test_argmax_first_maximum_bit_exact(hip, shape, axis):
    """neunet.argmax = np.argmax -> int32 (neunet/__init__.py:132-139) on nnhipArgmaxF32: values drawn from a handful of
    levels so that EVERY slice has ties -- the first maximum must win, as in NumPy -- and compared bit for bit."""
    rng = np.random.default_rng(abs(hash((shape, axis))) % (2 ** 31))
    X = rng.integers(0, 4, shape).astype(np.float32)           # 4 levels: ties everywhere
    for keepdims in (False, True):
        got = hip.argmax(T(hip, X, requires_grad=False), axis=axis, keepdims=keepdims)
        ref = np.argmax(X, axis=axis, keepdims=keepdims).astype(np.int32)
        assert got.data.dtype == torch.int32
        np.testing.assert_array_equal(host(got.data).reshape(ref.shape), ref)
    Xc = rng.standard_normal(shape).astype(np.float32)         # continuous values: no ties
    np.testing.assert_array_equal(host(hip.argmax(T(hip, Xc, requires_grad=False), axis=axis).data),
                                  np.argmax(Xc, axis=axis).astype(np.int32))


def test_argmax_nan_and_negative_rows(hip):
    """NumPy's corner rules: a NaN is the maximum (the first NaN wins); an all -inf row returns 0; negative zero ties +0."""
    X = np.array([[1.0, np.nan, 3.0, np.nan], [-np.inf, -np.inf, -np.inf, -np.inf], [-0.0, 0.0, -1.0, 0.0],
                  [-5.0, -2.0, -2.0, -9.0]], np.float32)
    with np.errstate(invalid="ignore"):
        ref = np.argmax(X, axis=1).astype(np.int32)
    np.testing.assert_array_equal(host(hip.argmax(T(hip, X, requires_grad=False), axis=1).data), ref)
    np.testing.assert_array_equal(host(hip.argmax(T(hip, X, requires_grad=False), axis=0).data), np.argmax(X, axis=0).astype(np.int32))
    with pytest.raises(ValueError):
        hip.argmax(T(hip, np.zeros((3, 0), np.float32), requires_grad=False), axis=1)
