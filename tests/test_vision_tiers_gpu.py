"""GPU: every kernel and dispatch branch of csrc/pool_norm.hip -- BatchNorm2d (three forward tiers, two backward tiers), MaxPool2d (one
forward kernel, three backward kernels; plain and LeakyReLU-fused), MSELoss (one-block and two-launch; plain and sigmoid-folded) and the
float4 maps (LeakyReLU, Sigmoid) -- through the C ABI (include/neunet_hip.h), against the float64 restatements of tests/vision_ref.py,
at the shapes on either side of each dispatch condition.  tests/test_hip_parity.py keeps the reference's fixtures and the classifier.

Which BatchNorm2d shape reaches which kernels (bn_fits_fused() in pool_norm.hip: a 1024-thread block per channel holds 16 values per
thread, wave w the images w, w + 16, ..., its lanes the positions l, l + 64, ... -- rounds = ceil(B / 16), chunks = ceil(HW / 64),
fused when rounds * chunks <= 16, C < 131072 and B C HW <= 2^29; eval never takes the fused forward):

    shape               rounds x chunks   training forward / backward        why this shape
    (256, 2, 7, 7)      16 x 1            fused / fused                      exactly 16 x 1: the last shape that fits, batch-wise
    (16, 2, 32, 32)     1 x 16            fused / fused                      exactly 1 x 16: the last shape that fits, position-wise
    (17, 3, 16, 32)     2 x 8             fused / fused                      image 16 alone in the second round (15 waves idle there)
    (33, 2, 20, 15)     3 x 5             fused / fused                      HW = 300 leaves 20 lanes of the last chunk empty
    (5, 4, 7, 10)       1 x 2             fused / fused                      HW = 70: six lanes in the second chunk, 11 waves without an image
    (1, 3, 1, 1)        1 x 1             fused / fused                      N = 1: var = 0, inv = 1 / sqrt(eps), Y = bias, dX = 0
    (257, 2, 7, 7)      17 x 1            stats + apply / stats + apply      one image too many
    (16, 2, 25, 41)     1 x 17            stats + apply / stats + apply      HW = 1025: one position too many
    (40, 3, 64, 64)     3 x 64            stats + apply / stats + apply      192 additions per lane before the tree
    (4, 65, 5, 5)       1 x 1             (eval) two blocks of 64 channels in bn_eval_stats_kernel, one channel in the second
    (3, 1, 9, 9)        1 x 2             (eval) a single channel
    (256, 2, 7, 7)      16 x 1            (eval) fits the fused forward, which eval must not take (it would normalise by batch statistics);
                                          the backward after it takes the fused kernel all the same, with the running mean as its mean
    (16, 70000, 32, 32) 1 x 16            stats + apply since B C HW <= 2^29 is required (1.15e9 floats): see test_batchnorm_large_offsets

Every shape runs every mode (two training steps, training without running statistics, eval, three backwards), so each row above is also
an eval case and the eval rows are also training cases.

Bounds.  Y, dX, dW, db: the project's 1e-4 of max(|ref|, rms(ref)) per element (assert_close_scaled).  save_mean, save_inv, running
statistics, the MSE loss: the derived sum bounds of vision_ref (c from the element -> thread map, nothing tuned).  Pooling: arg-max and
pooled values exact, dX exact where at most one window reaches a pixel and to 1e-6 elsewhere.  Maps: LeakyReLU exact (one multiply);
Sigmoid within 8 x 2^-24 relative (expf 2 ulp = 4 x 2^-24, the addition, the division, one to spare) plus one float32 underflow.
Each test prints its largest error / bound ratios before it asserts (run with -s); one run's figures are in EXPERIMENTS.md 5.14, with
the wrong variants of each rule that the restatement was held against."""
import ctypes

import numpy as np
import pytest

from test_hip_parity import assert_close_scaled, assert_within, rms_of
from test_vision_ref import (EPS, LEAKY_ALPHAS, LEAKY_GEOMS, LEAKY_INPUTS, POOL_GEOMS, POOL_INPUTS, bits, created_ties,
                             expected_backward_kernel, leaky_pool_input, offset_input, pool_desc, pool_input)
from vision_ref import (FLT_MIN, U24, PoolDesc, batchnorm_backward, batchnorm_forward, bn_stat_bounds, leaky_backward, leaky_forward,
                        maxpool_backward, maxpool_forward, mse, mse_sum_c, running_bound, sigmoid_backward, sigmoid_forward, sum_bound)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MOM = float(np.float32(0.3))          # the float32 the C ABI receives
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def call(name, *args):
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    return call_hip_function(name, *args, get_current_stream_ptr())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda", dtype=torch.float32)


def ratio(got, ref, bound):
    """Largest |got - ref| / bound: what the docstring tables and EXPERIMENTS.md quote."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(np.max(err / np.maximum(np.broadcast_to(bound, err.shape), 1e-300))) if err.size else 0.0


def scaled_bound(ref, tol=1e-4, scale=0.0):
    ref = np.asarray(ref, np.float64)
    return tol * np.maximum(np.maximum(np.abs(ref), rms_of(ref)), scale) + 1e-30


# ===================================================================================================== BatchNorm2d
def bn_fits_fused(B, C, HW):
    """bn_fits_fused() of pool_norm.hip, restated."""
    return -(-B // 16) * -(-HW // 64) <= 16 and C < 131072 and B * C * HW <= 2 ** 29


BN_SHAPES = [
    ((256, 2, 7, 7), "fused"),          # 16 rounds x 1 chunk = 16: fits exactly
    ((16, 2, 32, 32), "fused"),         # 1 x 16 = 16: fits exactly
    ((17, 3, 16, 32), "fused"),         # 2 x 8: image 16 alone in the second round
    ((33, 2, 20, 15), "fused"),         # 3 x 5 = 15, HW = 300 = 4 * 64 + 44: 20 empty lanes in the fifth chunk
    ((5, 4, 7, 10), "fused"),           # 1 x 2, HW = 70: the second chunk holds six positions
    ((1, 3, 1, 1), "fused"),            # N = 1
    ((257, 2, 7, 7), "two-launch"),     # 17 x 1 = 17 > 16
    ((16, 2, 25, 41), "two-launch"),    # HW = 1025 -> 1 x 17 = 17 > 16
    ((40, 3, 64, 64), "two-launch"),    # 3 x 64 = 192
    ((4, 65, 5, 5), "fused"),           # eval: C = 65 -> bn_eval_stats_kernel runs two blocks, one live thread in the second
    ((3, 1, 9, 9), "fused"),            # eval: C = 1
]                                       # ((256, 2, 7, 7) in eval is the first row: every shape runs every mode)


def bn_forward(x, w, b, rm, rv, training):
    B, C, H, W = x.shape
    y, mean, inv = nans(B, C, H, W), nans(C), nans(C)
    call("nnhipBatchNorm2dForward", x, w, b, y, mean, inv, rm, rv, B, C, H * W, EPS, MOM, int(training))
    return y, mean, inv


def bn_backward(dy, x, w, mean, inv, want_dw):
    B, C, H, W = x.shape
    dx = nans(B, C, H, W)
    dw, db = (nans(C), nans(C)) if want_dw else (None, None)
    call("nnhipBatchNorm2dBackward", dy, x, w, mean, inv, dx, dw, db, B, C, H * W)
    return dx, dw, db


def check_bn_backward(tag, X, w, mean, inv, dY, got, shares):
    """dX, dW, db against the float64 backward at the given statistics.  N = 1: the first and third term of dX cancel exactly (dX is
    mathematically dstd 2 (x - mean)), so its entries are held to 1e-4 of the uncancelled term w dY inv (assert_close_scaled's scale)."""
    dx, dw, db = got
    B, C, H, W = X.shape
    dXr, dWr, dbr = batchnorm_backward(X, w, mean, inv, dY)
    scale = 0.0
    if B * H * W == 1:
        scale = rms_of((1.0 if w is None else np.asarray(w, np.float64).reshape(1, C, 1, 1)) * dY * inv.reshape(1, C, 1, 1))
    shares[tag + " dX"] = ratio(host(dx), dXr, scaled_bound(dXr, scale=scale))
    if dw is not None:
        shares[tag + " dW"] = ratio(host(dw), dWr, scaled_bound(dWr))
        shares[tag + " db"] = ratio(host(db), dbr, scaled_bound(dbr))
    print(f"\n[bn {X.shape} {tag}] error / bound: " + ", ".join(f"{k.split()[-1]} {v:.3f}" for k, v in shares.items() if k.startswith(tag)))
    assert_close_scaled(host(dx), dXr, err_msg=tag + " dX", scale=scale)
    if dw is not None:
        assert_close_scaled(host(dw), dWr, err_msg=tag + " dW")
        assert_close_scaled(host(db), dbr, err_msg=tag + " db")


def run_batchnorm(shape, affine, X1, X2, seed):
    """Two training steps (X1, then X2) from non-trivial running statistics, training without running statistics, eval on the
    statistics the two steps left, and the backward after the training and after the eval forward, with and without dW / db."""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, C).astype(np.float32) if affine else None
    b = rng.uniform(-0.5, 0.5, C).astype(np.float32) if affine else None
    rm0, rv0 = rng.uniform(-1, 1, C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    dY = rng.standard_normal(shape).astype(np.float32)
    wd, bd = (dev(w), dev(b)) if affine else (None, None)
    rm, rv = dev(rm0), dev(rv0)
    shares = {}

    # ---- two training steps
    ref_rm, ref_rv, d_rm, d_rv = rm0.astype(np.float64), rv0.astype(np.float64), 0.0, 0.0
    kept = None
    for step, X in enumerate((X1, X2)):
        x = dev(X)
        y, mean, inv = bn_forward(x, wd, bd, rm, rv, True)
        Yr, mr, ir, _, _ = batchnorm_forward(X, w, b, None, None, EPS, MOM, True)
        vr = X.astype(np.float64).var(axis=(0, 2, 3))                                       # biased, as the forward's
        dmean, dvar, dinv = bn_stat_bounds(X, EPS)
        d_rm = running_bound(MOM, ref_rm, mr, d_rm, dmean)
        d_rv = running_bound(MOM, ref_rv, vr, d_rv, dvar)
        ref_rm, ref_rv = MOM * ref_rm + (1.0 - MOM) * mr, MOM * ref_rv + (1.0 - MOM) * vr
        tag = f"step {step + 1}"
        shares.update({tag + " Y": ratio(host(y), Yr, scaled_bound(Yr)), tag + " mean": ratio(host(mean), mr, dmean),
                       tag + " inv": ratio(host(inv), ir, dinv), tag + " running_mean": ratio(host(rm), ref_rm, d_rm),
                       tag + " running_var": ratio(host(rv), ref_rv, d_rv)})
        print(f"\n[bn {shape} {tag}] error / bound: " + ", ".join(f"{k.split()[-1]} {v:.3f}" for k, v in shares.items() if k.startswith(tag)))
        assert_close_scaled(host(y), Yr, err_msg=tag + " Y")
        assert_within(host(mean), mr, dmean, tag + " save_mean")
        assert_within(host(inv), ir, dinv, tag + " save_inv")
        assert_within(host(rm), ref_rm, d_rm, tag + " running_mean")
        assert_within(host(rv), ref_rv, d_rv, tag + " running_var")
        if step == 0:
            kept = (x, y, mean, inv, mr, ir)

    # ---- training with running_mean = running_var = NULL: the same kernel, the same bits, nothing else written
    x1, y1, mean1, inv1, mr1, ir1 = kept
    y, mean, inv = bn_forward(x1, wd, bd, None, None, True)
    assert torch.equal(y, y1) and torch.equal(mean, mean1) and torch.equal(inv, inv1)

    # ---- backward after the training forward: at the kernel's own saved statistics, against float64 at float64 statistics
    dy = dev(dY)
    got = bn_backward(dy, x1, wd, mean1, inv1, True)
    check_bn_backward("training", X1.astype(np.float64), w, mr1, ir1, dY, got, shares)
    dx_only, none_w, none_b = bn_backward(dy, x1, wd, mean1, inv1, False)
    assert none_w is None and torch.equal(dx_only, got[0])                                  # dW = db = NULL changes nothing in dX

    # ---- eval on the running statistics the two steps left (read back: the reference starts from the same float32 values)
    rm_h, rv_h = host(rm).astype(np.float64), host(rv).astype(np.float64)
    rm_before, rv_before = rm.clone(), rv.clone()
    y, mean, inv = bn_forward(x1, wd, bd, rm, rv, False)
    Yr, mr, ir, _, _ = batchnorm_forward(X1, w, b, rm_h, rv_h, EPS, MOM, False)
    assert torch.equal(rm, rm_before) and torch.equal(rv, rv_before)                        # eval leaves them alone
    assert torch.equal(mean, rm)                                                            # save_mean is the running mean itself
    shares["eval inv"] = ratio(host(inv), ir, 3 * U24 * ir)
    shares["eval Y"] = ratio(host(y), Yr, scaled_bound(Yr))
    assert_within(host(inv), ir, 3 * U24 * ir, "eval save_inv")                             # + eps, sqrt, 1 / x: three roundings
    assert_close_scaled(host(y), Yr, err_msg="eval Y")
    got = bn_backward(dy, x1, wd, mean, inv, True)
    check_bn_backward("eval", X1.astype(np.float64), w, mr, ir, dY, got, shares)
    return shares


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("shape,tier", BN_SHAPES, ids=[f"{'x'.join(map(str, s))}" for s, _ in BN_SHAPES])
def test_batchnorm_tiers(hip, shape, tier, affine):
    B, C, H, W = shape
    assert ("fused" if bn_fits_fused(B, C, H * W) else "two-launch") == tier
    rng = np.random.default_rng(B * 1000 + C * 100 + H * W)
    X1 = (rng.standard_normal(shape) * 2 + rng.uniform(-3, 3, (1, C, 1, 1))).astype(np.float32)
    X2 = (rng.standard_normal(shape) * 0.5 + rng.uniform(-3, 3, (1, C, 1, 1))).astype(np.float32)
    run_batchnorm(shape, affine, X1, X2, seed=B + C + H * W)


@pytest.mark.parametrize("shape,tier", [((256, 2, 7, 7), "fused"), ((40, 3, 64, 64), "two-launch")], ids=["fused", "two-launch"])
def test_batchnorm_offset_input(hip, shape, tier):
    """The input on which a one-pass variance is off by more than 1e-3 and the float32 two-pass oracle by less than 2.5e-5
    (test_vision_ref.py::test_one_pass_variance_is_visibly_wrong_at_the_offset_input), through both training tiers: Y to 1e-4, the
    statistics within their sum bounds (which a one-pass variance misses by two orders: its error is >= half a float32 spacing of
    E[x^2] = 10^4, 5e-4, against a bound of 42 x 2^-24 var = 2.5e-6)."""
    B, C, H, W = shape
    assert ("fused" if bn_fits_fused(B, C, H * W) else "two-launch") == tier
    run_batchnorm(shape, False, offset_input(shape), offset_input(shape, seed=9), seed=3)


def test_batchnorm_large_offsets(hip):
    """(16, 70000, 32, 32): 1.15e9 floats, image 15 begins at element 1.075e9 > 2^30.  ceil(16 / 16) * ceil(1024 / 64) = 16 fits the fused
    kernels' registers, and until B C HW <= 2^29 joined bn_fits_fused() this shape took them: bn_ld() computed the byte offset of a buffer
    load as off * 4 in int, which wraps modulo 2^32 from element 2^30 on, so image 15 was read from a lower address inside X -- another
    image's values; silent, nothing faults.  X is noise plus a per-image constant (image b centred at b): a read from the wrong image
    moves the channel mean by 1 / 16 of the difference, hundreds of times the bound.  Now the shape takes the two-launch kernels
    (64-bit indices): statistics, and Y, dX of image 15, for the first, a middle and the last channel against float64 on the device;
    only those slices travel to the host.  About 18 GB of device memory for X, Y, dY, dX."""
    B, C, H, W = 16, 70000, 32, 32
    HW = H * W
    assert (B - 1) * C * HW > 2 ** 30 and -(-B // 16) * -(-HW // 64) <= 16 and not bn_fits_fused(B, C, HW)
    chans = [0, 34999, 69999]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(70000)
    x = torch.empty((B, C, H, W), device="cuda", dtype=torch.float32)
    x.normal_(generator=gen)
    x += torch.arange(B, device="cuda", dtype=torch.float32).view(B, 1, 1, 1)
    w = torch.empty(C, device="cuda").uniform_(0.5, 1.5, generator=gen)
    b = torch.empty(C, device="cuda").uniform_(-0.5, 0.5, generator=gen)
    y = torch.empty_like(x).fill_(NAN)
    mean, inv = nans(C), nans(C)
    call("nnhipBatchNorm2dForward", x, w, b, y, mean, inv, None, None, B, C, HW, EPS, MOM, 1)
    # float64 on the device, the three channels only
    xs = x[:, chans].double()                                                               # (16, 3, 32, 32)
    w64, b64 = w[chans].double().view(1, 3, 1, 1), b[chans].double().view(1, 3, 1, 1)
    m64 = xs.mean(dim=(0, 2, 3))
    xc = xs - m64.view(1, 3, 1, 1)
    v64 = (xc * xc).mean(dim=(0, 2, 3))
    i64 = 1.0 / torch.sqrt(v64 + EPS)
    Y15 = host((xc * i64.view(1, 3, 1, 1) * w64 + b64)[15])
    dmean, dvar, dinv = bn_stat_bounds(host(xs), EPS)
    got_mean, got_inv, got_Y15 = host(mean[chans]), host(inv[chans]), host(y[15, chans])
    print(f"\n[bn large] error / bound: mean {ratio(got_mean, host(m64), dmean):.3f}, inv {ratio(got_inv, host(i64), dinv):.3f}, "
          f"Y[15] {ratio(got_Y15, Y15, scaled_bound(Y15)):.3f}; mean - float64 = {got_mean - host(m64)}")
    assert_within(got_mean, host(m64), dmean, "save_mean")
    assert_within(got_inv, host(i64), dinv, "save_inv")
    assert_close_scaled(got_Y15, Y15, err_msg="Y[15]")
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(inv).all())             # every channel was written
    # ---- backward
    dy = torch.empty_like(x).normal_(generator=gen)
    dx = y.fill_(NAN)                                                                       # Y has been checked: its buffer takes dX
    dw, db = nans(C), nans(C)
    call("nnhipBatchNorm2dBackward", dy, x, w, mean, inv, dx, dw, db, B, C, HW)
    gs = dy[:, chans].double()
    N = B * HW
    dxh = w64 * gs
    iv = i64.view(1, 3, 1, 1)
    dstd = -0.5 * iv ** 3 * (dxh * xc).sum(dim=(0, 2, 3), keepdim=True)
    dX15 = host((dxh * iv + dstd * 2.0 * xc / N - (dxh * iv).sum(dim=(0, 2, 3), keepdim=True) / N)[15])
    dW = host((gs * (xc * iv)).sum(dim=(0, 2, 3)))
    dB = host(gs.sum(dim=(0, 2, 3)))
    got_dX15, got_dW, got_db = host(dx[15, chans]), host(dw[chans]), host(db[chans])
    print(f"[bn large] error / bound: dX[15] {ratio(got_dX15, dX15, scaled_bound(dX15)):.3f}, dW {ratio(got_dW, dW, scaled_bound(dW)):.3f}, "
          f"db {ratio(got_db, dB, scaled_bound(dB)):.3f}")
    assert_close_scaled(got_dX15, dX15, err_msg="dX[15]")
    assert_close_scaled(got_dW, dW, err_msg="dW")
    assert_close_scaled(got_db, dB, err_msg="db")
    del x, y, dx, dy, xs, gs, xc, dxh
    torch.cuda.empty_cache()


# ===================================================================================================== MaxPool2d
def c_desc(d):
    from neunet_hip._lib import Pool2dDesc
    return ctypes.byref(Pool2dDesc(**{k: getattr(d, k) for k in PoolDesc.FIELDS}))


def run_pool(name, X, alpha=None, seed=0):
    """Forward (arg-max and pooled values exact, bit for bit) and backward (exact where at most one window reaches a pixel, 1e-6 of the
    float64 accumulation elsewhere) of one geometry on one input; alpha: the LeakyReLU-fused entries, dX = the gradient of the
    activation's input."""
    shape, _, misaligned, kernel = POOL_GEOMS[name]
    d = pool_desc(name)
    cd = c_desc(d)
    B, C, H, W = shape
    Ho, Wo = d.out_hw()
    x = dev(X)
    y = nans(B, C, Ho, Wo)
    arg = torch.full((B, C, Ho, Wo), -7, device="cuda", dtype=torch.int32)
    if alpha is None:
        call("nnhipMaxPool2dForward", y, arg, x, cd)
    else:
        call("nnhipMaxPool2dLeakyForward", y, arg, x, alpha, cd)
    Yr, ar = maxpool_forward(X, d, pre_alpha=alpha)
    np.testing.assert_array_equal(host(arg), ar, err_msg=f"{name}: argmax")
    np.testing.assert_array_equal(bits(host(y)), bits(Yr), err_msg=f"{name}: pooled values (bit patterns)")

    dY = np.random.default_rng(seed + 1).standard_normal((B, C, Ho, Wo)).astype(np.float32)
    n = B * C * H * W
    buf = nans(n + 2)                                           # torch allocations are at least 256-byte aligned
    dx = buf[1:n + 1] if misaligned else buf[:n]
    assert dx.data_ptr() % 8 == (4 if misaligned else 0)
    assert expected_backward_kernel(d, dx.data_ptr() % 8 != 0) == kernel
    if alpha is None:
        call("nnhipMaxPool2dBackward", dx, dev(dY), arg, cd)
    else:
        call("nnhipMaxPool2dLeakyBackward", dx, dev(dY), arg, y, alpha, cd)
    got = host(dx).reshape(shape)
    guard = host(buf)
    assert np.isnan(guard[n + 1]) and np.isnan(guard[0 if misaligned else n]), f"{name}: wrote outside dX"
    dXr = maxpool_backward(shape, ar, dY, d, pooled=None if alpha is None else Yr, alpha=1.0 if alpha is None else alpha)
    reach = maxpool_backward(shape, ar, np.ones_like(dY), d)    # how many windows route their gradient to each pixel
    single = reach <= 1
    np.testing.assert_array_equal(got[single], dXr.astype(np.float32)[single], err_msg=f"{name}: dX where windows do not overlap")
    np.testing.assert_allclose(got, dXr, rtol=1e-6, atol=1e-6, err_msg=f"{name}: dX")
    return Yr, ar, got


@pytest.mark.parametrize("kind", POOL_INPUTS)
@pytest.mark.parametrize("name", list(POOL_GEOMS))
def test_maxpool_geometries(hip, name, kind):
    """The twelve geometries of test_vision_ref.POOL_GEOMS (each names the backward kernel it reaches and why) on continuous noise,
    on integers in [-2, 2] (a third to two thirds of the windows tie), on a constant with +0.0 / -0.0 sprinkled in (most windows tie;
    the pooled zero keeps the FIRST tap's sign) and on noise with -inf and NaN entries, where the kernel must skip NaN taps like the
    reference's nanmax / nanargmax (every window keeps one finite tap)."""
    shape = POOL_GEOMS[name][0]
    X = pool_input(kind, shape, 11, pool_desc(name))
    Yr, ar, dX = run_pool(name, X, seed=12)
    if kind == "inf_nan":
        assert np.isfinite(Yr).all() and np.isnan(X).any()
    if name == "gather_k2s3":                                   # rows 2, 5 and columns 2, 5, 8 are in no window: exactly 0
        assert not dX[:, :, 2::3, :].any() and not dX[:, :, :, 2::3].any()


@pytest.mark.parametrize("alpha", LEAKY_ALPHAS)
@pytest.mark.parametrize("kind", LEAKY_INPUTS)
@pytest.mark.parametrize("name", LEAKY_GEOMS)
def test_leaky_maxpool(hip, name, kind, alpha):
    """MaxPool2d(LeakyReLU(X; alpha)) in one launch each way, on every tile geometry and two gather geometries.  zeros: windows that pool
    to exactly +0.0 or -0.0 take the factor alpha in the backward (f <= 0).  collapse: adjacent negative floats whose float32 products
    with alpha coincide -- the test asserts that such windows exist -- tie, and the first tap takes the gradient."""
    shape = POOL_GEOMS[name][0]
    d = pool_desc(name)
    X = leaky_pool_input(kind, shape, 21)
    if kind == "collapse":
        assert created_ties(X, d, alpha) > 0
    Yr, ar, dX = run_pool(name, X, alpha=alpha, seed=22)
    if kind == "zeros":
        assert np.sum(Yr == 0) > 0


# ===================================================================================================== MSELoss
MSE_SIZES = [1,                  # one thread of mse_small_kernel has an element
             1023,               # one short of a full pass of the 1024 threads
             16384,              # the last size of mse_small_kernel: 16 per thread
             16385,              # the first size of mse_kernel + mse_final_kernel: 17 blocks
             100003,             # 98 blocks, a ragged last one
             2 ** 20 + 13]       # 1025 blocks' worth on a grid capped at 1024: the grid-stride loop wraps for the last 13


@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "nograd"])
@pytest.mark.parametrize("folded", [False, True], ids=["plain", "sigmoid"])
@pytest.mark.parametrize("n", MSE_SIZES)
def test_mse_sizes(hip, n, folded, want_grad):
    rng = np.random.default_rng(n + folded)
    if folded:                                                   # pred is a Sigmoid's output: (0, 1) and its two ends
        P = rng.uniform(0, 1, n).astype(np.float32)
        P[::7] = 0.0
        P[3::11] = 1.0
    else:
        P = rng.standard_normal(n).astype(np.float32)
    Tg = rng.uniform(0, 1, n).astype(np.float32)
    loss, g = nans(1), nans(n + 1) if want_grad else None
    call("nnhipMSELossSigmoidForwardBackward" if folded else "nnhipMSELossForwardBackward", dev(P), dev(Tg), loss,
         g[:n] if want_grad else None, n)
    ref_loss, ref_g = mse(P, Tg, sigmoid_folded=folded)
    assert mse_sum_c(n) <= 64
    bound = float(sum_bound((P.astype(np.float64) - Tg) ** 2, 64.0)) / n
    got = float(host(loss)[0])
    print(f"\n[mse n = {n}] |loss - float64| / bound = {abs(got - ref_loss) / bound:.3f} (c = 64; derived c = {mse_sum_c(n)})")
    assert abs(got - ref_loss) <= bound, (got, ref_loss, bound)
    if want_grad:
        gh = host(g)
        assert np.isnan(gh[n])                                   # nothing past the end
        np.testing.assert_allclose(gh[:n], ref_g, rtol=1e-6, atol=0)


# ===================================================================================================== maps
MAP_SIZES = [1, 3,               # scalar tail only (n >> 2 = 0)
             4,                  # one float4, no tail
             5,                  # one float4 + a tail of one
             1023,               # 255 float4 + 3: one block
             4099,               # five blocks, tail of 3
             65535 * 1024 + 5]   # pn_blocks() caps the grid at 65535 blocks of 256 threads x 4 floats: the grid-stride loop wraps


def map_refs(n, x, f, dy, alpha):
    """(leaky Y float32, sigmoid Y float64, leaky dX float32, sigmoid dX float64) -- the restatements on the host, or for the one size
    that is 268 MB per operand the same formulas in torch on the device."""
    if n <= 4099:
        xh, fh, dh = host(x), host(f), host(dy)
        return (leaky_forward(xh, alpha, np.float32), sigmoid_forward(xh), leaky_backward(fh, dh, alpha, np.float32), sigmoid_backward(fh, dh))
    a = torch.tensor(np.float32(alpha), device="cuda")
    x64, f64, d64 = x.double(), f.double(), dy.double()
    return (torch.where(x <= 0, a * x, x), 1.0 / (1.0 + torch.exp(-x64)), torch.where(f <= 0, dy * a, dy), d64 * f64 * (1.0 - f64))


def worst(got, ref, rel):
    """max of |got - ref| / (rel |ref| + FLT_MIN), on whichever side the operands live."""
    if isinstance(got, torch.Tensor):
        return float(((got.double() - ref).abs() / (rel * ref.abs() + FLT_MIN)).max())
    return float(np.max(np.abs(got.astype(np.float64) - ref) / (rel * np.abs(ref) + FLT_MIN)))


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", MAP_SIZES)
def test_map_sizes(hip, n, misaligned):
    """The four maps at sizes around the float4 body / scalar tail and past the grid cap, with 16-byte aligned operands (float4 path) and
    with every operand one float into its buffer (all-scalar path).  The float just outside each output must stay untouched."""
    alpha = 0.3
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n + misaligned)
    o = 1 if misaligned else 0
    view = lambda t: t[o:o + n]                                  # noqa: E731
    x = view(torch.empty(n + 1, device="cuda").normal_(0, 3, generator=gen))
    f = view(torch.empty(n + 1, device="cuda").uniform_(-1, 1, generator=gen))     # an activation OUTPUT: both signs for LeakyReLU
    fs = view(torch.empty(n + 1, device="cuda").uniform_(0, 1, generator=gen))     # a Sigmoid output
    dy = view(torch.empty(n + 1, device="cuda").normal_(0, 1, generator=gen))
    assert x.data_ptr() % 16 == (4 if misaligned else 0)
    outs = [nans(n + 1) for _ in range(4)]
    ly, sy, ldx, sdx = (view(t) for t in outs)
    call("nnhipLeakyReLUForward", ly, x, alpha, n)
    call("nnhipSigmoidForward", sy, x, n)
    call("nnhipLeakyReLUBackward", ldx, dy, f, alpha, n)
    call("nnhipSigmoidBackward", sdx, dy, fs, n)
    for t in outs:
        assert bool(torch.isnan(t[0 if misaligned else n])), "wrote outside the output"
    r_ly, r_sy, r_ldx, _ = map_refs(n, x, f, dy, alpha)
    r_sdx = map_refs(n, x, fs, dy, alpha)[3]
    big = isinstance(r_ly, torch.Tensor)
    got = (ly, sy, ldx, sdx) if big else tuple(host(t) for t in (ly, sy, ldx, sdx))
    eq = torch.equal if big else np.array_equal
    assert eq(got[0], r_ly), "LeakyReLU forward: one multiply, exact"
    assert eq(got[2], r_ldx), "LeakyReLU backward: one multiply, exact"
    ws, wb = worst(got[1], r_sy, 8 * U24), worst(got[3], r_sdx, 4 * U24)
    print(f"\n[maps n = {n}] sigmoid forward {ws:.3f} of 8 x 2^-24, backward {wb:.3f} of 4 x 2^-24")
    assert ws <= 1.0 and wb <= 1.0, (ws, wb)                     # backward: two multiplications and 1 - f, one to spare


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "offset1"])
def test_map_special_values(hip, misaligned):
    """Sigmoid at +-0, +-inf, NaN, +-88.8 (expf(88.8) overflows float32: 1 / (1 + inf) must be 0, not NaN) and +-104 (the float64 value
    is below the smallest float32 denormal): no NaN where float64 has none, NaN kept where it has one.  LeakyReLU at 0 and -0.0 (both
    take alpha x: bit patterns compared) and at the same specials.  13 values: three float4 and a tail of one, or all scalar."""
    X = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 88.8, -88.8, 104.0, -104.0, 1.0, -1.0, 17.0, -17.0], np.float32)
    n, o = X.size, 1 if misaligned else 0
    xb = nans(n + 1)
    x = xb[o:o + n]
    x.copy_(dev(X))
    sy, ly = nans(n + 1)[o:o + n], nans(n + 1)[o:o + n]
    call("nnhipSigmoidForward", sy, x, n)
    got, ref = host(sy), sigmoid_forward(X)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(ref).sum() == 1
    ok = ~np.isnan(ref)
    assert_within(got[ok], ref[ok], 8 * U24 * np.abs(ref[ok]) + FLT_MIN, "sigmoid")
    assert got[2] == 1.0 and got[3] == 0.0 and got[0] == 0.5 and got[1] == 0.5
    for alpha in LEAKY_ALPHAS:
        call("nnhipLeakyReLUForward", ly, x, alpha, n)
        np.testing.assert_array_equal(bits(host(ly))[ok], bits(leaky_forward(X, alpha, np.float32))[ok])
        assert np.isnan(host(ly)[4])
        # backward: an output of exactly 0 or -0.0 takes alpha (f <= 0)
        dy = dev(np.arange(1, n + 1, dtype=np.float32))
        ldx = nans(n + 1)[o:o + n]
        call("nnhipLeakyReLUBackward", ldx, dy, ly.clone(), alpha, n)
        np.testing.assert_array_equal(host(ldx), leaky_backward(host(ly), host(dy), alpha, np.float32))
        assert host(ldx)[0] == np.float32(alpha) * np.float32(1) and host(ldx)[1] == np.float32(alpha) * np.float32(2)
    # Sigmoid backward at the ends of its output range
    F = np.array([0.0, 1.0, 0.5, 2.0 ** -126, 1.0 - 2.0 ** -24], np.float32)
    dyh = np.array([3.0, -2.0, 1.0, 1.0, 5.0], np.float32)
    sdx = nans(6)[o:o + 5]
    fb = nans(6)[o:o + 5]
    fb.copy_(dev(F))
    db_ = nans(6)[o:o + 5]
    db_.copy_(dev(dyh))
    call("nnhipSigmoidBackward", sdx, db_, fb, 5)
    assert_within(host(sdx), sigmoid_backward(F, dyh), 4 * U24 * np.abs(sigmoid_backward(F, dyh)) + FLT_MIN, "sigmoid backward")
    assert host(sdx)[0] == 0.0 and host(sdx)[1] == 0.0
