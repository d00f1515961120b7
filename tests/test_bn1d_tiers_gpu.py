"""GPU: both tiers of csrc/batchnorm1d.hip and both sides of each dispatch condition, through the C ABI (nnhipBatchNorm1dForward /
nnhipBatchNorm1dBackward), against the float64 restatements of tests/bn1d_ref.py.

A 1024-thread block owns a strip of 16 features; the lanes of a wave are 4 row groups x 16 features, the block has 64 row slots.
bn1_fits_regs() (restated in bn1d_ref.py): N <= 64 * 16 = 1024 rows and N F <= 2^29 -> the register tier (the strip's column segment
stays in registers between the passes); else the looped tier (64-bit indices, X re-read per pass).  Eval always takes the looped forward
kernel without its reduction.

    shape          tier       why this shape
    (1, 3)         register   N = 1: var = 0, inv = 1 / sqrt(eps), Y = bias, dX = 0
    (2, 1)         register   a single feature: 15 of 16 lanes of every row group idle
    (7, 5)         register   odd sizes, one row per live thread
    (100, 2)       register   the notebooks' latent layer
    (100, 256)     register   the notebooks' hidden layers: 16 strips
    (100, 512)     register   32 strips
    (33, 16)       register   F = the strip width: one full strip
    (33, 15)       register   one lane of the strip past the last feature
    (33, 17)       register   a second strip with a single feature
    (1024, 3)      register   the last N of the register tier: 16 rows per thread
    (1025, 3)      looped     one row too many
    (5000, 3)      looped     deep in the looped tier, 79 additions per accumulator, 13 of 16 lanes idle
    (4, 1000)      register   63 strips, the last with 8 features; 60 of 64 row slots empty
    (9, 2^28 + 1)  looped     N F > 2^29 with N <= 1024, and row 8 starts past element 2^31: test_batchnorm1d_large_offsets

Every shape runs every mode (two training steps so that the running statistics carry over, training without running statistics, eval,
with and without the affine pair, the backward after the training and after the eval forward, with and without dW / db), on inputs with
a per-column offset.  Bounds: Y, dX, dW, db at the project's 1e-4 of max(|ref|, rms(ref)) (assert_close_scaled); save_mean, save_inv and
the running statistics at the derived sum bounds of bn1d_ref (c from the element -> thread map).  Each test prints its largest
error / bound ratios before it asserts (run with -s)."""
import numpy as np
import pytest

from bn1d_ref import (BN1_REG_ROWS, BN1_SW, batchnorm1d_backward, batchnorm1d_forward, bn1_fits_regs, bn1_stat_bounds)
from test_hip_parity import assert_close_scaled, assert_within, rms_of
from test_vision_ref import EPS, OFFSET
from vision_ref import U24, bn_stat_bounds, running_bound

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
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(np.max(err / np.maximum(np.broadcast_to(bound, err.shape), 1e-300))) if err.size else 0.0


def scaled_bound(ref, tol=1e-4, scale=0.0):
    ref = np.asarray(ref, np.float64)
    return tol * np.maximum(np.maximum(np.abs(ref), rms_of(ref)), scale) + 1e-30


assert BN1_SW == 16 and BN1_REG_ROWS == 1024
BN1_SHAPES = [
    ((1, 3), "register"), ((2, 1), "register"), ((7, 5), "register"),
    ((100, 2), "register"), ((100, 256), "register"), ((100, 512), "register"),
    ((33, BN1_SW), "register"), ((33, BN1_SW - 1), "register"), ((33, BN1_SW + 1), "register"),
    ((BN1_REG_ROWS, 3), "register"), ((BN1_REG_ROWS + 1, 3), "looped"),
    ((5000, 3), "looped"), ((4, 1000), "register"),
]


def bn1_forward(x, w, b, rm, rv, training):
    N, F = x.shape
    y, mean, inv = nans(N, F), nans(F), nans(F)
    call("nnhipBatchNorm1dForward", x, w, b, y, mean, inv, rm, rv, N, F, EPS, MOM, int(training))
    return y, mean, inv


def bn1_backward(dy, x, w, mean, inv, want_dw):
    N, F = x.shape
    dx = nans(N, F)
    dw, db = (nans(F), nans(F)) if want_dw else (None, None)
    call("nnhipBatchNorm1dBackward", dy, x, w, mean, inv, dx, dw, db, N, F)
    return dx, dw, db


def check_backward(tag, X, w, mean, inv, dY, got):
    """dX, dW, db against the float64 backward at the given statistics.  N = 1: dX is mathematically 0 (N g - sum g = 0, x - mean = 0).
    N = 2: the two normalised values are +-1 / sqrt(1 + eps / var), so dX_1 = w inv / 2 ((g_1 - g_2) - xhat^2 (g_1 - g_2)) =
    w inv (g_1 - g_2) / 2 * eps inv^2 -- the terms cancel to eps inv^2 ~ 1e-5 of their size, mathematically zero but for eps, and no
    float32 evaluation of the formula (the reference's own included) keeps four digits of what is left.  In both cases the entries
    are held to 1e-4 of the uncancelled term w dY inv: assert_close_scaled's `scale`, which exists for tensors whose terms cancel."""
    dx, dw, db = got
    N, F = X.shape
    dXr, dWr, dbr = batchnorm1d_backward(X, w, mean, inv, dY)
    scale = 0.0
    if N <= 2:
        scale = rms_of((1.0 if w is None else np.asarray(w, np.float64).reshape(1, F)) * dY * inv.reshape(1, F))
    shares = {"dX": ratio(host(dx), dXr, scaled_bound(dXr, scale=scale))}
    if dw is not None:
        shares["dW"] = ratio(host(dw), dWr, scaled_bound(dWr))
        shares["db"] = ratio(host(db), dbr, scaled_bound(dbr))
    print(f"[bn1d {X.shape} {tag}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert_close_scaled(host(dx), dXr, err_msg=tag + " dX", scale=scale)
    if dw is not None:
        assert_close_scaled(host(dw), dWr, err_msg=tag + " dW")
        assert_close_scaled(host(db), dbr, err_msg=tag + " db")


def run_batchnorm1d(shape, affine, X1, X2, seed):
    """Two training steps (X1, then X2) from non-trivial running statistics, training without running statistics, eval on the statistics
    the two steps left, and the backward after the training and after the eval forward, with and without dW / db."""
    N, F = shape
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, F).astype(np.float32) if affine else None
    b = rng.uniform(-0.5, 0.5, F).astype(np.float32) if affine else None
    rm0, rv0 = rng.uniform(-1, 1, F).astype(np.float32), rng.uniform(0.5, 2, F).astype(np.float32)
    dY = rng.standard_normal(shape).astype(np.float32)
    wd, bd = (dev(w), dev(b)) if affine else (None, None)
    rm, rv = dev(rm0), dev(rv0)

    ref_rm, ref_rv, d_rm, d_rv = rm0.astype(np.float64), rv0.astype(np.float64), 0.0, 0.0
    kept = None
    for step, X in enumerate((X1, X2)):
        x = dev(X)
        y, mean, inv = bn1_forward(x, wd, bd, rm, rv, True)
        Yr, mr, ir, _, _ = batchnorm1d_forward(X, w, b, None, None, EPS, MOM, True)
        vr = X.astype(np.float64).var(axis=0)
        dmean, dvar, dinv = bn1_stat_bounds(X, EPS)
        d_rm = running_bound(MOM, ref_rm, mr, d_rm, dmean)
        d_rv = running_bound(MOM, ref_rv, vr, d_rv, dvar)
        ref_rm, ref_rv = MOM * ref_rm + (1.0 - MOM) * mr, MOM * ref_rv + (1.0 - MOM) * vr
        tag = f"step {step + 1}"
        shares = {"Y": ratio(host(y), Yr, scaled_bound(Yr)), "mean": ratio(host(mean), mr, dmean), "inv": ratio(host(inv), ir, dinv),
                  "running_mean": ratio(host(rm), ref_rm, d_rm), "running_var": ratio(host(rv), ref_rv, d_rv)}
        print(f"\n[bn1d {shape} {tag}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
        assert_close_scaled(host(y), Yr, err_msg=tag + " Y")
        assert_within(host(mean), mr, dmean, tag + " save_mean")
        assert_within(host(inv), ir, dinv, tag + " save_inv")
        assert_within(host(rm), ref_rm, d_rm, tag + " running_mean")
        assert_within(host(rv), ref_rv, d_rv, tag + " running_var")
        if step == 0:
            kept = (x, y, mean, inv, mr, ir)
    if N == 1:                                                                               # var = 0, Y = bias exactly
        assert np.array_equal(host(kept[3]), np.full(F, np.float32(1.0) / np.sqrt(np.float32(EPS)), np.float32))
        assert np.array_equal(host(kept[1]), np.broadcast_to(b if affine else np.zeros(F, np.float32), (1, F)))

    # ---- training with running_mean = running_var = NULL: the same kernel, the same bits, nothing else written
    x1, y1, mean1, inv1, mr1, ir1 = kept
    y, mean, inv = bn1_forward(x1, wd, bd, None, None, True)
    assert torch.equal(y, y1) and torch.equal(mean, mean1) and torch.equal(inv, inv1)

    # ---- backward after the training forward: at the kernel's own saved statistics, against float64 at float64 statistics
    dy = dev(dY)
    got = bn1_backward(dy, x1, wd, mean1, inv1, True)
    check_backward("training", X1.astype(np.float64), w, mr1, ir1, dY, got)
    if N == 1:
        assert not host(got[0]).any()                                                        # dX = 0 exactly
    dx_only, none_w, _ = bn1_backward(dy, x1, wd, mean1, inv1, False)
    assert none_w is None and torch.equal(dx_only, got[0])                                  # dW = db = NULL changes nothing in dX
    again = bn1_backward(dy, x1, wd, mean1, inv1, True)                                      # a second run is bit-identical
    assert all(torch.equal(a, b_) for a, b_ in zip(again, got))

    # ---- eval on the running statistics the two steps left (read back: the reference starts from the same float32 values)
    rm_h, rv_h = host(rm).astype(np.float64), host(rv).astype(np.float64)
    rm_before, rv_before = rm.clone(), rv.clone()
    y, mean, inv = bn1_forward(x1, wd, bd, rm, rv, False)
    Yr, mr, ir, _, _ = batchnorm1d_forward(X1, w, b, rm_h, rv_h, EPS, MOM, False)
    assert torch.equal(rm, rm_before) and torch.equal(rv, rv_before)                        # eval leaves them alone
    assert torch.equal(mean, rm)                                                            # save_mean is the running mean itself
    print(f"[bn1d {shape} eval] error / bound: inv {ratio(host(inv), ir, 3 * U24 * ir):.3f}, Y {ratio(host(y), Yr, scaled_bound(Yr)):.3f}")
    assert_within(host(inv), ir, 3 * U24 * ir, "eval save_inv")                             # + eps, sqrt, 1 / x: three roundings
    assert_close_scaled(host(y), Yr, err_msg="eval Y")
    got = bn1_backward(dy, x1, wd, mean, inv, True)
    check_backward("eval", X1.astype(np.float64), w, mr, ir, dY, got)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("shape,tier", BN1_SHAPES, ids=[f"{n}x{f}" for (n, f), _ in BN1_SHAPES])
def test_batchnorm1d_tiers(hip, shape, tier, affine):
    N, F = shape
    assert ("register" if bn1_fits_regs(N, F) else "looped") == tier
    rng = np.random.default_rng(N * 1000 + F)
    X1 = (rng.standard_normal(shape) * 2 + rng.uniform(-3, 3, (1, F))).astype(np.float32)       # a per-column offset
    X2 = (rng.standard_normal(shape) * 0.5 + rng.uniform(-3, 3, (1, F))).astype(np.float32)
    run_batchnorm1d(shape, affine, X1, X2, seed=N + F)


@pytest.mark.parametrize("shape,tier", [((1024, 20), "register"), ((3000, 20), "looped")], ids=["register", "looped"])
def test_batchnorm1d_offset_input(hip, shape, tier):
    """Unit-spread noise around 100 (test_vision_ref.offset_input's construction, per column 100 + the column's own offset in [-3, 3]):
    E[x^2] - E[x]^2 in float32 loses the variance's third digit there, the two-pass variance keeps all of it -- a one-pass kernel misses
    the variance bound by two orders of magnitude.  Through both tiers."""
    N, F = shape
    assert ("register" if bn1_fits_regs(N, F) else "looped") == tier
    rng = np.random.default_rng(8)
    X1 = (OFFSET + rng.uniform(-3, 3, (1, F)) + rng.standard_normal(shape)).astype(np.float32)
    X2 = (OFFSET + rng.uniform(-3, 3, (1, F)) + rng.standard_normal(shape)).astype(np.float32)
    x64 = X1.astype(np.float64)
    one_pass = (X1 * X1).mean(axis=0, dtype=np.float32) - X1.mean(axis=0, dtype=np.float32) ** 2
    assert np.max(np.abs(one_pass - x64.var(axis=0)) / bn1_stat_bounds(X1, EPS)[1]) > 10      # the input does tell the two apart
    run_batchnorm1d(shape, False, X1, X2, seed=3)


@pytest.mark.parametrize("shape", [(100, 256), (1025, 3), (300, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batchnorm1d_agrees_with_batchnorm2d(hip, shape):
    """The only route the library had before: nnhipBatchNorm2dForward / Backward at (N, F, 1, 1).  Same operation, other sums: the two
    agree within the sum of the two kernels' derived bounds (statistics) and twice the scaled bound (Y, dX, dW, db)."""
    N, F = shape
    rng = np.random.default_rng(N + F)
    X = (rng.standard_normal(shape) + rng.uniform(-3, 3, (1, F))).astype(np.float32)
    dY = rng.standard_normal(shape).astype(np.float32)
    w, b = rng.uniform(0.5, 1.5, F).astype(np.float32), rng.uniform(-0.5, 0.5, F).astype(np.float32)
    x, dy, wd, bd = dev(X), dev(dY), dev(w), dev(b)
    y1, m1, i1 = bn1_forward(x, wd, bd, None, None, True)
    dx1, dw1, db1 = bn1_backward(dy, x, wd, m1, i1, True)
    y2, m2, i2, dx2, dw2, db2 = nans(N, F), nans(F), nans(F), nans(N, F), nans(F), nans(F)
    call("nnhipBatchNorm2dForward", x, wd, bd, y2, m2, i2, None, None, N, F, 1, EPS, MOM, 1)
    call("nnhipBatchNorm2dBackward", dy, x, wd, m2, i2, dx2, dw2, db2, N, F, 1)
    dm1, _, di1 = bn1_stat_bounds(X, EPS)
    dm2, _, di2 = bn_stat_bounds(X[:, :, None, None], EPS)
    Yr, mr, ir, _, _ = batchnorm1d_forward(X, w, b, None, None, EPS, MOM, True)
    dXr, dWr, dbr = batchnorm1d_backward(X, w, mr, ir, dY)
    print(f"\n[bn1d vs bn2d {shape}] difference / bound: mean {ratio(host(m1), host(m2), dm1 + dm2):.3f}, inv {ratio(host(i1), host(i2), di1 + di2):.3f}, "
          f"Y {ratio(host(y1), host(y2), 2 * scaled_bound(Yr)):.3f}, dX {ratio(host(dx1), host(dx2), 2 * scaled_bound(dXr)):.3f}, "
          f"dW {ratio(host(dw1), host(dw2), 2 * scaled_bound(dWr)):.3f}, db {ratio(host(db1), host(db2), 2 * scaled_bound(dbr)):.3f}")
    assert_within(host(m1), host(m2), dm1 + dm2, "save_mean")
    assert_within(host(i1), host(i2), di1 + di2, "save_inv")
    assert_within(host(y1), host(y2), 2 * scaled_bound(Yr), "Y")
    assert_within(host(dx1), host(dx2), 2 * scaled_bound(dXr), "dX")
    assert_within(host(dw1), host(dw2), 2 * scaled_bound(dWr), "dW")
    assert_within(host(db1), host(db2), 2 * scaled_bound(dbr), "db")


@pytest.mark.parametrize("shape", [(100, 256), (1500, 5)], ids=["register", "looped"])
def test_batchnorm1d_rerun_is_bit_identical(hip, shape):
    N, F = shape
    rng = np.random.default_rng(5)
    x, dy = dev(rng.standard_normal(shape) + 2), dev(rng.standard_normal(shape))
    w, b = dev(rng.uniform(0.5, 1.5, F)), dev(rng.uniform(-0.5, 0.5, F))
    runs = []
    for _ in range(2):
        rm, rv = dev(np.zeros(F)), dev(np.ones(F))
        y, mean, inv = bn1_forward(x, w, b, rm, rv, True)
        runs.append((y, mean, inv, rm, rv) + bn1_backward(dy, x, w, mean, inv, True))
    assert all(torch.equal(a, b_) for a, b_ in zip(*runs))


def test_batchnorm1d_graph_capture(hip):
    """Forward + backward captured in one hipGraph (no workspace, no allocation, no host synchronisation inside the C calls) and replayed
    twice: the running statistics equal those of two eager steps, bit for bit, and so do Y and dX."""
    N, F = 100, 256
    rng = np.random.default_rng(11)
    x, dy = dev(rng.standard_normal((N, F)) * 2 + 1), dev(rng.standard_normal((N, F)))
    w, b = dev(rng.uniform(0.5, 1.5, F)), dev(rng.uniform(-0.5, 0.5, F))
    rm0, rv0 = rng.uniform(-1, 1, F), rng.uniform(0.5, 2, F)

    def step(rm, rv, y, mean, inv, dx, dw, db):
        call("nnhipBatchNorm1dForward", x, w, b, y, mean, inv, rm, rv, N, F, EPS, MOM, 1)
        call("nnhipBatchNorm1dBackward", dy, x, w, mean, inv, dx, dw, db, N, F)

    eager = [dev(rm0), dev(rv0), nans(N, F), nans(F), nans(F), nans(N, F), nans(F), nans(F)]
    step(*eager)
    step(*eager)
    graph = [dev(rm0), dev(rv0), nans(N, F), nans(F), nans(F), nans(N, F), nans(F), nans(F)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        step(*graph)
    assert torch.equal(graph[0], dev(rm0))                    # capturing runs nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for name, a, b_ in zip(("running_mean", "running_var", "Y", "save_mean", "save_inv", "dX", "dW", "db"), eager, graph):
        assert torch.equal(a, b_), name
    assert not torch.equal(eager[0], dev(rm0))


def test_batchnorm1d_large_offsets(hip):
    """(9, 2^28 + 1): 2.4e9 floats.  N F > 2^29 sends a shape whose N fits the register tier to the looped tier -- the register tier's
    buffer loads take a 32-bit byte offset -- and row 8 begins at element 2^31 + 8, past what a 32-bit element index reaches.  X is noise
    plus the row number: a read from a wrapped address (another row) moves a column mean by a ninth of the difference, thousands of
    times the bound.  Statistics, Y, dX, dW, db of the first, a middle and the last feature against float64 on the device; only those
    columns travel to the host.  About 29 GB of device memory (X, dY, and one buffer for Y then dX)."""
    N, F = 9, 2 ** 28 + 1
    assert N <= BN1_REG_ROWS and not bn1_fits_regs(N, F) and (N - 1) * F > 2 ** 31
    cols = [0, 2 ** 27 + 3, F - 1]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    x = torch.empty((N, F), device="cuda", dtype=torch.float32)
    x.normal_(generator=gen)
    x += torch.arange(N, device="cuda", dtype=torch.float32).view(N, 1)
    w = torch.empty(F, device="cuda").uniform_(0.5, 1.5, generator=gen)
    b = torch.empty(F, device="cuda").uniform_(-0.5, 0.5, generator=gen)
    y = torch.empty_like(x).fill_(NAN)
    mean, inv = nans(F), nans(F)
    call("nnhipBatchNorm1dForward", x, w, b, y, mean, inv, None, None, N, F, EPS, MOM, 1)
    X = host(x[:, cols])
    wh, bh = host(w[cols]), host(b[cols])
    Yr, mr, ir, _, _ = batchnorm1d_forward(X, wh, bh, None, None, EPS, MOM, True)
    dmean, _, dinv = bn1_stat_bounds(X, EPS)
    got_y = host(y[:, cols])
    print(f"\n[bn1d large] error / bound: mean {ratio(host(mean[cols]), mr, dmean):.3f}, inv {ratio(host(inv[cols]), ir, dinv):.3f}, "
          f"Y {ratio(got_y, Yr, scaled_bound(Yr)):.3f}")
    assert_within(host(mean[cols]), mr, dmean, "save_mean")
    assert_within(host(inv[cols]), ir, dinv, "save_inv")
    assert_close_scaled(got_y, Yr, err_msg="Y")
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(inv).all())             # every feature was written
    assert bool(torch.isfinite(y[N - 1]).all())                                             # and all of the last row
    dy = torch.empty_like(x).normal_(generator=gen)
    dx = y.fill_(NAN)                                                                       # Y has been checked: its buffer takes dX
    dw, db = nans(F), nans(F)
    call("nnhipBatchNorm1dBackward", dy, x, w, mean, inv, dx, dw, db, N, F)
    dXr, dWr, dbr = batchnorm1d_backward(X, wh, mr, ir, host(dy[:, cols]))
    print(f"[bn1d large] error / bound: dX {ratio(host(dx[:, cols]), dXr, scaled_bound(dXr)):.3f}, "
          f"dW {ratio(host(dw[cols]), dWr, scaled_bound(dWr)):.3f}, db {ratio(host(db[cols]), dbr, scaled_bound(dbr)):.3f}")
    assert_close_scaled(host(dx[:, cols]), dXr, err_msg="dX")
    assert_close_scaled(host(dw[cols]), dWr, err_msg="dW")
    assert_close_scaled(host(db[cols]), dbr, err_msg="db")
    assert bool(torch.isfinite(dx[N - 1]).all())
    del x, y, dx, dy
    torch.cuda.empty_cache()
