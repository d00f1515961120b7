"""The three one-launch step kernels restated: what nnhipLinearReLULinearBackward[Adam], nnhipLinearCrossEntropyLoss and
nnhipBatchNorm2dLinearSigmoidMSE compute, in float64; which kernel instance the host picks for a problem (csrc/gemm_small.hip:
gemm_small_mlp_fits and the grid of gemm_small_mlp_backward; csrc/rowops.hip: the launch of linear_ce_small_kernel and of
bn_linear_sigmoid_mse_kernel); the error bounds of tests/test_fused_step_gpu.py; and that module's case tables.
tests/test_fused_step_ref.py holds all of it to the oracle on the CPU.

Bounds (none new; dot_bound_of and epilogue_bound are tests/test_gemm_tiers_gpu.py's, U24 tests/test_hip_parity.py's):
  dW2, db2      dot_bound_of with c = 32: 32 2^-24 sum_b |dO||H| + 4 2^-24 |ref|
  dW1           32 2^-24 sum_b |dZ||X1| + sum_b dZerr_b |X1_b| + 4 2^-24 |ref| with dZerr = 32 2^-24 (|dO||W2|) (.) [H > 0], the dot bound on
                the float32 dZ the kernel forms in LDS (its mask is exact); db1 the same with X1 = 1
  logits        dot_bound_of(sum_k |X||W| + |b|)
  CE outputs    tests/test_rowops_tiers_gpu.py's: rtol = atol = 1e-5 for loss_rows, lse and loss, scaled_bound for dlogits
  BN head       save_mean, save_inv, the running statistics and Y: tests/test_hip_parity.py::test_batchnorm_linear_sigmoid_mse_entry's
                rtol 1e-5 (+ 1e-6) / 2e-5 and 1e-4 |Y| + 2e-5; pred: epilogue_bound's sigmoid expression on the dot bound of z plus
                sum_k Yerr |W|; dz = f(pred): |f'| predbound + |f''| predbound^2 / 2 + 8 2^-24 |dz| + 2^-126; loss 1e-5 absolute.

dZ follows the reference's expression, neunet/nn/activations.py:44-45 `grad * (f_x > 0)`: a PRODUCT.  A NaN in H is "not > 0" there as in
the kernel's comparison; an infinite or NaN (dO W2) entry under a closed mask is inf * 0 = NaN there."""
import numpy as np

from gemm_ref import ceil_div, small_wanted
from rowops_ref import cross_entropy
from test_hip_parity import U24

TINY = 2.0 ** -126


def _f64(a):
    return np.asarray(a, np.float64)


# ==================================================================================================== dispatch, restated
MLP_MAXROWS, MLP_MAXC, MLP_WAYS = 256, 16, 28
RESIDENT_BLOCKS_AT_LEAST = 256          # mlp_adam_grid_fits asks the occupancy API; one block per CU of an MI355X is a lower bound


def mlp_route(rows, in1, hid, out2, with_adam=False, resident=RESIDENT_BLOCKS_AT_LEAST):
    """(fits, NW, U, staging_tail_loop, n_checkin_blocks) of gemm_small_mlp_bwd_kernel<NW> / sg_tile16_dz<NW, U>.
    fits: gemm_small_mlp_fits -- with_adam adds the barrier rule, pollers (the dW2 tiles and the stepper) <= half of the blocks the chip
    holds, against `resident` (a lower bound of the occupancy query: True here implies 1 from the entry, not the other way round).
    staging_tail_loop: the `i >= PRE * BS` loops of the dO / dZ staging run (16 rows > 4 * 64 NW).  n_checkin_blocks: the blocks that add
    themselves to the arrival board of the Adam variant = the grid without the stepper."""
    fits = (0 < rows <= MLP_MAXROWS and 0 < out2 <= MLP_MAXC and in1 > 0 and hid > 0
            and small_wanted(out2, hid, rows, 1, out2, hid, False, False) and small_wanted(hid, in1, rows, 1, hid, in1, False, False)
            and rows * in1 * 4 < 1 << 31 and rows * hid * 4 < 1 << 31)
    groups = ceil_div(max(rows, 1), 16)
    nw = 8 if groups >= 8 else 4
    u = 1 if groups <= nw else 8
    pollers = ceil_div(hid, 16) * ceil_div(out2, 16) + 1
    if with_adam and pollers * 2 > resident:
        fits = False
    n = ceil_div(hid, 16) * ceil_div(out2, 16) + ceil_div(in1, 16) * ceil_div(hid, 16)
    return bool(fits), nw, u, rows * 16 > 4 * nw * 64, n


def board_wants(n):
    """`want` of everybody_here for the 28 words: blocks b with b % 28 == w."""
    return [n // MLP_WAYS + (1 if w < n % MLP_WAYS else 0) for w in range(MLP_WAYS)]


def lince_route(rows, K, classes, aligned=True):
    """(VEC, NW, one_group, nblk) of linear_ce_small_kernel<VEC, NW>: float4 loads need K % 4 == 0 and X, W on 16 bytes; NW is
    gemm_small()'s choice; one_group = every wave has at most one k-group of 16 (the U = 1 tile body)."""
    groups = ceil_div(K, 16)
    nw = 8 if groups >= 8 else 4
    return bool(K % 4 == 0 and aligned), nw, groups <= nw, ceil_div(rows, 16)


def lince_fits(rows, K, classes):
    return 1 <= rows <= 256 and 1 <= classes <= 32 and 1 <= K <= 2048


def bnhead_route(B, C, HW, N, nstat):
    """(fits, nblk, stat_rounds) of bn_linear_sigmoid_mse_kernel<8>: one block per 16 rows; the statistics loop takes 8 pairs per thread
    and round, 32 threads per channel."""
    fits = 1 <= B <= 4096 and 1 <= C <= 16 and HW >= 1 and 1 <= N <= 16 and (C * HW) % 4 == 0 and C * HW <= 2048
    return bool(fits), ceil_div(B, 16), ceil_div(nstat, 256)


def float4_channel_crossings(C, HW):
    """The largest number of channel boundaries inside one aligned float4 of a [C, HW] row (BnApplyA's carry)."""
    return max((k + 3) // HW - k // HW for k in range(0, C * HW, 4))


# ==================================================================================================== MLP backward
def _mm(a, b):
    """a @ b.  With a NaN or an infinity among the operands the product is formed term by term: a BLAS kernel may pad its panels
    with zeros, and inf * 0 then puts NaN into entries that hold none."""
    if np.isfinite(a).all() and np.isfinite(b).all():
        return a @ b
    return (a[:, :, None] * b[None, :, :]).sum(axis=1)


def mlp_backward64(X1, H, W2, dO):
    """dZ = (dO W2) (.) [H > 0] (the reference's product); dW2 = dO^T H, db2 = sum_b dO, dW1 = dZ^T X1, db1 = sum_b dZ."""
    X1, H, W2, dO = _f64(X1), _f64(H), _f64(W2), _f64(dO)
    with np.errstate(invalid="ignore", over="ignore"):
        dZ = _mm(dO, W2) * (H > 0)
        return dict(dW2=_mm(dO.T, H), db2=dO.sum(0), dW1=_mm(dZ.T, X1), db1=dZ.sum(0), dZ=dZ)


def mlp_bounds(X1, H, W2, dO, ref):
    from test_gemm_tiers_gpu import dot_bound_of
    X1, H, W2, dO = _f64(X1), _f64(H), _f64(W2), _f64(dO)
    with np.errstate(invalid="ignore", over="ignore"):
        aO, aX = np.abs(dO), np.abs(X1)
        dzerr = 32 * U24 * _mm(aO, np.abs(W2)) * (H > 0)
        adz = np.abs(ref["dZ"])
        return dict(dW2=dot_bound_of(_mm(aO.T, np.abs(H)), ref["dW2"]), db2=dot_bound_of(aO.sum(0), ref["db2"]),
                    dW1=32 * U24 * _mm(adz.T, aX) + _mm(dzerr.T, aX) + 4 * U24 * np.abs(ref["dW1"]),
                    db1=32 * U24 * adz.sum(0) + dzerr.sum(0) + 4 * U24 * np.abs(ref["db1"]))


def mlp_inputs(rows, in1, hid, out2, seed=0):
    """H = relu(random): about half zeros, with some exact -0 and +0 planted."""
    rng = np.random.default_rng(7000 + 131 * rows + 17 * in1 + 3 * hid + out2 + seed)
    X1 = rng.uniform(-1, 1, (rows, in1)).astype(np.float32)
    H = np.maximum(0, rng.standard_normal((rows, hid))).astype(np.float32)
    flat = H.reshape(-1)
    flat[::7] = -0.0
    flat[3::11] = 0.0
    W2 = (rng.standard_normal((out2, hid)) / np.sqrt(hid)).astype(np.float32)
    dO = rng.standard_normal((rows, out2)).astype(np.float32)
    return X1, H, W2, dO


MLP_ROWS = (1, 15, 16, 17, 63, 64, 65, 100, 112, 113, 128, 129, 255, 256)         # <4,1> | <4,8> | <8,1> | <8,8>
MLP_INSTANCE_ROWS = {(4, 1): (1, 15, 16, 17, 63, 64), (4, 8): (65, 100, 112), (8, 1): (113, 128), (8, 8): (129, 255, 256)}
G_EXACT, G_RAGGED = (16, 16, 16), (17, 17, 7)                                     # (in1, hid, out2)
MLP_EXTRA = {1: (1, 1, 1), 17: (15, 50, 1), 64: (90, 16, 15), 100: (90, 50, 15), 113: (90, 1, 15), 128: (15, 50, 1), 255: (90, 50, 15),
             256: (1, 1, 1)}
MLP_CASES = [(r,) + g for r in MLP_ROWS for g in (G_EXACT, G_RAGGED) + ((MLP_EXTRA[r],) if r in MLP_EXTRA else ())]   # (rows, in1, hid, out2)

# (rows, in1, hid, out2) on both sides of every limit of gemm_small_mlp_fits: rows, out2, tiles128 <= 8 and tiles32 <= 256 of the dW2
# GEMM (out2 x hid) and of the dW1 GEMM (hid x in1), and tiles32 <= 512 where rows <= 64
MLP_FITS_GRID = [(256, 16, 16, 16), (257, 16, 16, 16), (16, 16, 16, 16), (16, 16, 16, 17),
                 (65, 16, 1024, 16), (65, 16, 1025, 16), (64, 16, 1025, 16), (64, 16, 16384, 1), (64, 16, 16385, 1),
                 (65, 1024, 128, 4), (65, 1025, 128, 4), (64, 1025, 128, 4), (64, 4096, 128, 4), (64, 4097, 128, 4),
                 (65, 256, 512, 4), (65, 257, 512, 4)]

# ---- the Adam variant: (rows, in1, hid, out2) -> check-in blocks
MLP_ADAM_SHAPES = [(5, 16, 16, 1), (37, 120, 40, 7), (100, 90, 50, 10), (120, 440, 10, 16), (32, 200, 64, 10), (200, 280, 48, 3)]
MLP_ADAM_N = (2, 27, 28, 29, 56, 57)
MLP_ADAM_INSTANCE = ((4, 1), (4, 1), (4, 8), (8, 1), (4, 1), (8, 8))
MLP_ADAM_SEQUENCE = (5, 0, 2, 5)                     # indices into MLP_ADAM_SHAPES: n = 57, 2, 28, 57
# (decay_mode, wd, step (0 = device stepping), grad_scale, divisor)
ADAM_AXES = [(0, 0.0, 1, 1.0, None), (1, 0.0, 7, 1.0, None), (0, 1e-2, 7, 1.0, None), (1, 1e-2, 1, 1.0, None),
             (0, 1e-2, 0, 1.0, None), (1, 1e-2, 0, 1.0, None), (1, 1e-2, 1, 0.5, None), (0, 1e-2, 7, 0.5, 4.0), (1, 0.0, 0, 0.5, 4.0)]
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-3, (0.9, 0.999), 1e-8


def adam_state(rows, in1, hid, out2, seed=0):
    """p (W2 comes from mlp_inputs), m, v of b2, W1, b1 and W2: a state some steps into training."""
    rng = np.random.default_rng(8000 + rows + in1 + hid + out2 + seed)
    shapes = [(out2, hid), (out2,), (hid, in1), (hid,)]
    p = [rng.standard_normal(s).astype(np.float32) * 0.3 for s in shapes]
    m = [rng.standard_normal(s).astype(np.float32) * 0.1 for s in shapes]
    v = [(rng.standard_normal(s).astype(np.float32) * 0.1) ** 2 for s in shapes]
    return p, m, v


# ==================================================================================================== Linear + CrossEntropy
LINCE_K = (1, 15, 16, 63, 64, 65, 68, 112, 113, 116, 128, 129, 132, 2047, 2048)   # NW 4 one group | NW 4 | NW 8 one group | NW 8
LINCE_CLASSES = (1, 2, 15, 16, 17, 31, 32)
LINCE_ROWS = (1, 15, 16, 17, 32, 33, 255, 256)
# (rows, K, classes, offX, offW): every K with two class counts and two row counts; K = 64 and 132 with X, then W, 4 bytes off 16
LINCE_CASES = ([(LINCE_ROWS[i % 8], K, LINCE_CLASSES[i % 7], 0, 0) for i, K in enumerate(LINCE_K)] +
               [(LINCE_ROWS[(i + 3) % 8], K, LINCE_CLASSES[(i + 4) % 7], 0, 0) for i, K in enumerate(LINCE_K)] +
               [(33, 64, 17, 1, 0), (33, 64, 17, 0, 1), (17, 132, 31, 1, 0), (17, 132, 31, 0, 1)])
LINCE_SEQUENCE = (32, 16, 256, 32)                   # rows: nblk = 2, 1, 16, 2
# (reduction, weighted, ignore_index is the in-range one)
LINCE_RUNS = [("n", False, False), ("n", True, True), ("m", False, False), ("m", True, False), ("m", False, True), ("m", True, True),
              ("s", False, False), ("s", True, False), ("s", True, True)]


def lince_id(c):
    rows, K, classes, ox, ow = c
    vec, nw, one, nblk = lince_route(rows, K, classes, not (ox or ow))
    return f"{rows}x{K}x{classes}-{'vec' if vec else 'scalar'}-nw{nw}-{'one' if one else 'multi'}" + ("-offX" if ox else "") + ("-offW" if ow else "")


def lince_ignore(classes):
    """The in-range ignore_index of a case."""
    return classes // 2


def lince_inputs(rows, K, classes, seed=0):
    """X, W, b, class weights and labels: in range, the in-range ignore_index, -100, -1 and `classes` (the last two: out of range)."""
    rng = np.random.default_rng(9000 + 257 * rows + 33 * K + classes + seed)
    X = rng.standard_normal((rows, K)).astype(np.float32)
    W = (rng.standard_normal((classes, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(classes).astype(np.float32)
    cw = rng.uniform(0.5, 2.0, classes).astype(np.float32)
    y = rng.integers(0, classes, rows).astype(np.int64)
    y[1::5] = lince_ignore(classes)
    y[2::7] = -100
    y[3::9] = -1
    y[4::9] = classes
    return X, W, b, cw, y


def logits64(X, W, b):
    X, W = _f64(X), _f64(W)
    z = X @ W.T + _f64(b)[None, :]
    return z, np.abs(X) @ np.abs(W).T + np.abs(_f64(b))[None, :]


# ==================================================================================================== BatchNorm -> Linear -> Sigmoid -> MSE
# (B, C, HW, N, nstat, affine, running statistics, Linear bias)
BN_CASES = [(1, 16, 1, 1, 1, True, True, True), (16, 2, 2, 15, 32, False, False, True), (17, 4, 3, 16, 1, True, False, False),
            (32, 4, 5, 1, 32, True, True, True), (33, 2, 6, 16, 33, False, True, False), (300, 16, 49, 10, 1, True, True, True),
            (16, 16, 49, 15, 16, True, False, True), (31, 4, 127, 15, 31, True, True, True), (16, 4, 341, 16, 31, False, False, True),
            (257, 2, 2, 1, 257, True, True, False), (33, 4, 511, 7, 33, True, False, True), (32, 16, 128, 16, 256, True, True, True),
            (32, 16, 128, 15, 1024, False, True, False), (4096, 2, 2, 15, 1024, True, True, True), (17, 16, 1, 16, 1, True, True, True)]
BN_OFFSET_CASE = (64, 4, 12, 3, 16, True, True, True)          # channel 1: mean about 100, standard deviation about 0.01
BN_EPS, BN_MOMENTUM, BN_RM0, BN_RV0 = 1e-5, 0.1, 0.25, 2.0


def bn_id(c):
    B, C, HW, N, nstat = c[:5]
    return f"B{B}-C{C}xHW{HW}-N{N}-nstat{nstat}" + ("" if c[5] else "-plain") + ("" if c[6] else "-norun") + ("" if c[7] else "-nobias")


def bn_inputs(c, offset_channel=False):
    B, C, HW, N, nstat, affine, running, bias = c
    rng = np.random.default_rng(9500 + B + 7 * C + 13 * HW + N + nstat)
    X = (rng.standard_normal((B, C, HW)) * 1.7 + 0.3 + 3.0 * rng.standard_normal((1, C, 1))).astype(np.float32)
    if offset_channel:
        X[:, 1, :] = (100.0 + 0.01 * rng.standard_normal((B, HW))).astype(np.float32)
    d = dict(X=X, T=rng.uniform(0, 1, (B, N)).astype(np.float32), W=rng.uniform(-0.2, 0.2, (N, C * HW)).astype(np.float32),
             b=rng.uniform(-0.2, 0.2, N).astype(np.float32) if bias else None,
             g=rng.uniform(0.5, 1.5, C).astype(np.float32) if affine else None,
             be=rng.uniform(-0.5, 0.5, C).astype(np.float32) if affine else None)
    count = B * HW // nstat
    assert nstat * count == B * HW
    groups = X.transpose(1, 0, 2).reshape(C, nstat, count).astype(np.float64)          # any partition of a channel's values will do
    gm = groups.mean(axis=2)
    d["stats"] = np.stack([gm, ((groups - gm[:, :, None]) ** 2).sum(axis=2)], axis=-1).transpose(1, 0, 2).astype(np.float32)   # [nstat][C][2]
    d["count"] = count
    return d


def bnhead64(d, dtype=np.float64):
    """The chain with the batch statistics taken from X itself (two-pass), evaluated in `dtype`."""
    X, T, W = (np.asarray(d[k], dtype) for k in ("X", "T", "W"))
    B, N = T.shape
    mean = X.mean(axis=(0, 2), dtype=dtype)
    var = ((X - mean[None, :, None]) ** 2).mean(axis=(0, 2), dtype=dtype)
    inv = dtype(1) / np.sqrt(var + dtype(BN_EPS))
    Y = (X - mean[None, :, None]) * inv[None, :, None]
    if d["g"] is not None:
        Y = Y * np.asarray(d["g"], dtype)[None, :, None] + np.asarray(d["be"], dtype)[None, :, None]
    z = Y.reshape(B, -1) @ W.T
    if d["b"] is not None:
        z = z + np.asarray(d["b"], dtype)[None, :]
    pred = dtype(1) / (dtype(1) + np.exp(-z))
    dz = dtype(2) * (pred - T) / dtype(B * N) * pred * (dtype(1) - pred)
    mo = dtype(BN_MOMENTUM)
    return dict(mean=mean, var=var, inv=inv, Y=Y, z=z, pred=pred, dz=dz, loss=((pred - T) ** 2).mean(dtype=dtype),
                rm=mo * dtype(BN_RM0) + (dtype(1) - mo) * mean, rv=mo * dtype(BN_RV0) + (dtype(1) - mo) * var)


def bnhead_bounds(d, ref, y_bound=None):
    """Bounds on every output (header); y_bound replaces the old test's bound on Y (the offset-channel case)."""
    from test_gemm_tiers_gpu import epilogue_bound
    T, W = _f64(d["T"]), _f64(d["W"])
    B, N = T.shape
    Y, z, p = ref["Y"], ref["z"], ref["pred"]
    yb = 1e-4 * np.abs(Y) + 2e-5 if y_bound is None else np.broadcast_to(y_bound, Y.shape)
    mag = np.abs(Y).reshape(B, -1) @ np.abs(W).T + (0 if d["b"] is None else np.abs(_f64(d["b"]))[None, :])
    carried = yb.reshape(B, -1) @ np.abs(W).T
    pb, _ = epilogue_bound("act3", {}, None, None, mag + carried / (32 * U24), z)        # zb = dot_bound_of(mag, z) + carried
    k = 2.0 / (B * N)
    f1 = k * np.abs(p * (1 - p) + (p - T) * (1 - 2 * p))
    f2 = k * np.abs(2 * (1 - 2 * p) - 2 * (p - T))
    return dict(mean=1e-5 * np.abs(ref["mean"]) + 1e-6, inv=2e-5 * np.abs(ref["inv"]), rm=1e-5 * np.abs(ref["rm"]) + 1e-6,
                rv=2e-5 * np.abs(ref["rv"]), Y=yb, pred=pb, dz=f1 * pb + 0.5 * f2 * pb * pb + 8 * U24 * np.abs(ref["dz"]) + TINY, loss=1e-5)


def bn_offset_allowance():
    """The offset-channel case on the CPU: the float32 two-pass chain against float64.  Returns (largest |Y32 - Y64|, rms of Y64)."""
    d = bn_inputs(BN_OFFSET_CASE, offset_channel=True)
    r64, r32 = bnhead64(d), bnhead64(d, np.float32)
    return float(np.abs(_f64(r32["Y"]) - r64["Y"]).max()), float(np.sqrt((r64["Y"] ** 2).mean()))
