"""Float64 restatements of the operations of csrc/pool_norm.hip -- LeakyReLU, Sigmoid, MaxPool2d (plain and LeakyReLU-fused),
BatchNorm2d, MSELoss -- written loop-level-obvious from the reference's layer sources (the lines oracle/neunet_oracle.py cites), NumPy
only, independent of the oracle and of the kernels.  tests/test_vision_ref.py holds them against the reference's fixtures and against
the oracle; tests/test_vision_tiers_gpu.py holds the kernels against them.

Also here: the rounding bounds of the kernels' sums.  A float32 sum of N terms whose additions are arranged as a chain of length L
per thread followed by a reduction tree of depth D differs from the exact sum by at most (L + D + k) * 2^-24 * sum|terms| to first
order (each term passes through at most L + D additions, each of relative error 2^-24, plus k roundings of its own arithmetic).  The
c = L + D + k of every kernel is derived from its element -> thread map in the helper that returns it; none is tuned to a run."""
import numpy as np

U24 = 2.0 ** -24
FLT_MIN = 2.0 ** -126          # smallest normal float32: what a result may lose to underflow


# ------------------------------------------------------------------------------------------- activations
def leaky_forward(x, alpha, dtype=np.float64):
    """f = x <= 0 ? alpha x : x (neunet/nn/activations.py:79-81).  alpha is the float32 the C ABI receives.  dtype = float32 is the
    kernel's own arithmetic: one multiply, correctly rounded, so the float32 restatement is exact, not approximate."""
    x = np.asarray(x)
    a = np.float32(alpha)
    if dtype == np.float32:
        with np.errstate(invalid="ignore"):
            return np.where(x <= 0, a * x.astype(np.float32), x.astype(np.float32)).astype(np.float32)
    x = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x <= 0, np.float64(a) * x, x)


def leaky_backward(f, dy, alpha, dtype=np.float64):
    """dx = dy * (f <= 0 ? alpha : 1), f the activation's OUTPUT (activations.py:64-68)."""
    f, dy = np.asarray(f), np.asarray(dy).astype(dtype)
    a = dtype(np.float32(alpha))
    with np.errstate(invalid="ignore"):
        return np.where(f <= 0, dy * a, dy)


def sigmoid_forward(x):
    """f = 1 / (1 + exp(-x)) (activations.py:24-25), float64: exp overflows to inf only beyond |x| = 709, and 1 / (1 + inf) = 0."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def sigmoid_backward(f, dy):
    """dx = dy * f * (1 - f), f the activation's OUTPUT (activations.py:12-13)."""
    f, dy = np.asarray(f, np.float64), np.asarray(dy, np.float64)
    return dy * f * (1.0 - f)


# ------------------------------------------------------------------------------------------- MaxPool2d
class PoolDesc:
    """The fields of struct nnhipPool2dDesc (include/neunet_hip.h).  dh / dw = 0 mean 1, as in the C ABI."""

    def __init__(self, B, C, H, W, kh, kw, sh=None, sw=None, pu=0, pd=0, pl=0, pr=0, dh=1, dw=1):
        self.B, self.C, self.H, self.W, self.kh, self.kw = B, C, H, W, kh, kw
        self.sh, self.sw = (kh if sh is None else sh), (kw if sw is None else sw)
        self.pu, self.pd, self.pl, self.pr, self.dh, self.dw = pu, pd, pl, pr, dh, dw

    FIELDS = ("B", "C", "H", "W", "kh", "kw", "sh", "sw", "pu", "pd", "pl", "pr", "dh", "dw")

    def out_hw(self):
        """maxpool2d.py:152-167."""
        dh, dw = max(self.dh, 1), max(self.dw, 1)
        return ((self.H + self.pu + self.pd - dh * (self.kh - 1) - 1) // self.sh + 1,
                (self.W + self.pl + self.pr - dw * (self.kw - 1) - 1) // self.sw + 1)

    def __repr__(self):
        return "PoolDesc(" + ", ".join(f"{k}={getattr(self, k)}" for k in self.FIELDS) + ")"


def maxpool_forward(X, desc, pre_alpha=None):
    """(Y float64, argmax int32) of MaxPool2d (maxpool2d.py:187-220): padding is -inf, the taps of output (ho, wo) sit at
    (ho sh - pu + r dh, wo sw - pl + s dw), the FIRST maximum in row-major (r, s) order wins and argmax = r kw + s.

    NaN taps are SKIPPED: the reference takes nanmax / nanargmax (:219, :48 -- it needs them because it marks the gaps of a dilated
    window with NaN).  oracle.maxpool2d_forward takes np.max / np.argmax over the taps alone and so PROPAGATES a NaN input; on NaN-free
    inputs the two agree.  That difference is why this restatement does not call the oracle.  A window without any tap above -inf
    (every tap padding, -inf or NaN) keeps -inf and argmax 0.

    pre_alpha: the window is taken over LeakyReLU(X; pre_alpha).  The activation is evaluated in FLOAT32 with one multiply, as the
    kernel does, and only then widened: distinct negative inputs whose products round to the same float32 tie, the first wins, and
    that tie belongs to the operation (a float64 product would order them and pick the other tap)."""
    X = np.asarray(X, np.float32)
    if pre_alpha is not None:
        X = leaky_forward(X, pre_alpha, np.float32)
    X = X.astype(np.float64)
    B, C, H, W = X.shape
    d = desc
    dh, dw = max(d.dh, 1), max(d.dw, 1)
    Ho, Wo = d.out_hw()
    Y = np.full((B, C, Ho, Wo), -np.inf)
    arg = np.zeros((B, C, Ho, Wo), np.int32)
    for ho in range(Ho):
        for wo in range(Wo):
            best = np.full((B, C), -np.inf)
            bi = np.zeros((B, C), np.int32)
            for r in range(d.kh):
                for s in range(d.kw):
                    y, x = ho * d.sh - d.pu + r * dh, wo * d.sw - d.pl + s * dw
                    if not (0 <= y < H and 0 <= x < W):
                        continue                                   # padding: -inf never beats anything
                    v = X[:, :, y, x]
                    with np.errstate(invalid="ignore"):
                        better = v > best                          # False for NaN: skipped; False for an equal value: first wins
                    best = np.where(better, v, best)
                    bi = np.where(better, r * d.kw + s, bi).astype(np.int32)
            Y[:, :, ho, wo], arg[:, :, ho, wo] = best, bi
    return Y, arg


def maxpool_backward(x_shape, argmax, dY, desc, pooled=None, alpha=1.0):
    """dX (float64) of MaxPool2d (maxpool2d.py:44-80): each window's gradient goes to its arg-max tap, overlapping windows accumulate,
    what lands in the padding is cropped.  pooled (the forward's output) given: dX is the gradient of the LeakyReLU's INPUT -- the
    routed gradient times alpha where pooled <= 0 (activations.py:64-68 applied to the one element that received the gradient)."""
    B, C, H, W = x_shape
    d = desc
    dh, dw = max(d.dh, 1), max(d.dw, 1)
    Ho, Wo = d.out_hw()
    g = np.asarray(dY, np.float64).reshape(B, C, Ho, Wo)
    if pooled is not None:
        g = np.where(np.asarray(pooled).reshape(B, C, Ho, Wo) <= 0, g * np.float64(np.float32(alpha)), g)
    argmax = np.asarray(argmax).reshape(B, C, Ho, Wo)
    dXp = np.zeros((B, C, H + d.pu + d.pd, W + d.pl + d.pr))
    for ho in range(Ho):
        for wo in range(Wo):
            a = argmax[:, :, ho, wo]
            for r in range(d.kh):
                for s in range(d.kw):
                    dXp[:, :, ho * d.sh + r * dh, wo * d.sw + s * dw] += np.where(a == r * d.kw + s, g[:, :, ho, wo], 0.0)
    return dXp[:, :, d.pu: d.pu + H, d.pl: d.pl + W]


# ------------------------------------------------------------------------------------------- BatchNorm2d
def batchnorm_forward(X, w, b, running_mean, running_var, eps, momentum, training):
    """BatchNorm2d (neunet/nn/layers/batchnorm2d.py:73-104) on X (B, C, H, W); w, b, running_* are (C,) or None.
    Training: mean and BIASED variance (np.var) over (B, H, W), two passes; running = momentum * running + (1 - momentum) * stat -- the
    reference's convention (:84-85; torch's is the other way round).  Eval: mean = running_mean, var = running_var.
    Returns (Y, mean, inv, new_running_mean, new_running_var) in float64; mean and inv = 1 / sqrt(var + eps) are what the backward
    reads (save_mean / save_inv of the C ABI); the running statistics come back unchanged in eval and as None where None was given."""
    X = np.asarray(X, np.float64)
    B, C, H, W = X.shape
    n = B * H * W
    rm = None if running_mean is None else np.asarray(running_mean, np.float64).reshape(C).copy()
    rv = None if running_var is None else np.asarray(running_var, np.float64).reshape(C).copy()
    mean, var = np.zeros(C), np.zeros(C)
    for c in range(C):
        if training:
            xc = X[:, c].reshape(-1)
            mean[c] = xc.sum() / n
            var[c] = ((xc - mean[c]) ** 2).sum() / n
            if rm is not None:
                rm[c] = momentum * rm[c] + (1.0 - momentum) * mean[c]
                rv[c] = momentum * rv[c] + (1.0 - momentum) * var[c]
        else:
            mean[c], var[c] = rm[c], rv[c]
    inv = 1.0 / np.sqrt(var + eps)
    Y = (X - mean[None, :, None, None]) * inv[None, :, None, None]
    if w is not None:
        Y = np.asarray(w, np.float64).reshape(1, C, 1, 1) * Y + np.asarray(b, np.float64).reshape(1, C, 1, 1)
    return Y, mean, inv, rm, rv


def batchnorm_backward(X, w, mean, inv, dY):
    """(dX, dW, db) of BatchNorm2d (batchnorm2d.py:15-50): the reference's ONE formula, whatever the mode -- it reads X - mean with
    the mean the forward used (in eval: the running mean) and treats that mean and 1 / std as the statistics of this batch.
        dxh = w dY;  dstd = -1/2 inv^3 sum(dxh (X - mean));  dX = dxh inv + dstd 2 (X - mean) / N - sum(dxh inv) / N
        dW = sum(dY (X - mean) inv);  db = sum(dY).      dW, db are returned whether or not w is given."""
    X, dY = np.asarray(X, np.float64), np.asarray(dY, np.float64)
    B, C, H, W = X.shape
    N = B * H * W
    dX, dW, db = np.zeros_like(X), np.zeros(C), np.zeros(C)
    for c in range(C):
        wc = 1.0 if w is None else float(np.asarray(w, np.float64).reshape(C)[c])
        xc = X[:, c] - mean[c]
        dxh = wc * dY[:, c]
        dstd = -0.5 * inv[c] ** 3 * np.sum(dxh * xc)
        dX[:, c] = dxh * inv[c] + dstd * 2.0 * xc / N - np.sum(dxh * inv[c]) / N
        dW[c] = np.sum(dY[:, c] * (xc * inv[c]))
        db[c] = np.sum(dY[:, c])
    return dX, dW, db


# ------------------------------------------------------------------------------------------- MSELoss
def mse(pred, target, sigmoid_folded=False):
    """(loss, gradient) of MSELoss (neunet/nn/losses.py:9-22): loss = sum((p - t)^2) / N, d loss / dp = 2 (p - t) / N.
    sigmoid_folded: pred is a Sigmoid's OUTPUT and the gradient is taken to the Sigmoid's input: times p (1 - p) (activations.py:12-13)."""
    p, t = np.asarray(pred, np.float64).reshape(-1), np.asarray(target, np.float64).reshape(-1)
    n = p.size
    d = p - t
    g = 2.0 * d / n
    if sigmoid_folded:
        g = g * p * (1.0 - p)
    return float(np.sum(d * d) / n), g


# ------------------------------------------------------------------------------------------- bounds
WAVE_TREE = 6      # wave_sum (csrc/common.h): four cross-lane additions, then (a + b) + (c + d) over the four rows of 16 lanes


def bn_sum_c(B, HW):
    """c of the per-channel sums of the BatchNorm2d kernels (bn_stats_kernel, bn_bwd_stats_kernel and the fused pair: one element ->
    thread map).  A 1024-thread block per channel; wave w takes images w, w + 16, ..., lane l the positions l, l + 64, ... of each:
        chain   ceil(B / 16) * ceil(HW / 64) additions in one thread's accumulator,
        tree    6 in wave_sum + 16 for the serial sum over the sixteen waves' partials (block_sum<16>),
        k = 4   the term's own arithmetic: at most a subtraction and three multiplications (w * g * xc, g * (xc * inv), d * d)."""
    return -(-B // 16) * -(-HW // 64) + WAVE_TREE + 16 + 4


def bn_stat_bounds(X, eps):
    """Bounds of save_mean, the batch variance and save_inv against float64, per channel, from bn_sum_c:
        mean   c u sum|x| / n  (+ u |mean| for the division),
        var    c u sum (x - mean)^2 / n  +  dmean^2  (the deviations are taken from the ROUNDED mean: sum (x - m - dm)^2 / n = var + dm^2)
               + 2 u var (division, and the rounding of x - mean doubles in the square -- already counted in k, kept for safety),
        inv    inv * (dvar / (2 (var + eps)) + 3 u): d(v^-1/2) = -1/2 v^-3/2 dv, and the addition of eps, the square root and the division round."""
    X = np.asarray(X, np.float64)
    B, C, H, W = X.shape
    n = B * H * W
    c = bn_sum_c(B, H * W)
    mean = X.mean(axis=(0, 2, 3))
    var = ((X - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
    dmean = c * U24 * np.abs(X).sum(axis=(0, 2, 3)) / n + U24 * np.abs(mean)
    dvar = c * U24 * var + dmean ** 2 + 2 * U24 * var
    inv = 1.0 / np.sqrt(var + eps)
    dinv = inv * (dvar / (2.0 * (var + eps)) + 3 * U24)
    return dmean, dvar, dinv


def running_bound(momentum, run_prev, stat, d_prev, d_stat):
    """Bound of running = momentum * running + (1 - momentum) * stat after one step: the inputs' own errors pass through with their
    weights; the float32 momentum and 1 - momentum, the two products and the sum add 4 u (|momentum running| + |(1 - momentum) stat|)."""
    return momentum * d_prev + (1.0 - momentum) * d_stat + 4 * U24 * (np.abs(momentum * run_prev) + np.abs((1.0 - momentum) * stat))


def mse_sum_c(n):
    """c of the MSE loss sum (mse_small_kernel / mse_kernel + mse_final_kernel).  k = 4: p - t, the square, and the final * (1 / n)
    with its rounded 1 / n.
        n <= 16384   one 1024-thread block: chain ceil(n / 1024) <= 16, tree 6 + 16                        -> at most 16 + 22 + 4 = 42
        n >  16384   blocks = min(ceil(n / 1024), 1024) of 256 threads: chain ceil(n / (256 blocks)) -- 4 while the grid is not capped
                     (16385 -> 4, 100003 -> 4), 5 at 2^20 + 13 (the capped grid wraps once more for the last 13) -- tree 6 + 4; then
                     mse_final_kernel over the partials: chain ceil(blocks / 256) <= 4, tree 6 + 4             -> at most 5 + 10 + 4 + 10 + 4 = 33
    so c = 64 covers every size the tests use (asserted where it is used)."""
    if n <= 16384:
        return -(-n // 1024) + WAVE_TREE + 16 + 4
    blocks = min(-(-n // 1024), 1024)
    return -(-n // (256 * blocks)) + WAVE_TREE + 4 + -(-blocks // 256) + WAVE_TREE + 4 + 4


def sum_bound(terms, c, axis=None):
    """c * 2^-24 * sum|terms|: the bound of a float32 sum against the exact one (see the module docstring)."""
    return c * U24 * np.sum(np.abs(np.asarray(terms, np.float64)), axis=axis)
