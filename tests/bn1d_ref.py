"""Float64 restatements of the operations behind the MLP generative examples (examples/gan.py, examples/vae.py) -- BatchNorm1d, Tanh,
BCELoss, the Gaussian reparameterisation and the KL term -- written from the reference's layer sources, NumPy only, independent of
the kernels; and the rounding bounds of the kernels' sums, derived from their element -> thread maps (nothing tuned to a run).
tests/test_mlp_generative.py holds them against the reference's fixtures; tests/test_bn1d_tiers_gpu.py and
tests/test_mlp_generative_gpu.py hold the kernels against them.

BatchNorm1d on [N, F] is BatchNorm2d on [N, F, 1, 1] (neunet/nn/layers/batchnorm1d.py:15-41, 66-99 against batchnorm2d.py): the same
statistics over axis 0, the same running-statistics convention, the same one backward formula -- the restatement reuses
vision_ref.batchnorm_forward / batchnorm_backward at that shape (checked against the reference's own 1d formula in
test_mlp_generative.py)."""
import numpy as np

from vision_ref import FLT_MIN, U24, batchnorm_backward, batchnorm_forward

# ---- the element -> thread map of csrc/batchnorm1d.hip, restated ----------------------------------------------------------------
BN1_SW = 16                      # features per block (strip width)
BN1_NW = 16                      # waves per block
BN1_RG = BN1_NW * (64 // BN1_SW)  # row slots per block: 64
BN1_NE = 16                      # rows per thread in the register tier
BN1_REG_ROWS = BN1_RG * BN1_NE   # 1024: the last N of the register tier


def bn1_fits_regs(N, F):
    """bn1_fits_regs() of csrc/batchnorm1d.hip, restated: the register tier's condition (else: the looped tier)."""
    return N <= BN1_RG * BN1_NE and N * F <= 2 ** 29


# ---- BatchNorm1d ------------------------------------------------------------------------------------------------------------
def batchnorm1d_forward(X, w, b, running_mean, running_var, eps, momentum, training):
    """(Y [N, F], mean [F], inv [F], new running mean, new running var) in float64: batchnorm1d.py:66-99."""
    X = np.asarray(X, np.float64)
    Y, mean, inv, rm, rv = batchnorm_forward(X[:, :, None, None], w, b, running_mean, running_var, eps, momentum, training)
    return Y[:, :, 0, 0], mean, inv, rm, rv


def batchnorm1d_backward(X, w, mean, inv, dY):
    """(dX, dW, db) in float64: batchnorm1d.py:15-41, the one formula of both modes."""
    X, dY = np.asarray(X, np.float64), np.asarray(dY, np.float64)
    dX, dW, db = batchnorm_backward(X[:, :, None, None], w, mean, inv, dY[:, :, None, None])
    return dX[:, :, 0, 0], dW, db


def batchnorm1d_backward_reference_form(X, w, mean, inv, dY):
    """The reference's own expression, term for term (batchnorm1d.py:18-36), for the identity check against the 2d restatement."""
    X, dY = np.asarray(X, np.float64), np.asarray(dY, np.float64)
    N = X.shape[0]
    xc = X - mean[None, :]
    si = inv[None, :]
    wd = 1.0 if w is None else np.asarray(w, np.float64).reshape(1, -1)
    dX = (1 / N) * wd * si * (N * dY - dY.sum(axis=0) - xc * si ** 2 * (dY * xc).sum(axis=0))
    return dX, (dY * xc * si).sum(axis=0), dY.sum(axis=0)


def bn1_sum_c(N):
    """c of the column sums of the BatchNorm1d kernels (one element -> thread map for all four: bn1_thread() in batchnorm1d.hip).
    A 1024-thread block owns 16 features; a wave's 64 lanes are 4 row groups x 16 features, so the block has 64 row slots and a
    thread takes rows slot, slot + 64, ... of one feature:
        chain   ceil(N / 64) additions in one thread's accumulator (16 at the register tier's last N = 1024),
        tree    2 xor-shuffle additions fold the four row groups of a wave, then 16 for the serial sum over the sixteen waves'
                partials in LDS (bn1_colsum),
        k = 2   the term's own arithmetic: a subtraction and a multiplication ((x - mean)^2, g * (x - mean))."""
    return -(-N // BN1_RG) + 2 + BN1_NW + 2


def bn1_stat_bounds(X, eps):
    """vision_ref.bn_stat_bounds restated for [N, F] with this kernel's c: bounds of save_mean, the batch variance and save_inv
    against float64, per feature."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    c = bn1_sum_c(n)
    mean = X.mean(axis=0)
    var = ((X - mean[None, :]) ** 2).mean(axis=0)
    dmean = c * U24 * np.abs(X).sum(axis=0) / n + U24 * np.abs(mean)
    dvar = c * U24 * var + dmean ** 2 + 2 * U24 * var
    inv = 1.0 / np.sqrt(var + eps)
    dinv = inv * (dvar / (2.0 * (var + eps)) + 3 * U24)
    return dmean, dvar, dinv


# ---- Tanh ---------------------------------------------------------------------------------------------------------------------
def tanh_forward(x):
    """f = tanh(x) (neunet/nn/activations.py:120-122)."""
    return np.tanh(np.asarray(x, np.float64))


def tanh_backward(f, dy):
    """dx = dy (1 - f^2), f the activation's OUTPUT (activations.py:107-110)."""
    f, dy = np.asarray(f, np.float64), np.asarray(dy, np.float64)
    return dy * (1.0 - f ** 2)


def tanh_backward_bound(f, dy):
    """The kernel's three operations (f * f, 1 - ., dy * .), each rounded once (or the first two fused into one rounding):
    |dy| u (f^2 + |1 - f^2|) + u |dx|, plus one float32 underflow."""
    f, dy = np.asarray(f, np.float64), np.asarray(dy, np.float64)
    return np.abs(dy) * U24 * (f ** 2 + np.abs(1.0 - f ** 2)) + U24 * np.abs(tanh_backward(f, dy)) + FLT_MIN


# ---- BCELoss ------------------------------------------------------------------------------------------------------------------
def bce_terms(p, y, w=None):
    """-(y log p + (1 - y) log(1 - p)) w per element (neunet/nn/losses.py:36-46 and the final mul(-1)); no clamp."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    w = 1.0 if w is None else np.asarray(w, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return -((y * np.log(p) + (1.0 - y) * np.log(1.0 - p)) * w)


def bce(p, y, w=None, reduction="mean"):
    """(loss, d loss / dp, d loss / dz with p = sigmoid(z)) of BCELoss (losses.py:25-56) for a unit upstream gradient; for 'none' the
    loss is the array of terms and the gradients are those of its sum."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    wd = np.ones_like(p) if w is None else np.broadcast_to(np.asarray(w, np.float64), p.shape)
    t = bce_terms(p, y, wd)
    scale = 1.0 / p.size if reduction == "mean" else 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        dp = -(y / p - (1.0 - y) / (1.0 - p)) * wd * scale
    dz = (p - y) * wd * scale
    loss = t if reduction == "none" else (t.sum() * scale)
    return loss, dp, dz


BCE_K = 8      # one term's own arithmetic: logf at 2 ulp (one log per addend), y * log, the rounding of 1 - y and its product, the
               # addition, the weight, the final scale


def bce_sum_c(n):
    """c of the BCE / KLD loss sums (ll_small_kernel / ll_part_kernel + ll_final_kernel in losses_latent.hip: the element -> thread map
    of the MSE kernels, vision_ref.mse_sum_c, with this term's k)."""
    if n <= 16384:
        return -(-n // 1024) + 6 + 16 + BCE_K
    blocks = min(-(-n // 1024), 1024)
    return -(-n // (256 * blocks)) + 6 + 4 + -(-blocks // 256) + 6 + 4 + BCE_K


def bce_term_bound(p, y, w=None, k=BCE_K):
    """Per-element bound of one float32 term: k u |term|, plus u (1 - y) w for the rounding of 1 - p, which enters log(1 - p) as an
    ABSOLUTE error u (d log(1 - p) = -dp / (1 - p)) -- not small relative to a log that is itself near 0 -- plus one underflow."""
    y = np.asarray(y, np.float64)
    wd = 1.0 if w is None else np.abs(np.asarray(w, np.float64))
    return k * U24 * np.abs(bce_terms(p, y, w)) + U24 * np.abs(1.0 - y) * wd + FLT_MIN


def bce_loss_bound(p, y, w=None, reduction="mean"):
    """Bound of the reduced loss: every term passes through at most c - k additions (its own arithmetic is in bce_term_bound)."""
    n = np.asarray(p).size
    scale = 1.0 / n if reduction == "mean" else 1.0
    return float((bce_sum_c(n) - BCE_K) * U24 * np.abs(bce_terms(p, y, w)).sum() + bce_term_bound(p, y, w).sum()) * scale


# ---- the VAE's latent expressions -------------------------------------------------------------------------------------------------
def reparam(mu, logvar, eps, g=None):
    """z = mu + eps exp(logvar / 2) (examples/vae.ipynb, VAE.reparameterize); with g = dL/dz also (dmu, dlogvar) = (g, g eps std / 2)."""
    mu, lv, eps = (np.asarray(a, np.float64) for a in (mu, logvar, eps))
    std = np.exp(0.5 * lv)
    z = mu + eps * std
    if g is None:
        return z
    g = np.asarray(g, np.float64)
    return z, g, g * eps * 0.5 * std


def reparam_bound(mu, logvar, eps):
    """z: expf at 2 ulp, the product, one to spare on eps std; the final addition on z."""
    z = reparam(mu, logvar, eps)
    es = np.abs(np.asarray(eps, np.float64) * np.exp(0.5 * np.asarray(logvar, np.float64)))
    return U24 * np.abs(z) + 4 * U24 * es + FLT_MIN


def kld(mu, logvar):
    """(KLD, dKLD/dmu, dKLD/dlogvar): -1/2 sum(1 + logvar - mu^2 - exp(logvar)) (examples/vae.ipynb, VAE.loss_function)."""
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    return float(-0.5 * np.sum(1.0 + lv - mu ** 2 - np.exp(lv))), mu.copy(), 0.5 * (np.exp(lv) - 1.0)


def kld_bound(mu, logvar):
    """The terms 1 + logvar - mu^2 - exp(logvar) cancel (0 at mu = logvar = 0), so a term's own rounding is bounded by its PARTS:
    6 u (1 + |logvar| + mu^2 + exp(logvar)) -- expf at 2 ulp, the square, three additions; the sum's additions by (c - k) u sum|term|."""
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    t = 1.0 + lv - mu ** 2 - np.exp(lv)
    parts = 1.0 + np.abs(lv) + mu ** 2 + np.exp(lv)
    c = bce_sum_c(mu.size) - BCE_K + 1                      # + the final * -0.5 ... exact; + 1 to spare
    return float(0.5 * (c * U24 * np.abs(t).sum() + 6 * U24 * parts.sum())) + FLT_MIN
