"""float64 restatement of the vector-quantisation entries (csrc/vector_quantize.hip): the nearest-code search under np.argmin's rule, its
near-optimality bound per tier, vq_loss + beta * commit_loss with both gradients and their rounding bounds, the last-wins codebook
gradient and the straight-through gradient.

The search's guarantee.  The kernel does not promise the float64 argmin: it ranks codes by a float32 score and two codes closer than
the score's rounding error may swap.  It promises NEAR-OPTIMALITY in exact arithmetic,

    d(n, idx[n]) - min_k d(n, k) <= bound_n,        d(n, k) = sum_j (z_nj - e_kj)^2,

and therefore idx[n] == argmin wherever the gap between the two nearest codes exceeds bound_n.  With u = 2^-24 and
g(m) = m u / (1 - m u) (the standard bound on a product of m factors (1 + delta), |delta| <= u):

  narrow tier (D <= VQ_NARROW_MAX_D), direct form.  Per component t = fl(z - e) (one rounding, exact at underflow), then s = fma(t, t, s):
  t^2 carries (1 + d)^2 and every later fma of the chain one more factor, so the computed score S_k = d(n, k) (1 + theta), |theta| <=
  g(D + 2) =: G.  If the kernel prefers c to the true nearest k*, S_c <= S_k*, hence d_c (1 - G) <= d_k* (1 + G) and
      d_c - d_k* <= 2 G d_k* / (1 - G)                                               = narrow_bound.
  (A product t t below 2^-126 loses at most 2^-149 absolutely: D 2^-148 is added for the two scores.)

  wide tier, expansion form  S_k = fl(nrm_k - 2 acc_k):
    acc_k  -- the MFMA's k-ordered fma chain over the D components (zero padding adds exact zeros): |acc - z.e| <= g(D) |z| |e|;
    nrm_k  -- per kq lane an fma chain over its 4 ceil(D / 16) <= D components, then two adds across the four lanes:
              |nrm - |e|^2| <= g(D + 2) |e|^2;
    the final fmaf(-2, acc, nrm) -- one rounding of a value of size <= |e|^2 + 2 |z| |e| (to first order).
  Together |S_k - (|e_k|^2 - 2 z.e_k)| <= g(D + 3) (|e_k|^2 + 2 |z| |e_k|) <= g(D + 3) (|z| + |e_k|)^2, and two scores are compared:
      d_c - d_k* <= VQ_WIDE_C g(D + 3) (|z_n| + max_k |e_k|)^2,    VQ_WIDE_C = 2      = wide_bound
  (plus (2 D + 4) 2^-149 for products that underflow).  The constants restate the kernel source (tests/test_vq.py checks them)."""
import numpy as np

U24 = 2.0 ** -24
TINY = 2.0 ** -149
VQ_NARROW_MAX_D = 8          # NNHIP_VQ_NARROW_MAX_D
VQ_WIDE_RESIDENT_D = 256     # beyond: the looped-D path of the wide tier
VQ_ROWS = 16                 # rows per block of the wide tier
VQ_SUPER = 64                # codes per super-tile (VQ_TILES x 16)
VQ_NARROW_CODES = 512        # codes per LDS tile of the narrow tier
VQ_WIDE_C = 2.0
VQ_LOSS_THREADS = 1024


def gamma(m):
    return m * U24 / (1.0 - m * U24)


def distances(z, e):
    """d[n, k] = sum_j (z_nj - e_kj)^2 in float64, the direct form (no cancellation)."""
    z, e = np.asarray(z, np.float64), np.asarray(e, np.float64)
    z = z.reshape(-1, z.shape[-1])
    out = np.empty((z.shape[0], e.shape[0]))
    step = max(1, (1 << 22) // max(1, e.shape[0] * e.shape[1]))          # row chunks: the N x K x D temporary stays below 32 MB
    for lo in range(0, z.shape[0], step):
        out[lo:lo + step] = ((z[lo:lo + step, None, :] - e[None, :, :]) ** 2).sum(-1)
    return out


def nearest(z, e):
    """(indices, z_q) under np.argmin's rule: ties to the lower index, a NaN distance beats any number, the first NaN wins."""
    d = distances(z, e)
    idx = np.argmin(d, axis=1).astype(np.int32)
    return idx, np.asarray(e)[idx]


def is_narrow(D):
    return D <= VQ_NARROW_MAX_D


def narrow_bound(z, e, d=None):
    d = distances(z, e) if d is None else d
    D = np.asarray(e).shape[1]
    G = gamma(D + 2)
    return 2.0 * G * d.min(axis=1) / (1.0 - G) + D * 2.0 * TINY


def wide_bound(z, e):
    z, e = np.asarray(z, np.float64), np.asarray(e, np.float64)
    z = z.reshape(-1, z.shape[-1])
    D = e.shape[1]
    zn, en = np.sqrt((z * z).sum(1)), np.sqrt((e * e).sum(1)).max()
    return VQ_WIDE_C * gamma(D + 3) * (zn + en) ** 2 + (2 * D + 4) * TINY


def nearest_bound(z, e, d=None):
    """bound_n of the tier the kernel takes at this D."""
    return narrow_bound(z, e, d) if is_narrow(np.asarray(e).shape[1]) else wide_bound(z, e)


def excess(z, e, idx, d=None):
    """d(n, idx[n]) - min_k d(n, k) per row."""
    d = distances(z, e) if d is None else d
    return d[np.arange(d.shape[0]), np.asarray(idx, np.int64)] - d.min(axis=1)


def second_gap(d):
    """Per row: the distance of the second-nearest code minus the nearest's (0 for a duplicated nearest code, inf for K = 1)."""
    if d.shape[1] == 1:
        return np.full(d.shape[0], np.inf)
    two = np.partition(d, 1, axis=1)[:, :2]
    return two[:, 1] - two[:, 0]


# ------------------------------------------------------------------------------------------------------------------------ the loss
def vq_loss(z_e, z_q, beta):
    """(loss, dz_e, dz_q) of vq_loss + beta * commit_loss = (1 + beta) mean((z_q - z_e)^2); beta as the float32 the entry receives."""
    ze, zq, b = np.asarray(z_e, np.float64), np.asarray(z_q, np.float64), float(np.float32(beta))
    n = ze.size
    d = zq - ze
    return (1.0 + b) * (d * d).sum() / n, -2.0 * b * d / n, 2.0 * d / n


def vq_loss_sum_c(n):
    """Roundings on the way to loss[0]: the term (the difference squared: 2), a thread's strided fma chain (ceil(n / 1024)), wave_sum
    (4 DPP steps + 2 levels over the four rows: 6), block_sum over the 16 waves (16), the scale (1 + beta, float(n), the division, the
    product: 4)."""
    return 2 + -(-n // VQ_LOSS_THREADS) + 6 + VQ_LOSS_THREADS // 64 + 4


def vq_loss_bounds(z_e, z_q, beta):
    """(loss bound, dz_e bound, dz_q bound).  Gradients: d = fl(z_q - z_e), the factor 2 / n (float(n) and a division: 2 roundings),
    times beta for dz_e (1), the product (1): 4 resp. 5 roundings of |reference|, plus one underflow quantum."""
    loss, dze, dzq = vq_loss(z_e, z_q, beta)
    n = np.asarray(z_e).size
    return gamma(vq_loss_sum_c(n)) * loss + n * TINY, gamma(5) * np.abs(dze) + TINY, gamma(4) * np.abs(dzq) + TINY


# ------------------------------------------------------------------------------------------------------------------- tape gradients
def last_wins_codebook_grad(grad, idx, K):
    """The reference's Embedding gradient (Tensor.__getitem__'s backward: `_grad[index] = grad`, an ASSIGNMENT): row k of the result is
    the gradient row of the LAST n with idx[n] == k, zero for a code no row chose."""
    grad = np.asarray(grad, np.float64)
    grad = grad.reshape(-1, grad.shape[-1])
    out = np.zeros((K, grad.shape[1]))
    out[np.asarray(idx, np.int64).reshape(-1)] = grad          # NumPy's fancy assignment keeps the last write, as the reference does
    return out


def straight_through_grad(grad):
    """z + (z_q - z).detach(): z receives z_q's gradient unchanged."""
    return np.asarray(grad, np.float64)
