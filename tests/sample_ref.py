"""NumPy restatement of nnhipSampleTopK's contract (include/neunet_hip.h, csrc/sample.hip): the uniform's hash in uint32
arithmetic, the candidate order, the float64 CDF and the acceptance rule of a draw.  No device code is involved."""
import numpy as np

M32 = 0xFFFFFFFF


def _u32(a):
    return np.asarray(a, dtype=np.uint64) & np.uint64(M32)


def uniform(seed, word, rows):
    """u of rows `rows` (an int: rows 0 .. rows-1, or an array of row numbers) for s = seed + word mod 2^32: the lowbias32-style
    hash of csrc/common.h (at_hash(at_rowkey(s, r), 0)), its top 24 bits scaled to [0, 1).  seed / word may be arrays too."""
    r = np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint64)
    s = _u32(_u32(seed) + _u32(word))
    x = _u32(_u32(s * np.uint64(0x85EBCA6B)) + np.uint64(0x9E3779B9)) ^ _u32(_u32(r) * np.uint64(0xC2B2AE35))
    x = x ^ (x >> np.uint64(16))
    x = _u32(x * np.uint64(0x7FEB352D))
    x = x ^ (x >> np.uint64(15))
    x = _u32(x * np.uint64(0x846CA68B))
    x = x ^ (x >> np.uint64(16))
    return ((x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def candidates(x, k):
    """Indices of the min(k, n) best elements of the row x, best first, under nnhipArgmaxF32's total order: a NaN beats any
    number, a larger value beats a smaller one (-0 == +0), ties go to the lower index."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    order = np.lexsort((np.arange(x.size), -np.where(nan, np.float32(0), x), ~nan))
    return order[:min(int(k), x.size)]


def cdf64(x, idx, t):
    """Cumulative probabilities of the sorted candidates idx at temperature t, in float64."""
    xs = np.asarray(x, dtype=np.float64)[idx]
    e = np.exp((xs - xs[0]) / max(float(t), 1e-6))
    c = np.cumsum(e)
    return c / c[-1]


def draw64(x, k, t, u):
    """The float64 inverse-CDF sampler: the first sorted candidate whose cumulative probability exceeds u."""
    idx = candidates(x, k)
    j = int(np.searchsorted(cdf64(x, idx, t), float(u), side="right"))
    return int(idx[min(j, len(idx) - 1)])


def check_draw(x, k, t, u, token):
    """Raises AssertionError unless `token` is an acceptable draw for the uniform u: candidate j with
    cdf64[j-1] - m <= u <= cdf64[j] + m, m = (k + 32) 2^-22 (k = the number of candidates): four times the bound of the float32
    sequential sum plus the exponentials' rounding.  A degenerate row (best element NaN or not finite) must give that element.
    Returns the slack the draw needed (0 when u lies inside the float64 interval)."""
    x = np.asarray(x, dtype=np.float32)
    idx = candidates(x, k)
    token = int(token)
    assert 0 <= token < x.size, f"token {token} outside [0, {x.size})"
    x0 = x[idx[0]]
    if not np.isfinite(x0):
        assert token == idx[0], f"degenerate row (best = {x0}): token {token}, expected {idx[0]}"
        return 0.0
    pos = np.nonzero(idx == token)[0]
    assert pos.size == 1, f"token {token} is not among the {len(idx)} candidates"
    j = int(pos[0])
    assert x[token] != -np.inf, f"token {token} has probability zero (-inf logit)"
    cdf = cdf64(x, idx, t)
    lo, hi = (cdf[j - 1] if j else 0.0), cdf[j]
    m = (len(idx) + 32) * 2.0 ** -22
    u = float(u)
    assert lo - m <= u <= hi + m, f"token {token} = candidate {j}: u = {u!r} outside [{lo!r}, {hi!r}] -+ {m:.3g}"
    return max(lo - u, u - hi, 0.0)


def ks_distance(u):
    """Kolmogorov-Smirnov distance of the sample u to U(0, 1)."""
    u = np.sort(np.asarray(u, dtype=np.float64))
    n = u.size
    i = np.arange(1, n + 1)
    return float(max(np.max(i / n - u), np.max(u - (i - 1) / n)))
