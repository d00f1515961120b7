"""AvgPool2d restated in float64 (neunet/nn/layers/avgpool2d.py:126-172 forward, :14-46 backward -- the taps, the count that includes
the zero padding, and the crop, but with the correct (up, down, left, right) crop where the reference sizes its buffer from the first
two entries of the 4-tuple), the host's tier rule of csrc/avgpool.hip restated (route, tiles_mode), the case table and the bounds.
Shared by tests/test_shape_layers.py (CPU), tests/test_shape_layers_gpu.py and tools/gen_golden.py (gen_shape_layers records the
reference on the equal-padding rows).

Bounds, with u = 2^-24, n = kh kw and m = the number of windows that cover an input element:
    forward   |y  - y64 | <= (n + 2) u (sum |taps| / n)
    backward  |dx - dx64| <= (m + 2) u (sum |dY_j| / n)          and an element no window covers is exactly +0.0
n - 1 (m - 1) additions, the scale -- a divide, or a multiply by the rounded reciprocal -- and one to spare.  Derived, not fitted."""
import numpy as np

U = 2.0 ** -24
GLOBAL_WAVE_MAX = 1024              # kAvgGlobalWaveMax (csrc/avgpool.hip): planes up to here take one wave, larger ones a block

# (shape, kernel, stride, padding, what it exercises): the smallest shapes at which each thing can break
CASES = [
    ((2, 3, 6, 6), 2, None, 0, "tiles"),
    ((1, 1, 4, 6), 2, None, 0, "tiles, row length not a multiple of 4"),
    ((1, 2, 8, 12), (2, 4), None, 0, "tiles, 16-byte path"),
    ((3, 2, 64, 64), 2, None, 0, "tiles over several blocks"),
    ((2, 4, 9, 11), (2, 3), (2, 3), 0, "leftover row and column: not tiles, their gradient 0"),
    ((1, 2, 7, 5), 2, None, 0, "leftover again"),
    ((1, 1, 5, 5), 3, 1, 0, "overlap"),
    ((1, 1, 8, 8), 2, 3, 0, "gaps"),
    ((2, 3, 7, 5), 3, 2, 1, "equal padding"),
    ((1, 2, 7, 5), (3, 2), (2, 1), (1, 1), "rectangular kernel and stride with padding"),
    ((1, 2, 13, 13), 5, 2, 2, "larger kernel with padding"),
    ((1, 1, 3, 3), 3, 1, 3, "windows wholly in the padding"),
    ((1, 2, 7, 5), 3, 1, (1, 2), "unequal padding"),
    ((1, 2, 7, 5), 3, 1, (1, 0, 2, 1), "4-tuple padding"),
    ((2, 3, 7, 5), (7, 5), None, 0, "global"),
    ((2, 64, 7, 7), 7, None, 0, "global"),
    ((1, 2, 40, 40), 40, None, 0, "global, plane larger than one wave pass"),
    ((1, 2, 1, 1), 1, None, 0, "global, identity"),
    # one case on each side of route()'s only numeric threshold (GLOBAL_WAVE_MAX elements per plane)
    ((1, 2, 32, 32), 32, None, 0, "global, the largest plane one wave takes"),
    ((1, 2, 25, 41), (25, 41), None, 0, "global, the smallest plane a block takes"),
]


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def geometry(shape, kernel, stride, padding):
    """The descriptor fields (nnhipPool2dDesc) plus Ho, Wo, as the module derives them (avgpool2d.py:52-62, :110-123)."""
    B, C, H, W = shape
    kh, kw = pair(kernel)
    sh, sw = pair(stride) if stride else (kh, kw)
    p = pair(padding)
    pu, pd, pl, pr = (p[0], p[0], p[1], p[1]) if len(p) == 2 else p
    return dict(B=B, C=C, H=H, W=W, kh=kh, kw=kw, sh=sh, sw=sw, pu=pu, pd=pd, pl=pl, pr=pr,
                Ho=(H + pu + pd - kh) // sh + 1, Wo=(W + pl + pr - kw) // sw + 1)


def case_id(case):
    shape, k, s, p, _ = case
    return "x".join(map(str, shape)) + f"-k{k}-s{s}-p{p}".replace(" ", "")


def equal_padding(case):
    """The rows whose backward the reference can run: vertical padding == horizontal padding, given as an int or a 2-tuple."""
    p = pair(case[3])
    return len(p) == 2 and p[0] == p[1]


def route(g):
    """avgpool_tier (csrc/avgpool.hip): 'general' | 'tiles' | 'global_wave' | 'global_block'.  global before tiles."""
    if g["pu"] + g["pd"] + g["pl"] + g["pr"] != 0:
        return "general"
    if g["kh"] == g["H"] and g["kw"] == g["W"]:
        return "global_wave" if g["H"] * g["W"] <= GLOBAL_WAVE_MAX else "global_block"
    if g["kh"] == g["sh"] and g["kw"] == g["sw"] and g["H"] == g["Ho"] * g["kh"] and g["W"] == g["Wo"] * g["kw"]:
        return "tiles"
    return "general"


TIER_IDS = {"general": 0, "tiles": 1, "global_wave": 2, "global_block": 3}          # NNHIP_AVGPOOL_TIER_*


def tiles_mode(g, full_ptr, pooled_ptr):
    """avgpool_tiles_mode: 1 = pairs of 2-wide windows through float4 / float2, 2 = 4-wide windows through float4, 0 = scalar.
    full_ptr: the full-resolution tensor (X / dX), pooled_ptr: the pooled one (out / dY)."""
    if g["kw"] == 2 and g["W"] % 4 == 0 and full_ptr % 16 == 0 and pooled_ptr % 8 == 0:
        return 1
    if g["kw"] == 4 and full_ptr % 16 == 0:
        return 2
    return 0


def _pad64(X, g):
    return np.pad(np.asarray(X, np.float64), ((0, 0), (0, 0), (g["pu"], g["pd"]), (g["pl"], g["pr"])))


def forward64(X, g):
    """(y, sum |taps|) in float64."""
    Xp = _pad64(X, g)
    Ap = np.abs(Xp)
    y = np.zeros((g["B"], g["C"], g["Ho"], g["Wo"]))
    a = np.zeros_like(y)
    for r in range(g["kh"]):
        for s in range(g["kw"]):
            win = (slice(None), slice(None), slice(r, r + g["sh"] * g["Ho"], g["sh"]), slice(s, s + g["sw"] * g["Wo"], g["sw"]))
            y += Xp[win]
            a += Ap[win]
    return y / (g["kh"] * g["kw"]), a


def backward64(dY, g):
    """(dX, sum |dY_j| over the covering windows, m = their number) in float64 / int."""
    Hp, Wp = g["H"] + g["pu"] + g["pd"], g["W"] + g["pl"] + g["pr"]
    dY = np.asarray(dY, np.float64)
    acc = np.zeros((3, g["B"], g["C"], Hp, Wp))
    for r in range(g["kh"]):
        for s in range(g["kw"]):
            win = (slice(None), slice(None), slice(r, r + g["sh"] * g["Ho"], g["sh"]), slice(s, s + g["sw"] * g["Wo"], g["sw"]))
            acc[0][win] += dY
            acc[1][win] += np.abs(dY)
            acc[2][win] += 1
    crop = acc[:, :, :, g["pu"]:Hp - g["pd"], g["pl"]:Wp - g["pr"]]
    return crop[0] / (g["kh"] * g["kw"]), crop[1], crop[2].astype(np.int64)


def forward_bound(sumabs, g):
    n = g["kh"] * g["kw"]
    return (n + 2) * U * sumabs / n


def backward_bound(sumabs, m, g):
    return (m + 2) * U * sumabs / (g["kh"] * g["kw"])


def check_forward(got, X, g, what=""):
    """Asserts the forward bound; returns the largest error / bound ratio (0 where the bound is 0 and the result exact)."""
    y, a = forward64(X, g)
    return _check(got, y, forward_bound(a, g), what + " forward")


def check_backward(got, dY, g, what=""):
    dx, a, m = backward64(dY, g)
    got = np.asarray(got)
    hole = m == 0
    if hole.any():
        h = got[hole]
        assert not h.any() and not np.signbit(h).any(), f"{what} backward: an element no window covers is not +0.0"
    return _check(got, dx, backward_bound(a, m, g), what + " backward")


def _check(got, ref, bound, what):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, f"{what}: {got.dtype} {got.shape} vs {ref.shape}"
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements over the bound, worst error {err[bad].max():.3e} at bound {bound[bad][np.argmax(err[bad])]:.3e}"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio.max()) if ratio.size else 0.0
