"""ConvTranspose2d in float64, written from the closed form of the reference layer (neunet/nn/layers/convtranspose2d.py)
rather than from its as_strided code:

    O[b,o,y,x] = bias[o] + sum_{i,k,l} W[o,i,k,l] X[b,i,h,w]   with   h sh = y + pu - (kh-1-k) dh,   w sw = x + pl - (kw-1-l) dw
    Ho = (H-1) sh - (pu+pd) + dh (kh-1) + oph + 1    (likewise Wo)

i.e. input pixel h feeds output row y = h sh - pu + (kh-1-k) dh through tap k.  The weight is [out, in, kh, kw] and is NOT
flipped; this equals torch's conv_transpose2d with W.flip(2, 3).transpose(0, 1).  Shared by the CPU and the GPU tests, as are the
tier table and the restatement of the library's selection rules (route, tile, k-loop length per phase, weight-gradient configuration)
further down."""
import numpy as np

# (B, Cin, H, W, Cout, kernel, stride, padding, dilation, output_padding): the fixtures of tools/gen_golden.py:gen_convtranspose
GEOMETRIES = {
    "convt_k4s2p1": (2, 3, 4, 4, 5, 4, 2, 1, 1, 0),
    "convt_uneven": (2, 5, 4, 5, 3, (3, 2), (2, 3), (0, 1), 1, (1, 2)),
    "convt_dil_gcd": (2, 4, 4, 4, 3, 3, 2, 1, 2, 1),
    "convt_s3k2": (1, 2, 3, 3, 3, 2, 3, 0, 1, 0),
    "convt_mixed": (1, 2, 3, 4, 3, 3, (3, 2), (2, 0), (1, 2), (0, 1)),
    "convt_op_ge_s": (2, 2, 3, 4, 3, 3, 2, 1, 3, 2),
    "convt_s1_bigpad": (1, 2, 5, 5, 3, 3, 1, 3, 1, 0),
    "convt_pad4": (2, 4, 4, 4, 3, 3, 2, (1, 2, 0, 1), 1, 1),
    "convt_unet_in": (2, 3, 8, 8, 4, 5, 1, 0, 1, 0),
    "convt_unet_out": (2, 8, 6, 6, 3, 3, 1, 1, 1, 0),
}
# which stride phases have no tap (row-major (py, px)), for the fixtures that have such phases
EMPTY_PHASES = {
    "convt_uneven": [2, 5],               # kw = 2 < sw = 3: taps s in {0, 1} reach px in {0, 1} of 3
    "convt_dil_gcd": [1, 2, 3],           # r*2 mod 2 is always 0: only phase (0, 0) is reached
    "convt_s3k2": [2, 5, 6, 7, 8],        # taps r in {0, 1} reach py in {0, 1} of 3
    "convt_mixed": [1, 3, 5],             # x: dilation 2, stride 2 -> px = 0 only
}

# Tier table (tests/test_convtranspose.py: test_tier_table_reaches_every_condition checks on the CPU what it reaches; the GPU tests
# run every row).  WM = 2 (128-row tile, BK = 32, BN = 128) when the forward's Cout > 64, else WM = 1 (64 rows, BK = 16, BN = 256);
# T = taps of the phase x channel tiles = the phase's k-loop length; wgrad (WM, CB): WM by Cin > 64, CB by Cout.
TIER_CASES = {
    # WM1, a full 64-row tile, 2 channel tiles; taps per phase 4/2/2/1 -> T = 8, 4, 4, 2; N = 297: 2 pixel tiles that span images;
    # wgrad (1, 64), FLAT
    "k3s2_w1": (3, 17, 9, 11, 64, 3, 2, 1, 1, 1),
    # WM2 with one row in the second m-tile; Cin one over a k-tile; wgrad (1, 128)
    "k3s2_w2": (3, 33, 9, 11, 65, 3, 2, 1, 1, 1),
    # T = 1 on four phases, T = 0 on five; phase sizes 70/56/60/48
    "k2s3_w1": (2, 16, 7, 5, 40, 2, 3, 0, 1, 0),
    # the same at WM2 with 3 channel tiles: T = 3 (odd) and 0; dX on WM2; wgrad (2, 128)
    "k2s3_w2": (2, 70, 7, 5, 130, 2, 3, 0, 1, 2),
    # gcd(d, s) = 2: one phase holds all 9 taps (T = 18), three are empty; wgrad (1, 64) and (1, 256)
    "gcd_w1": (2, 20, 6, 6, 33, 3, 2, 1, 2, 1),
    "gcd_w2": (2, 40, 6, 6, 129, 3, 2, 1, 2, 1),
    # 16 phases, rstep = 2 < stride, T = 18/12/12/8 on four phases, twelve empty
    "d2s4_w2": (2, 36, 5, 5, 70, 5, 4, 2, 2, 3),
    # kh != kw, sh != sw; T = 6/3/0 at WM1 and 4/2/0 at WM2; phase sizes 84/98
    "uneven_w1": (2, 35, 6, 7, 50, (3, 2), (2, 3), (0, 1), 1, (1, 2)),
    "uneven_w2": (2, 35, 6, 7, 100, (3, 2), (2, 3), (0, 1), 1, (1, 2)),
    # dilation on one axis only; phases of 108 and 81 pixels
    "mixed_w2": (3, 64, 5, 6, 96, (3, 4), (3, 2), (2, 0), (1, 2), (0, 1)),
    # four-sided padding, an exact 128-row tile, one channel tile; T = 4, 2, 2, 1; four different phase sizes
    "pad4_w2": (2, 32, 6, 6, 128, 3, 2, (1, 2, 0, 1), 1, 1),
    # output padding >= stride, dilation 3
    "opges_w1": (2, 18, 5, 6, 48, 3, 2, 1, 3, 2),
    # T = 9, 6, 6, 4; Cin one under a k-tile
    "k5s2_w2": (2, 31, 7, 7, 72, 5, 2, 2, 1, 1),
    # 3 channel tiles at WM2 with 4/2/2/1 taps: T = 12, 6, 6, 3 and the fetch moves to the next tap in the middle of a pair of k-tiles
    "k3s2_c3_w2": (2, 70, 5, 5, 72, 3, 2, 1, 1, 1),
    # a 1 x 1 kernel: a single k-tile in one phase, bias only elsewhere; H W % 4 == 0: AVEC on, not FLAT
    "k1s2_w1": (2, 16, 8, 8, 64, 1, 2, 0, 1, 1),
    "k1s2_w2": (2, 32, 8, 8, 66, 1, 2, 0, 1, 1),
    # output extent < stride: phases with zero pixels; db with HW = 4
    "nopix_w1": (5, 9, 1, 1, 7, 2, 3, 0, 1, 0),
    "nopix_w2": (5, 9, 1, 3, 67, 2, (3, 2), 0, 1, 0),
    # padding larger than the kernel reach crops to 6 x 6; nine phases of 8 pixels, T = 4, 2, 1
    "crop_w2": (2, 24, 4, 4, 80, 4, 3, (4, 3, 5, 2), 1, 0),
    # an 11 x 11 output with phases of 144/120/120/100 pixels at BN = 128: the grid is sized for 2 tiles, three phases use 1
    "uneq_tiles_w2": (4, 40, 6, 6, 68, 3, 2, 1, 1, 0),
    # 9 and 8 pixel tiles per phase, ragged last tile; wgrad (1, 32)
    "many_n_w1": (4, 8, 23, 25, 12, 4, 2, 1, 1, 0),
    "many_n_w2": (4, 40, 17, 15, 68, 4, 2, 1, 1, 0),
    # dX on conv_tap_kernel<false, 2>; wgrad (2, 32) and (2, 64)
    "bw_w2_cb32": (2, 66, 5, 5, 20, 3, 2, 1, 1, 1),
    "bw_w2_cb64": (2, 100, 4, 6, 64, 3, 2, 0, 1, 0),
    # stride 1 with padding > d (k-1): not a Conv2d, one phase, always the gather route
    "s1_bigpad_w2": (2, 34, 7, 7, 90, 3, 1, 3, 1, 0),
    # stride 1 with padding <= d (k-1): `auto` hands the layer to Conv2d (the one route the rows above do not resolve to)
    "s1_conv_w2": (2, 34, 7, 7, 90, 3, 1, 1, 1, 0),
}


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def pad4(p):
    p = _pair(p)
    return (p[0], p[0], p[1], p[1]) if len(p) == 2 else tuple(p)


def normalise(geom):
    """-> dict(B, Cin, H, W, Cout, kh, kw, sh, sw, dh, dw, pu, pd, pl, pr, oph, opw, Ho, Wo)"""
    B, Cin, H, W, Cout, k, s, p, d, op = geom
    (kh, kw), (sh, sw), (dh, dw), (oph, opw) = _pair(k), _pair(s), _pair(d), _pair(op)
    pu, pd, pl, pr = pad4(p)
    Ho = (H - 1) * sh - (pu + pd) + dh * (kh - 1) + oph + 1
    Wo = (W - 1) * sw - (pl + pr) + dw * (kw - 1) + opw + 1
    return dict(B=B, Cin=Cin, H=H, W=W, Cout=Cout, kh=kh, kw=kw, sh=sh, sw=sw, dh=dh, dw=dw, pu=pu, pd=pd, pl=pl, pr=pr,
                oph=oph, opw=opw, Ho=Ho, Wo=Wo)


def _tap_axis(n_in, n_out, stride, pad, dil, k, tap):
    """input indices h and the output indices y = h stride - pad + (k-1-tap) dil they feed, both inside their ranges"""
    h = np.arange(n_in)
    y = h * stride - pad + (k - 1 - tap) * dil
    ok = (y >= 0) & (y < n_out)
    return h[ok], y[ok]


def _taps(g):
    for k in range(g["kh"]):
        hs, ys = _tap_axis(g["H"], g["Ho"], g["sh"], g["pu"], g["dh"], g["kh"], k)
        for l in range(g["kw"]):
            ws, xs = _tap_axis(g["W"], g["Wo"], g["sw"], g["pl"], g["dw"], g["kw"], l)
            if hs.size and ws.size:
                yield k, l, np.ix_(hs, ws), np.ix_(ys, xs)


def forward(X, W, b, g, dtype=np.float64):
    """dtype = float32: the same sums in float32 (numpy einsum), to place a float32 reference against the tests' bounds"""
    X, W = np.asarray(X, dtype), np.asarray(W, dtype)
    O = np.zeros((g["B"], g["Cout"], g["Ho"], g["Wo"]), dtype)
    for k, l, src, dst in _taps(g):
        O[(slice(None), slice(None)) + dst] += np.einsum("oi,bihw->bohw", W[:, :, k, l], X[(slice(None), slice(None)) + src])
    if b is not None:
        O += np.asarray(b, dtype).reshape(1, -1, 1, 1)
    return O


def backward(X, W, dO, g, dtype=np.float64):
    """-> dX, dW, db"""
    X, W, dO = np.asarray(X, dtype), np.asarray(W, dtype), np.asarray(dO, dtype)
    dX, dW = np.zeros_like(X), np.zeros_like(W)
    for k, l, src, dst in _taps(g):
        go = dO[(slice(None), slice(None)) + dst]
        dX[(slice(None), slice(None)) + src] += np.einsum("oi,bohw->bihw", W[:, :, k, l], go)
        dW[:, :, k, l] = np.einsum("bihw,bohw->oi", X[(slice(None), slice(None)) + src], go)
    return dX, dW, dO.sum(axis=(0, 2, 3))


def abs_sum(X, W, g):
    return forward(np.abs(X), np.abs(W), None, g)


def dot_bound(X, W, ref, g, c=32.0):
    """The project's dot-product bound (tests/test_hip_parity.py: assert_dot_close) for the forward: per element
    c 2^-24 sum|x||w| + 4 2^-24 |ref|, the sum evaluated by running the restatement on |X|, |W|."""
    return c * 2.0 ** -24 * abs_sum(X, W, g) + 4 * 2.0 ** -24 * np.abs(np.asarray(ref, np.float64))


def tap_pixel_pairs(g):
    """Brute force: the number of (output pixel, tap) pairs per image whose divisions are exact, border ignored."""
    n = 0
    for y in range(g["Ho"]):
        for x in range(g["Wo"]):
            for k in range(g["kh"]):
                if (y + g["pu"] - (g["kh"] - 1 - k) * g["dh"]) % g["sh"]:
                    continue
                for l in range(g["kw"]):
                    n += (x + g["pl"] - (g["kw"] - 1 - l) * g["dw"]) % g["sw"] == 0
    return n


def phase_tap_pixel_counts(g):
    """Brute force per stride phase (row-major (py, px)): -> (taps, pixels), pixels = the output pixels per image with
    ((y + pu) mod sh, (x + pl) mod sw) = (py, px), taps = the taps whose divisions are exact at such a pixel (border ignored; the
    same for every pixel of a phase, which is checked here; for a phase without a pixel: counted from the residues r dh mod sh)."""
    sh, sw = g["sh"], g["sw"]
    ny = [sum(((r * g["dh"]) % sh) == py for r in range(g["kh"])) for py in range(sh)]
    nx = [sum(((s * g["dw"]) % sw) == px for s in range(g["kw"])) for px in range(sw)]
    taps = [ny[py] * nx[px] for py in range(sh) for px in range(sw)]
    pixels = [0] * (sh * sw)
    for y in range(g["Ho"]):
        for x in range(g["Wo"]):
            ph = ((y + g["pu"]) % sh) * sw + (x + g["pl"]) % sw
            pixels[ph] += 1
            n = sum((y + g["pu"] - (g["kh"] - 1 - k) * g["dh"]) % sh == 0 for k in range(g["kh"])) * \
                sum((x + g["pl"] - (g["kw"] - 1 - l) * g["dw"]) % sw == 0 for l in range(g["kw"]))
            assert n == taps[ph], (y, x, n, taps[ph])
    return taps, pixels


def backward_bounds(X, W, dO, refs, g, c=32.0):
    """-> the bounds of dX, dW, db.  dX, dW: the dot-product bound of dot_bound, c 2^-24 sum|.||.| + 4 2^-24 |ref|, the sums taken by
    running backward on |X|, |W|, |dO|.  db: 4 2^-24 sum|dO| per channel + 2^-24 |ref| (the rounding of the float32 result)."""
    u = 2.0 ** -24
    aX, aW, adb = backward(np.abs(X), np.abs(W), np.abs(dO), g)
    rdX, rdW, rdb = refs
    return c * u * aX + 4 * u * np.abs(rdX), c * u * aW + 4 * u * np.abs(rdW), 4 * u * adb + u * np.abs(rdb)


# ---- the library's selection rules, restated (the C++ they copy is named at each) ---------------------------------------------------
ROUTE_PHASE, ROUTE_GATHER, ROUTE_CONV2D = 1, 2, 3
MAX_PHASES = 65535                                                         # conv_transpose.hip: kMaxPhases


def _ceil_div(a, b):
    return -(-a // b)


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def phase_axis(p, pad, stride, out):
    """conv_transpose.hip: phase_axis -> (first output coordinate of the phase, number of coordinates)"""
    first = (p - pad) % stride
    return first, ((out - 1 - first) // stride + 1 if first < out else 0)


def phase_taps(p, d, stride, step, k):
    """conv_transpose.hip: phase_taps -> (first tap r0 with r0 d = p (mod stride), or k; number of taps r0, r0 + step, ... < k)"""
    r0 = k
    for r in range(min(k, stride)):
        if (r * d) % stride == p:
            r0 = r
            break
    return r0, ((k - 1 - r0) // step + 1 if r0 < k else 0)


def tile_cfg(wm):
    """conv_tap.h: TapCfg<WM> / conv_mfma.hip: WgCfg<WM> -> BM, BN, BK"""
    return 64 * wm, 256 // wm, 32 if wm == 2 else 16


def auto_route(g):
    """conv_transpose.hip: make_plan (as_conv2d, full_phases) and resolve_route with `auto`"""
    eh, ew = g["dh"] * (g["kh"] - 1), g["dw"] * (g["kw"] - 1)
    if g["sh"] == 1 and g["sw"] == 1 and g["pu"] <= eh and g["pl"] <= ew and eh - g["pd"] + g["oph"] >= 0 and ew - g["pr"] + g["opw"] >= 0:
        return ROUTE_CONV2D
    phases = g["sh"] * g["sw"]
    if phases == 1 or phases > MAX_PHASES:
        return ROUTE_GATHER
    full = _gcd(g["dh"], g["sh"]) == 1 and _gcd(g["dw"], g["sw"]) == 1 and g["kh"] >= g["sh"] and g["kw"] >= g["sw"]
    return ROUTE_PHASE if full else ROUTE_GATHER


def forced_route(g, requested):
    """resolve_route with the phase / gather route requested: only a stride > 1 layer follows the request"""
    r = auto_route(g)
    return r if r == ROUTE_CONV2D or g["sh"] * g["sw"] == 1 or g["sh"] * g["sw"] > MAX_PHASES else requested


def forward_plan(g):
    """conv_transpose.hip: launch_conv_phase (:210-235: the tile, Mp / Csp, tiles_m, the grid's pixel tiles, rstep / sstep) and the
    head of conv_phase_kernel (:63-76 per block: N, the `n0 >= N` return, nt; :135-136: T).  -> dict(wm, m_tiles, ctiles, rstep, sstep, grid_n, phases) with
    phases = [dict(taps, pixels, T, N, tiles, spans)] row-major in (py, px); spans: a pixel tile of the phase holds pixels of two
    images."""
    wm = 2 if g["Cout"] > 64 else 1
    BM, BN, BK = tile_cfg(wm)
    ctiles = _ceil_div(g["Cin"], BK)
    rstep, sstep = g["sh"] // _gcd(g["dh"], g["sh"]), g["sw"] // _gcd(g["dw"], g["sw"])
    grid_n = _ceil_div(g["B"] * _ceil_div(g["Ho"], g["sh"]) * _ceil_div(g["Wo"], g["sw"]), BN)
    phases = []
    for py in range(g["sh"]):
        _, nyq = phase_axis(py, g["pu"], g["sh"], g["Ho"])
        _, nr = phase_taps(py, g["dh"], g["sh"], rstep, g["kh"])
        for px in range(g["sw"]):
            _, nxq = phase_axis(px, g["pl"], g["sw"], g["Wo"])
            _, ns = phase_taps(px, g["dw"], g["sw"], sstep, g["kw"])
            hwq = nyq * nxq
            N = g["B"] * hwq
            tiles = _ceil_div(N, BN)
            assert tiles <= grid_n, "the grid is sized for the largest phase"
            # image b starts at column b hwq: inside a tile iff it is no multiple of BN
            spans = any((b * hwq) % BN for b in range(1, g["B"])) if hwq else False
            phases.append(dict(taps=nr * ns, pixels=hwq, T=nr * ns * ctiles, N=N, tiles=tiles, spans=spans))
    return dict(wm=wm, m_tiles=_ceil_div(g["Cout"], BM), ctiles=ctiles, rstep=rstep, sstep=sstep, grid_n=grid_n, phases=phases)


def backward_plan(g, aligned=True):
    """The stride > 1 backward of nnhipConvTranspose2dBackward (conv_transpose.hip:405-416).  dX: conv_mfma.hip: launch_conv_tap<false>
    on the mirrored geometry (:262-264: M = the layer's Cin, `wm = M > 64 ? 2 : 1`; :321 cvec: H W % 4 == 0 and dX 16-byte aligned).
    dW: conv_mfma.hip: conv_mfma_wgrad with dO in the input role and X in the output-gradient role: :737 `wm = g.Cout > 64` is the
    layer's Cin, :740-741 CB the smallest power of two >= the layer's Cout in [32, BN], :760 FLAT `tpi BK 32 > HWo 33` and :781 AVEC
    `HWo % 4 == 0 && aligned16` on the layer's H W and X."""
    dx_wm = wm = 2 if g["Cin"] > 64 else 1                                # two rules, one threshold: the layer's Cin on both
    _, BN, BK = tile_cfg(wm)
    cb = 32
    while cb < g["Cout"] and cb < BN:
        cb *= 2
    hw = g["H"] * g["W"]
    return dict(dx_wm=dx_wm, dx_cvec=hw % 4 == 0 and aligned, wg=(wm, cb), flat=_ceil_div(hw, BK) * BK * 32 > hw * 33,
                avec=hw % 4 == 0 and aligned)


def tapless_pixels(g):
    """[Ho][Wo] bool: the output pixels of the stride phases no tap reaches (bias only), from phase_axis / phase_taps"""
    rstep, sstep = g["sh"] // _gcd(g["dh"], g["sh"]), g["sw"] // _gcd(g["dw"], g["sw"])
    mask = np.zeros((g["Ho"], g["Wo"]), bool)
    for py in range(g["sh"]):
        yf, nyq = phase_axis(py, g["pu"], g["sh"], g["Ho"])
        nr = phase_taps(py, g["dh"], g["sh"], rstep, g["kh"])[1]
        for px in range(g["sw"]):
            xf, nxq = phase_axis(px, g["pl"], g["sw"], g["Wo"])
            ns = phase_taps(px, g["dw"], g["sw"], sstep, g["kw"])[1]
            if nr * ns == 0 and nyq * nxq:
                mask[np.ix_(yf + g["sh"] * np.arange(nyq), xf + g["sw"] * np.arange(nxq))] = True
    return mask


def make_case(geom, seed):
    """Seeded X, W, b, dO for a geometry (float32) and its normalised description."""
    g = normalise(geom)
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (g["B"], g["Cin"], g["H"], g["W"])).astype(np.float32)
    sd = 1.0 / np.sqrt(g["Cin"] * g["kh"] * g["kw"])
    W = rng.uniform(-sd, sd, (g["Cout"], g["Cin"], g["kh"], g["kw"])).astype(np.float32)
    b = rng.uniform(-0.3, 0.3, g["Cout"]).astype(np.float32)
    dO = rng.uniform(-1, 1, (g["B"], g["Cout"], g["Ho"], g["Wo"])).astype(np.float32)
    return g, X, W, b, dO
