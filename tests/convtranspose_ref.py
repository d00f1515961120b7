"""ConvTranspose2d in float64, written from the closed form of the reference layer (neunet/nn/layers/convtranspose2d.py)
rather than from its as_strided code:

    O[b,o,y,x] = bias[o] + sum_{i,k,l} W[o,i,k,l] X[b,i,h,w]   with   h sh = y + pu - (kh-1-k) dh,   w sw = x + pl - (kw-1-l) dw
    Ho = (H-1) sh - (pu+pd) + dh (kh-1) + oph + 1    (likewise Wo)

i.e. input pixel h feeds output row y = h sh - pu + (kh-1-k) dh through tap k.  The weight is [out, in, kh, kw] and is NOT
flipped; this equals torch's conv_transpose2d with W.flip(2, 3).transpose(0, 1).  Shared by the CPU and the GPU tests."""
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


def forward(X, W, b, g):
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    O = np.zeros((g["B"], g["Cout"], g["Ho"], g["Wo"]))
    for k, l, src, dst in _taps(g):
        O[(slice(None), slice(None)) + dst] += np.einsum("oi,bihw->bohw", W[:, :, k, l], X[(slice(None), slice(None)) + src])
    if b is not None:
        O += np.asarray(b, np.float64).reshape(1, -1, 1, 1)
    return O


def backward(X, W, dO, g):
    """-> dX, dW, db"""
    X, W, dO = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(dO, np.float64)
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
