"""Float64 restatements of Conv2d (forward, backward, the fused conv -> LeakyReLU -> MaxPool2d(2, 2) chain and the pooled weight-gradient
chain), the sums of absolute products the rounding bounds need, the dispatch of csrc/conv2d.hip + csrc/conv_mfma.hip restated in Python
(route()), and the case table shared by tests/test_conv_ref.py (CPU), tests/test_conv_tiers_gpu.py and tests/conv_child.py.

The references are written from the formulas in the oracle/neunet_oracle.py docstrings -- a sum over the taps of shifted, strided slices
of the zero-padded input -- in float64, with a 4-sided padding; no im2col matrix is built.  NumPy only, independent of the oracle and of
the kernels: tests/test_conv_ref.py pins them to the oracle and to the reference's fixtures.

route() is a restatement, checked by review against the sources: every constant in it names the line of conv2d.hip / conv_mfma.hip it
restates.  It returns, per entry point, the kernel instantiation that runs and the launch plan the host computes."""
import zlib

import numpy as np

U24 = 2.0 ** -24
LDS_LIMIT = 60 * 1024            # conv2d.hip: `wg_lds <= 60 * 1024`, `m_lds <= 60 * 1024`
CD_MAXC, CD_MAXTAPS = 16, 25      # conv2d.hip


# ===================================================================================================== descriptor
class ConvDesc:
    """The fields of struct nnhipConv2dDesc (include/neunet_hip.h)."""
    FIELDS = ("B", "Cin", "H", "W", "Cout", "kh", "kw", "sh", "sw", "dh", "dw", "pu", "pd", "pl", "pr")

    def __init__(self, B, Cin, H, W, Cout, k, stride=1, pad=0, dil=1):
        pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)      # noqa: E731
        self.B, self.Cin, self.H, self.W, self.Cout = B, Cin, H, W, Cout
        self.kh, self.kw = pair(k)
        self.sh, self.sw = pair(stride)
        self.dh, self.dw = pair(dil)
        p = pair(pad)
        self.pu, self.pd, self.pl, self.pr = (p[0], p[0], p[1], p[1]) if len(p) == 2 else p

    def out_hw(self):
        """conv2d.py:245-258 (make_geom in conv2d.hip)."""
        return ((self.H + self.pu + self.pd - self.dh * (self.kh - 1) - 1) // self.sh + 1,
                (self.W + self.pl + self.pr - self.dw * (self.kw - 1) - 1) // self.sw + 1)

    def replace(self, **kw):
        d = ConvDesc.__new__(ConvDesc)
        d.__dict__.update(self.__dict__)
        d.__dict__.update(kw)
        return d

    def __repr__(self):
        return "ConvDesc(" + ", ".join(f"{k}={getattr(self, k)}" for k in self.FIELDS) + ")"


def make_inputs(name, d, bias=True):
    """X, dO uniform(-1, 1); W uniform(-1, 1) / sqrt(Cin kh kw); bias uniform(-0.3, 0.3); seeded by the case's name."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    Ho, Wo = d.out_hw()
    X = rng.uniform(-1, 1, (d.B, d.Cin, d.H, d.W)).astype(np.float32)
    Wt = (rng.uniform(-1, 1, (d.Cout, d.Cin, d.kh, d.kw)) / np.sqrt(d.Cin * d.kh * d.kw)).astype(np.float32)
    b = rng.uniform(-0.3, 0.3, d.Cout).astype(np.float32)
    dO = rng.uniform(-1, 1, (d.B, d.Cout, Ho, Wo)).astype(np.float32)
    return X, Wt, (b if bias else None), dO


# ===================================================================================================== float64 references
def _taps(d):
    Ho, Wo = d.out_hw()
    for r in range(d.kh):
        for s in range(d.kw):
            yield r, s, (slice(None), slice(None), slice(r * d.dh, r * d.dh + d.sh * (Ho - 1) + 1, d.sh),
                         slice(s * d.dw, s * d.dw + d.sw * (Wo - 1) + 1, d.sw))


def _padded(X, d):
    return np.pad(np.asarray(X, np.float64), ((0, 0), (0, 0), (d.pu, d.pd), (d.pl, d.pr)))


def conv2d_forward64(X, Wt, bias, d):
    """O[b, o, h, w] = sum_{i, r, s} Xpad[b, i, h sh + r dh, w sw + s dw] W[o, i, r, s] + bias[o], float64."""
    Xp, W64 = _padded(X, d), np.asarray(Wt, np.float64)
    Ho, Wo = d.out_hw()
    O = np.zeros((d.B, d.Cout, Ho, Wo))
    for r, s, sl in _taps(d):
        O += np.einsum("bihw,oi->bohw", Xp[sl], W64[:, :, r, s], optimize=True)
    if bias is not None:
        O += np.asarray(bias, np.float64)[None, :, None, None]
    return O


def conv2d_backward64(X, Wt, dO, d):
    """(dX, dW, db), float64:  dW[o, i, r, s] = sum_{b, h, w} Xpad[b, i, h sh + r dh, w sw + s dw] dO[b, o, h, w];  db[o] = sum dO;
    dX = the scatter of dO through the same taps, cropped to the un-padded input (input pixels no window covers stay 0)."""
    Xp, W64, g = _padded(X, d), np.asarray(Wt, np.float64), np.asarray(dO, np.float64)
    dXp, dW = np.zeros_like(Xp), np.zeros_like(W64)
    for r, s, sl in _taps(d):
        dW[:, :, r, s] = np.einsum("bihw,bohw->oi", Xp[sl], g, optimize=True)
        dXp[sl] += np.einsum("bohw,oi->bihw", g, W64[:, :, r, s], optimize=True)
    return np.ascontiguousarray(dXp[:, :, d.pu: d.pu + d.H, d.pl: d.pl + d.W]), dW, g.sum(axis=(0, 2, 3))


def forward_abs_sum(X, Wt, d):
    """sum |a||b| per forward output: |X| * |W| (no bias term: its addition is the bound's 4 x 2^-24 |ref|)."""
    return conv2d_forward64(np.abs(X), np.abs(Wt), None, d)


def dgrad_abs_sum(Wt, dO, d):
    """sum |a||b| per dX element: |dO| scattered through |W|."""
    return conv2d_backward64(np.zeros((d.B, d.Cin, d.H, d.W)), np.abs(Wt), np.abs(dO), d)[0]


def dot_rule(ref, abs_sum):
    """The bound of a float32 dot product against float64 (test_hip_parity.py:43-52, c = 32) + four roundings of the result."""
    return 32 * U24 * abs_sum + 4 * U24 * np.abs(ref) + 1e-30


def leaky64(v, alpha):
    a = np.float64(np.float32(alpha))
    return v if float(np.float32(alpha)) == 1.0 else np.where(v <= 0, a * v, v)


def conv_leaky_pool64(X, Wt, bias, alpha, d):
    """MaxPool2d(2, 2)(LeakyReLU(Conv2d(X); alpha)) in float64 (alpha = 1: no activation).  Returns (P, arg, V, Vbound): pooled values,
    the window-local arg-max in the kernel's r * kw + s convention (first maximum in row-major order), the activation's output V
    [B, Cout, Ho, Wo] and the forward bound of every V element (the conv's bound times alpha where the value is negative)."""
    conv = conv2d_forward64(X, Wt, bias, d)
    bound = dot_rule(conv, forward_abs_sum(X, Wt, d))
    a = float(np.float32(alpha))
    V = leaky64(conv, alpha)
    Vb = np.where(conv <= 0, a * bound, bound) + (0 if a == 1.0 else U24 * np.abs(V))
    B, C, Ho, Wo = V.shape
    win = V.reshape(B, C, Ho // 2, 2, Wo // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, Ho // 2, Wo // 2, 4)
    arg = np.argmax(win, axis=-1).astype(np.int32)            # first maximum; index = r * 2 + s
    return np.max(win, axis=-1), arg, V, Vb


def window_view(V, kh=2, kw=2):
    B, C, Ho, Wo = V.shape
    return V.reshape(B, C, Ho // kh, kh, Wo // kw, kw).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, Ho // kh, Wo // kw, kh * kw)


def near_ties(V, Vb):
    """Windows whose float64 top two values are closer than the sum of their two bounds: there a float32 kernel may pick either."""
    w, wb = window_view(V), window_view(Vb)
    order = np.argsort(-w, axis=-1, kind="stable")
    top = np.take_along_axis(w, order[..., :2], -1)
    tb = np.take_along_axis(wb, order[..., :2], -1)
    return (top[..., 0] - top[..., 1]) <= (tb[..., 0] + tb[..., 1])


def pooled_dO32(dP, arg, pooled, alpha, pool):
    """The dO the pooled weight-gradient chain implies, in the kernel's float32 arithmetic (one multiply, exact restatement):
    gg = pooled <= 0 ? dP * alpha : dP  (pooled = None: no activation), placed at the window's arg-max cell, 0 elsewhere."""
    kh, kw = pool
    dP = np.asarray(dP, np.float32)
    gg = dP if pooled is None else np.where(np.asarray(pooled) <= 0, dP * np.float32(alpha), dP).astype(np.float32)
    B, C, Hq, Wq = dP.shape
    dO = np.zeros((B, C, Hq * kh, Wq * kw), np.float32)
    for r in range(kh):
        for s in range(kw):
            dO[:, :, r::kh, s::kw] = np.where(arg == r * kw + s, gg, np.float32(0))
    return dO


def pooled_wgrad64(X, dP, arg, pooled, alpha, pool, d):
    """(dW, db, dO32) of the chain dP -> (arg-max, pooled sign) -> dO -> dW, db."""
    dO = pooled_dO32(dP, arg, pooled, alpha, pool)
    _, dW, db = conv2d_backward64(X, np.zeros((d.Cout, d.Cin, d.kh, d.kw)), dO, d)
    return dW, db, dO


def recip_div(p, div):
    """`(int)(((float)p + 0.5f) * (1.0f / (float)div))` of conv_mfma_wgrad_kernel, in NumPy float32."""
    inv = np.float32(1.0) / np.float32(div)
    return ((np.asarray(p).astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


# ===================================================================================================== dispatch, restated
DEFAULT = dict(quad=1, direct=1, wgrad_mfma=1, dgrad_quad2=1, tail_split=1, wgrad_flat=-1, minkt=4)
ENV = dict(quad="NNHIP_CONV_QUAD", direct="NNHIP_CONV_DIRECT", wgrad_mfma="NNHIP_CONV_WGRAD_MFMA", dgrad_quad2="NNHIP_CONV_DGRAD_QUAD2",
           tail_split="NNHIP_CONV_TAIL_SPLIT", wgrad_flat="NNHIP_CONV_WGRAD_FLAT", minkt="NNHIP_CONV_WGRAD_MINKT")
SETTINGS = {
    "nosplit": dict(quad=0, wgrad_mfma=0, tail_split=0, wgrad_flat=0),
    "igemm": dict(direct=0, wgrad_flat=1, minkt=1),
    "quad1": dict(dgrad_quad2=0),
}


def switches(setting=None):
    return dict(DEFAULT, **(SETTINGS[setting] if setting else {}))


def setting_env(setting):
    return {ENV[k]: str(v) for k, v in SETTINGS[setting].items()}


def cdiv(a, b):
    return -(-a // b)


def direct_ok(d, sw):
    """conv_direct_ok()."""
    Ho, Wo = d.out_hw()
    lim = 1 << 29
    return bool(sw["direct"]) and d.Cin <= CD_MAXC and d.Cout <= CD_MAXC and d.kh * d.kw <= CD_MAXTAPS and \
        d.B * d.Cin * d.H * d.W < lim and d.B * d.Cout * Ho * Wo < lim


def tap_plan(d, dgrad, sw, cus=256, dst_aligned=True):
    """launch_conv_tap<DGRAD>."""
    Ho, Wo = d.out_hw()
    M, Cs = (d.Cin, d.Cout) if dgrad else (d.Cout, d.Cin)
    Hd, Wd = (d.H, d.W) if dgrad else (Ho, Wo)
    wm = 2 if M > 64 else 1
    BM, BN, BK = 64 * wm, 256 // wm, 32 if wm == 2 else 16
    taps = d.kh * d.kw
    Mp, Csp = cdiv(M, BM) * BM, cdiv(Cs, BK) * BK
    N = d.B * Hd * Wd
    tiles_m, tiles_n = Mp // BM, cdiv(N, BN)
    slots = cus * (2 if wm == 2 else 3)
    T = taps * (Csp // BK)
    tn_main = (((tiles_n * tiles_m) // slots) * slots) // tiles_m
    tail = tiles_n - tn_main
    splits, ktps = 1, T
    if sw["tail_split"] and tail > 0:
        best = 1e30
        for sp in range(1, min(16, T // 3 if T >= 3 else 1) + 1):
            k = cdiv(T, sp)
            se = cdiv(T, k)
            cost = float(cdiv(tail * tiles_m * se, slots)) * (k + 1.5)
            if cost < best - 1e-9:
                best, splits, ktps = cost, se, k
    if splits <= 1:
        tn_main, tail, splits, ktps = tiles_n, 0, 1, T
    side = "dgrad" if dgrad else "fwd"
    aux = ["conv_repack_kernel"] + (["conv_tap_reduce_kernel"] if tail > 0 else [])
    return dict(kernel=f"conv_tap_kernel<{side},{wm}>", aux=aux, wm=wm, BM=BM, BN=BN, BK=BK, M=M, Cs=Cs, Mp=Mp, Csp=Csp, tiles_m=tiles_m,
                tiles=tiles_n, tn_main=tn_main, tail=tail, splits=splits, ktps=ktps, T=T, cvec=int((Hd * Wd) % 4 == 0 and dst_aligned))


def mfma_wgrad_plan(d, sw):
    """mfma_wgrad_plan(): (ok, ncols, nt, nt_inst, m_lds)."""
    Ho, Wo = d.out_hw()
    ncols = d.Cin * 9 + 1
    nt = cdiv(ncols, 16)
    nt_inst = nt if nt <= 3 else 5 if nt <= 5 else 10
    Hp, Wp = (Ho - 1) * d.sh + 2 * d.dh + 1, (Wo - 1) * d.sw + 2 * d.dw + 1
    Lg = 4 * cdiv(Ho * Wo, 4)
    m_lds = max((d.Cin * Hp * Wp + 4 + d.Cout * Lg) * 4, 4 * 16 * 16 * nt_inst * 4)
    ok = bool(sw["wgrad_mfma"]) and direct_ok(d, sw) and d.kh == 3 and d.kw == 3 and nt <= 10 and m_lds <= LDS_LIMIT
    return ok, ncols, nt, nt_inst, m_lds


def igemm_wgrad_plan(d, sw, want_dw=True, do_aligned=True):
    """conv_mfma_wgrad()."""
    Ho, Wo = d.out_hw()
    HWo = Ho * Wo
    wm = 2 if d.Cout > 64 else 1
    BM, BN, BK = 64 * wm, 256 // wm, 32 if wm == 2 else 16
    CB = 32
    while CB < d.Cin and CB < BN:
        CB *= 2
    TPT, taps = BN // CB, d.kh * d.kw
    cblks, tgroups = cdiv(d.Cin, CB), cdiv(taps, TPT)
    tiles_m = cdiv(d.Cout, BM)
    tpi = cdiv(HWo, BK)
    flat = (sw["wgrad_flat"] != 0) if sw["wgrad_flat"] >= 0 else tpi * BK * 32 > HWo * 33
    ktiles = cdiv(d.B * HWo, BK) if flat else d.B * tpi
    chunks = max(512 // (tiles_m * tgroups * cblks), 1)
    chunks = min(chunks, cdiv(ktiles, max(sw["minkt"], 1)))
    tpc = cdiv(ktiles, chunks)
    chunks = cdiv(ktiles, tpc)
    avec = HWo % 4 == 0 and do_aligned
    b = lambda v: "true" if v else "false"                                  # noqa: E731
    return dict(kernel=f"conv_wgrad_mfma_kernel<{wm},{CB},{b(avec)},{b(flat)}>", aux=["conv_wgrad_mfma_reduce_kernel"], wm=wm, CB=CB, TPT=TPT,
                tgroups=tgroups, cblks=cblks, tiles_n=tgroups * cblks if want_dw else 1, flat=flat, avec=avec, chunks=chunks, tpc=tpc,
                ktiles=ktiles)


def pool_fwd_ok(d, pool, sw):
    """conv_pool_fwd_ok(): 'window', 'quad' or None.  pool: a tests/vision_ref.PoolDesc or None."""
    Ho, Wo = d.out_hw()
    p = pool
    if not (p is not None and p.kh == 2 and p.kw == 2 and p.sh == 2 and p.sw == 2 and p.pu + p.pd + p.pl + p.pr == 0 and p.dh <= 1 and
            p.dw <= 1 and (p.B, p.C, p.H, p.W) == (d.B, d.Cout, Ho, Wo) and Ho % 2 == 0 and Wo % 2 == 0 and direct_ok(d, sw) and
            d.kh == 3 and d.kw == 3):
        return None
    unit = d.sh == 1 and d.sw == 1 and d.dh == 1 and d.dw == 1
    if unit and d.Cout > 4 and d.Cin <= 4 and d.B * (Ho // 2) * (Wo // 2) >= 128 * 256:       # conv_pool_window_ok
        return "window"
    if sw["quad"] and d.B * Ho * Wo <= 512 * 256 and d.Cin >= 4 and d.Cout > 4 and unit:      # conv_pool_quad_ok
        return "quad"
    return None


def stats_blocks(d, pool, sw):
    """nnhipConv2dLeakyMaxPoolStatsBlocks()."""
    if pool_fwd_ok(d, pool, sw) != "quad":
        return 0
    Ho, Wo = d.out_hw()
    N = d.B * (Ho // 2) * (Wo // 2)
    return N // 64 if N % 64 == 0 and N // 64 <= 65535 else 0


def pooled_wgrad_ok(d, pool, sw):
    """pooled_wgrad_ok()."""
    Ho, Wo = d.out_hw()
    p = pool
    return p is not None and p.kh == p.sh and p.kw == p.sw and p.pu + p.pd + p.pl + p.pr == 0 and p.dh <= 1 and p.dw <= 1 and p.kh >= 1 and \
        p.kw >= 1 and p.kh * p.kw <= 16 and (p.B, p.C, p.H, p.W) == (d.B, d.Cout, Ho, Wo) and Ho % p.kh == 0 and Wo % p.kw == 0 and \
        mfma_wgrad_plan(d, sw)[0]


def route(d, sw=None, cus=256, pool=None, stats=False, aligned=True):
    """Which kernels nnhipConv2dForward / nnhipConv2dBackward (and, with `pool`, the fused entries) launch for descriptor d under the
    developer switches sw on a chip of `cus` compute units.  aligned: the output / dO pointers are 16-byte aligned."""
    sw = dict(DEFAULT, **(sw or {}))
    Ho, Wo = d.out_hw()
    k33 = d.kh == 3 and d.kw == 3
    direct = direct_ok(d, sw)
    out = {}
    # ---- nnhipConv2dForward
    N = d.B * Ho * Wo
    if direct:
        if sw["quad"] and k33 and N <= 512 * 256 and d.Cin >= 4 and d.Cout > 4:
            out["fwd"] = dict(kernel=f"conv_direct_fwd_quad_kernel<{8 if d.Cout <= 8 else 16}>", aux=[])
        else:
            out["fwd"] = dict(kernel=f"conv_direct_fwd_kernel<{4 if d.Cout <= 4 else 8 if d.Cout <= 8 else 16}>", aux=[],
                              path="3x3 buffer" if k33 else "generic")
    else:
        out["fwd"] = tap_plan(d, False, sw, cus, aligned)
    # ---- nnhipConv2dBackward: dX
    Nd = d.B * d.H * d.W
    if direct:
        if sw["quad"] and k33 and Nd <= 512 * 256 and d.Cout >= 4 and 2 < d.Cin <= 8:
            unit = d.sh == 1 and d.sw == 1 and d.dh == 1 and d.dw == 1
            which = "quad2" if sw["dgrad_quad2"] and unit else "quad"
            out["dgrad"] = dict(kernel=f"conv_direct_dgrad_{which}_kernel<{4 if d.Cin <= 4 else 8}>", aux=[])
        else:
            out["dgrad"] = dict(kernel=f"conv_direct_dgrad_kernel<{4 if d.Cin <= 4 else 8 if d.Cin <= 8 else 16}>", aux=[],
                                path="3x3 buffer" if k33 else "generic")
    else:
        out["dgrad"] = tap_plan(d, True, sw, cus, aligned)
    # ---- nnhipConv2dBackward: dW, db
    wg_lds = (d.Cin * d.H * d.W + d.Cout * Ho * Wo) * 4
    ok, ncols, nt, nt_inst, m_lds = mfma_wgrad_plan(d, sw)
    if direct and k33 and wg_lds <= LDS_LIMIT:
        if ok:
            out["wgrad"] = dict(kernel=f"conv_mfma_wgrad_kernel<{nt_inst},false>", aux=["conv_wgrad_reduce_kernel"], ncols=ncols, nt=nt,
                                nt_inst=nt_inst, m_lds=m_lds, wg_lds=wg_lds)
        else:
            cip = 1 if d.Cin <= 1 else 2 if d.Cin <= 2 else 4 if d.Cin <= 4 else 8 if d.Cin <= 8 else 16
            out["wgrad"] = dict(kernel=f"conv_direct_wgrad_kernel<{8 if d.Cout <= 8 else 16},{cip}>", aux=["conv_wgrad_reduce_kernel"],
                                ncols=ncols, m_lds=m_lds, wg_lds=wg_lds)
    else:
        out["wgrad"] = dict(igemm_wgrad_plan(d, sw, True, aligned), wg_lds=wg_lds, m_lds=m_lds)
    # ---- the fused entries
    if pool is not None:
        kind = pool_fwd_ok(d, pool, sw)
        co = 8 if d.Cout <= 8 else 16
        if kind == "window":
            out["pool_fwd"] = dict(kernel=f"conv_pool_fwd_kernel<{co}>", aux=[])
        elif kind == "quad":
            st = bool(stats) and stats_blocks(d, pool, sw) > 0
            out["pool_fwd"] = dict(kernel=f"conv_pool_fwd_quad_kernel<{co},{'true' if st else 'false'}>", aux=[],
                                   stats_blocks=stats_blocks(d, pool, sw))
        else:
            out["pool_fwd"] = None
        if pooled_wgrad_ok(d, pool, sw):
            out["pool_wgrad"] = dict(kernel=f"conv_mfma_wgrad_kernel<{nt_inst},true>", aux=["conv_wgrad_reduce_kernel"], nt=nt, nt_inst=nt_inst,
                                     m_lds=m_lds, fast2x2=pool.kh == 2 and pool.kw == 2 and ((d.Cin * ((Ho - 1) * d.sh + 2 * d.dh + 1) *
                                                                                             ((Wo - 1) * d.sw + 2 * d.dw + 1)) | Wo) & 1 == 0)
        else:
            out["pool_wgrad"] = None
    return out


def kernels_of(r):
    """Every kernel name a route() result launches."""
    names = set()
    for v in r.values():
        if v:
            names.add(v["kernel"])
            names.update(v["aux"])
    return names


# ===================================================================================================== the case table
class Case:
    def __init__(self, name, desc, why, child=True, big=False):
        self.name, self.desc, self.why, self.child, self.big = name, desc, why, child, big

    def __repr__(self):
        return f"Case({self.name}: {self.desc})"


def _c(name, why, *a, child=True, big=False, **kw):
    return Case(name, ConvDesc(*a, **kw), why, child, big)


ASYM = (0, 2, 3, 1)       # pu, pd, pl, pr
NT_CIN, NT_COUT = (1, 3, 5, 6, 8, 9, 16), (1, 7, 16)
WG_CIN, WG_COUT = (17, 33, 65, 129), (24, 65)
WG_MAPS = {"2x2": (2, 2), "3x3": (3, 3), "8x8": (8, 8), "7x9": (7, 9)}


def _table():
    t = [
        _c("big_fwd_c11", "conv_direct_fwd_kernel<8> buffer path, channel groups 8 + 3; dgrad direct <16>; igemm wgrad CB = 32, K = 133128",
           2, 11, 258, 258, 6, 3, pad=1, child=False, big=True),
        _c("big_dgrad_c5", "conv_direct_dgrad_kernel<8> at 3x3 above 131072 positions", 2, 5, 258, 258, 6, 3, pad=1, child=False, big=True),
        _c("tile64_main_tail", "launch_conv_tap at wm = 1 with tn_main > 0: 781 pixel tiles = 768 whole + 13 split, fwd and dgrad",
           3, 17, 258, 258, 20, 3, pad=1, child=False, big=True),
        _c("dwg_c16", "conv_direct_wgrad_kernel<8,16> by default: wg_lds 56784 <= 61440 < m_lds 63712", 3, 16, 26, 26, 5, 3, pad=1),
        _c("dwg_c16_o6", "conv_direct_wgrad_kernel<8,16>: the last Cout whose un-padded image fits (wg_lds 59488)", 3, 16, 26, 26, 6, 3, pad=1),
        _c("dwg_c16_o4", "one channel fewer: m_lds 61008 fits, conv_mfma_wgrad_kernel<10>", 3, 16, 26, 26, 4, 3, pad=1),
        _c("dwg_c16_o7", "one channel more: wg_lds 62192 > 61440, small channels in conv_wgrad_mfma_kernel", 3, 16, 26, 26, 7, 3, pad=1),
        _c("dwg_c1", "conv_direct_wgrad_kernel<8,1>: 7569 pixels per image, wg_lds 60552, m_lds 61988", 2, 1, 87, 87, 1, 3, pad=1),
        _c("dwg_c1_86", "86 x 86: m_lds 60576 fits, conv_mfma_wgrad_kernel<1> at its largest image", 2, 1, 86, 86, 1, 3, pad=1),
        _c("dwg_c1_88", "88 x 88: wg_lds 61952 > 61440, one channel in conv_wgrad_mfma_kernel", 2, 1, 88, 88, 1, 3, pad=1),
        _c("igemm_c16_32", "16 channels at 32 x 32: the weight gradient of a small-channel layer in conv_wgrad_mfma_kernel (wg_lds 131072)",
           2, 16, 32, 32, 16, 3, pad=1),
        _c("taps49_c3", "> 25 taps: conv_tap_kernel<.,1> with Cs = 3 of a 16-deep tile, M = 8 of 64; wgrad CB = 32, 49 taps",
           2, 3, 20, 20, 8, 7, stride=2, pad=3),
        _c("taps26_c2", "26 taps (2 x 13), pad (0, 6): the first tap count past conv_direct_ok", 1, 2, 9, 30, 5, (2, 13), pad=(0, 6)),
        _c("taps25_c3", "25 taps (5 x 5): the last tap count of the direct kernels, generic loop", 2, 3, 9, 9, 4, 5, pad=2),
        _c("lim_c16_o16", "Cin = Cout = 16: the last direct layer", 2, 16, 6, 7, 16, 3, pad=1),
        _c("lim_c17_o16", "Cin = 17: implicit GEMM", 2, 17, 6, 7, 16, 3, pad=1),
        _c("lim_c16_o17", "Cout = 17: implicit GEMM", 2, 16, 6, 7, 17, 3, pad=1),
        _c("nt_c2_o16", "Cin = 2: NT = 2 with nt = 2; conv_direct_wgrad_kernel<16,2> with the MFMA kernel off", 3, 2, 7, 9, 16, 3, pad=1),
        _c("quad_s2", "stride 2: conv_direct_dgrad_quad_kernel<4>'s division path (not quad2)", 2, 4, 9, 11, 8, 3, stride=2, pad=1),
        _c("quad_d2", "dilation 2: conv_direct_dgrad_quad_kernel<8> at unit stride (not quad2)", 2, 8, 9, 11, 8, 3, pad=2, dil=2),
        _c("c200_o24", "Cin = 200: CB = 256 with 56 padded channels", 2, 200, 5, 6, 24, 3, pad=1),
        _c("c200_o65", "Cin = 200, Cout = 65: CB = 128, two channel blocks", 2, 200, 5, 6, 65, 3, pad=1),
        _c("asym_direct", "pad (0, 2, 3, 1) on the direct kernels: pd / pr only through Ho / Wo", 2, 2, 8, 9, 3, 3, pad=ASYM),
        _c("asym_quad", "pad (0, 2, 3, 1) on the quad kernels and conv_mfma_wgrad_kernel", 2, 8, 8, 9, 8, 3, pad=ASYM),
        _c("asym_igemm", "pad (0, 2, 3, 1) on the implicit-GEMM kernels", 2, 20, 8, 9, 24, 3, pad=ASYM),
        _c("asym_igemm_s2", "pad (0, 2, 3, 1), stride 2, 4 x 3 taps on the implicit-GEMM kernels", 2, 20, 9, 8, 24, (4, 3), stride=2, pad=ASYM),
    ]
    for ci in NT_CIN:
        for co in NT_COUT:
            t.append(_c(f"nt_c{ci}_o{co}", "every nt_inst of conv_mfma_wgrad_kernel at 7 x 9 (63 pixels: zero-padded Lg step, columns past Nw); "
                        "both sides of the quad / quad2 conditions; a ragged last quad (189 positions)", 3, ci, 7, 9, co, 3, pad=1))
    for ci, co in ((3, 5), (4, 4), (4, 5), (9, 5)):                        # (8, 16) is nt_c8_o16
        t.append(_c(f"quad_c{ci}_o{co}", "3 x 3 on either side of Cin >= 4, Cout > 4 (fwd) and Cout >= 4, 2 < Cin <= 8 (dgrad)", 3, ci, 7, 9, co, 3,
                    pad=1))
    for ci in WG_CIN:
        for co in WG_COUT:
            for tag, (h, w) in WG_MAPS.items():
                t.append(_c(f"wg_c{ci}_o{co}_{tag}", "launch_wgrad_cfg<WM, CB> x avec x flat: 2 x 2 (flat, avec), 3 x 3 (flat), 8 x 8 (avec), "
                            "7 x 9 (neither)", 3, ci, h, w, co, 3, pad=1, child=tag in ("2x2", "8x8")))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def child_cases():
    """What tests/conv_child.py runs under each switch setting: the small cases (nothing at 258 x 258)."""
    return [c for c in CASES if c.child]


# ---- the fused entries' cases: (name, desc, alpha list, why)
POOL_FWD_CASES = [
    ("pf_window8", ConvDesc(170, 1, 28, 28, 8, 3, pad=1), "conv_pool_fwd_kernel<8>: 33320 windows >= 32768, Cin = 1"),
    ("pf_window16", ConvDesc(170, 2, 28, 28, 12, 3, pad=1), "conv_pool_fwd_kernel<16>"),
    ("pf_quad16", ConvDesc(16, 8, 14, 14, 16, 3, pad=1), "conv_pool_fwd_quad_kernel<16,false>: C5's second layer at batch 16"),
    ("pf_quad8_ragged", ConvDesc(3, 5, 10, 14, 7, 3, pad=1), "conv_pool_fwd_quad_kernel<8,false>: 105 windows, Cin = 5 (lanes past Cin)"),
    ("pf_quad16_pad2", ConvDesc(2, 16, 6, 6, 12, 3, pad=2), "conv_pool_fwd_quad_kernel<16,false>: pad 2, 8 x 8 conv output"),
]
POOL_STATS_CASES = [
    ("ps_quad16", ConvDesc(4, 8, 8, 8, 16, 3, pad=1), "conv_pool_fwd_quad_kernel<16,true>: one block of 64 windows"),
    ("ps_quad8", ConvDesc(8, 4, 8, 8, 6, 3, pad=1), "conv_pool_fwd_quad_kernel<8,true>: two blocks"),
]
# (name, desc, pool window, why): Cin 1, 3, 5, 8, 16 -> NT 1, 2, 3, 5, 10 of conv_mfma_wgrad_kernel<NT, true>
POOL_WGRAD_CASES = [
    ("pw_c1_22_even", ConvDesc(3, 1, 12, 12, 8, 3, pad=1), (2, 2), "NT = 1; nXp = 196 even, Wo even: the float2 fast path"),
    ("pw_c3_22_even", ConvDesc(3, 3, 10, 12, 7, 3, pad=(2, 1)), (2, 2), "NT = 2; pad (2, 1): a 12 x 12 conv output, fast path"),
    ("pw_c5_32", ConvDesc(2, 5, 9, 10, 6, 3, pad=(1, 1, 1, 1)), (3, 2), "NT = 3; (3, 2) windows on a 9 x 10 map: the general path"),
    ("pw_c3_22_oddnxp", ConvDesc(3, 3, 16, 16, 7, 3, stride=2, pad=1), (2, 2), "NT = 2; stride 2: Hp = Wp = 17, nXp = 867 odd -> 2 x 2 windows on the "
     "general path (Gs would not be 8-byte aligned)"),
    ("pw_c8_23", ConvDesc(2, 8, 8, 9, 16, 3, pad=1), (2, 3), "NT = 5; (2, 3) windows"),
    ("pw_c16_33", ConvDesc(2, 16, 9, 9, 12, 3, pad=1), (3, 3), "NT = 10; (3, 3) windows"),
    ("pw_c3_11", ConvDesc(2, 3, 6, 7, 4, 3, pad=1), (1, 1), "(1, 1) windows: arg-max always 0, dO = the LeakyReLU backward of dP"),
]
