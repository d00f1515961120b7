"""CPU: the float64 restatements of tests/gemm_ref.py against what the project already trusts -- the reference's Linear and Linear-Swish
fixtures under tests/golden/ and oracle/neunet_oracle.py -- each also shown to REJECT four wrong variants of its rules; and gemm_route
pinned on both sides of every dispatch threshold of csrc/gemm.hip, gemm_small.hip and gemm_pst.hip.

This file also holds the case tables of tests/test_gemm_tiers_gpu.py and tests/test_gemm_small_pst_gpu.py.  Every case names the
branches it is there for (`tags`); BRANCHES maps each branch to a predicate on the case's ROUTE (gemm_route of its shape, layout,
alignment and epilogue), and test_tables_cover_branches asserts that every tag's predicate holds for its case and that the tags of the
tables are exactly BRANCHES -- a case that silently moves to another kernel after a dispatcher change fails here, without a GPU.

Shapes: {M, N} from {4, 100, 128, 132, 264, 1032, 1100} (1, 3 and 9 tile rows: a last row group of fewer than 8, grids that are not
multiples of 8; split-K makes the multiples: 27 tiles x 8 splits), with 1030 / 130 / 262 where an extent must NOT be a multiple of 4.
A lone matrix must not fit gemm_small: 264 x 1032 has 27 tiles of 128 (more than 8) -- but only 297 tiles of 32, so K <= 64 runs as a
batch of two -- or K > 2048, or batch > 1.

Two things the dispatcher cannot do with its default constants, found while pinning it (and therefore without a GPU case):
  * the split-K bail-out `few && K < 1024 && s < 4` never fires: few means tiles <= 64 and K >= 256, so 512 / tiles >= 8 and K / 64 >= 4
    (test_splitk_bailout_is_unreachable walks the whole range);
  * `tiles32 <= 256` in gemm_small_wanted is implied by `tiles128 <= 8` (a 128-tile holds at most 16 32-tiles: 128 at the most).
splitk = 2 needs 512 / tiles = 2, i.e. exactly 171..191 tiles (170 tiles give three splits, 128 give four), and K >= 1024: the tile
limit's own pair, 191 | 192 tile rows of one tile column, supplies it -- 24448 x 128 (x 126 for the scalar reduce) at K = 1024 is two slabs
on a classic grid of 191 x 2 blocks whose last row group has 7 tile rows; 24576 x 128 is the unsplit neighbour; at K = 512 neither splits."""
import numpy as np
import pytest

from gemm_ref import (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SWISH, ACT_SWISH_D, asum64, ceil_div, epilogue64, gemm64, gemm_route, group_launches,
                      operand, pair_instance, pair_route, route_id, small_wanted, wgrad_route)
from oracle import neunet_oracle as O

TOL = dict(rtol=1e-5, atol=1e-6)          # tests/test_oracle_golden.py's, for the same fixtures
GTOL = dict(rtol=1e-5, atol=1e-5)


# ==================================================================================================== the Linear entries as GEMMs
# op -> (layout, C entry, epilogue): what linear.hip turns each public entry into.  (M, N, K) is the GEMM's shape:
#   kk  forward        O[rows, out] = X[rows, in] W[out, in]^T       M = rows, N = out, K = in
#   ko  input gradient dX[rows, in] = dO[rows, out] W[out, in]       M = rows, N = in,  K = out
#   oo  weight grad.   dW[out, in] = dO[rows, out]^T X[rows, in]     M = out,  N = in,  K = rows   (+ asum = db)
LIN_OPS = {
    "fwd": ("kk", dict(bias=1)),
    "fwd_add": ("kk", dict(bias=1, addend=1)),
    "act1": ("kk", dict(bias=1, act=ACT_SWISH)),
    "act2": ("kk", dict(bias=1, act=ACT_RELU)),
    "act3": ("kk", dict(bias=1, act=ACT_SIGMOID)),
    "swish_z": ("kk", dict(bias=1, act=ACT_SWISH, preact=1)),
    "swish_d": ("kk", dict(bias=1, act=ACT_SWISH_D, preact=1)),
    "dx": ("ko", dict()),
    "dx_add": ("ko", dict(addend=1)),
    "dx_d1": ("ko", dict(dact=1)),
    "dx_d1_ip": ("ko", dict(dact=1)),        # in place over z
    "dx_d2": ("ko", dict(dact=2)),
    "dx_d3": ("ko", dict(dact=3)),
    "dx_d3_ip": ("ko", dict(dact=3)),        # in place over the saved derivative
    "dw": ("oo", dict(asum=1)),
    "dw_nodb": ("oo", dict()),
}
BETA = 1.3                                 # of every Swish case


def lin_route(op, M, N, K, off=None, mode=0, slots=512):
    lay, epi = LIN_OPS[op]
    akm, bkm = lay[0] == "k", lay[1] == "k"
    return gemm_route(M, N, K, K if akm else M, K if bkm else N, N, akm, bkm, off=off, epi=epi, mode=mode, slots=slots)


def lin_inputs(op, M, N, K, seed=0):
    """a [M, K], b [N, K] (logical: C = a b^T), and the epilogue operands of `op`, all float32; variance-preserving b."""
    rng = np.random.default_rng(1000003 * seed + 7919 * M + 104729 * N + K)
    d = dict(a=rng.standard_normal((M, K)).astype(np.float32), b=(rng.standard_normal((N, K)) / np.sqrt(max(K, 1))).astype(np.float32))
    epi = LIN_OPS[op][1]
    if epi.get("bias"):
        d["bias"] = rng.standard_normal(N).astype(np.float32)
    if epi.get("addend"):
        d["addend"] = rng.standard_normal((M, N)).astype(np.float32)
    if epi.get("dact"):
        x = (rng.standard_normal((M, N)) * 2).astype(np.float32)
        d["dact"] = np.maximum(x, 0) if epi["dact"] == 2 else x     # dact 2 takes the forward OUTPUT of a ReLU
    return d


def lin_reference(op, d):
    """(C, preact, asum) in float64 and the dot bound's sum |a||b|, from lin_inputs' dict."""
    epi = LIN_OPS[op][1]
    a, b = d["a"].astype(np.float64), d["b"].astype(np.float64)
    v = a @ b.T
    if "bias" in d:
        v = v + d["bias"].astype(np.float64)
    c, pre = epilogue64(v, d.get("addend"), epi.get("dact", 0), d.get("dact"), epi.get("act", ACT_NONE), BETA)
    return c, pre, (a.sum(1) if epi.get("asum") else None), np.abs(a) @ np.abs(b).T, v


# ==================================================================================================== case tables
def G(M, N, K, lay, tags, pad=(0, 0, 0), batch=(1, 1), off=None, alpha=1.0, bias=True, share_b=False, odd=None, entry="ex"):
    """A call of the general entries.  pad: floats added to the dense lda / ldb / ldc; batch = (batch1, batch2); off: floats past a
    16-byte boundary per operand; odd: the operand ('A' or 'C') whose batch strides are NOT multiples of 4; entry 'f32': nnhipGemmF32
    (one batch level, alpha 1), 'ex': nnhipGemmF32Ex."""
    return dict(M=M, N=N, K=K, lay=lay, tags=list(tags), pad=pad, batch=batch, off=dict(off or {}), alpha=alpha, bias=bias, share_b=share_b,
                odd=odd, entry=entry)


def gen_geometry(c):
    """Leading dimensions, extents and batch strides of a general case: operands of one batch index lie `extent rounded to 4, + 4` apart
    (+ 1 for the `odd` operand), the outer level 8 floats further -- independent strides, gaps the kernel must not write."""
    M, N, K = c["M"], c["N"], c["K"]
    akm, bkm = c["lay"][0] == "k", c["lay"][1] == "k"
    lda, ldb, ldc = (K if akm else M) + c["pad"][0], (K if bkm else N) + c["pad"][1], N + c["pad"][2]
    ext = dict(A=((M - 1) * lda + K if akm else (K - 1) * lda + M) if M and K else 0,
               B=((N - 1) * ldb + K if bkm else (K - 1) * ldb + N) if N and K else 0, C=(M - 1) * ldc + N if M else 0)
    b1, b2 = c["batch"]
    st, size = {}, {}
    for name in "ABC":
        s2 = ceil_div(ext[name], 4) * 4 + 4 + (1 if c["odd"] == name else 0)
        s1 = b2 * s2 + 8
        if name == "B" and c["share_b"]:
            s1 = s2 = 0
        st[name] = (s1 if b1 > 1 else 0, s2 if b2 > 1 else 0)
        size[name] = (b1 - 1) * st[name][0] + (b2 - 1) * st[name][1] + ext[name]
    if c["pad"][2]:
        size["C"] += c["pad"][2]          # the padding columns of the last row belong to the allocation too (and stay NaN)
    return dict(akm=akm, bkm=bkm, lda=lda, ldb=ldb, ldc=ldc, st=st, size=size)


def gen_route(c, mode=0, slots=512, **change):
    c = dict(c, **change)
    g = gen_geometry(c)
    return gemm_route(c["M"], c["N"], c["K"], g["lda"], g["ldb"], g["ldc"], g["akm"], g["bkm"], c["batch"][0], c["batch"][1],
                      (g["st"]["A"], g["st"]["B"], g["st"]["C"]), c["off"], dict(bias=c["bias"], alpha=c["alpha"]), mode, slots)


def gen_inputs(c):
    g = gen_geometry(c)
    rng = np.random.default_rng(c["M"] * 31 + c["N"] * 17 + c["K"] + 1000 * sum(c["pad"]) + 7 * c["batch"][0])
    A = rng.standard_normal(max(g["size"]["A"], 1)).astype(np.float32)
    B = (rng.standard_normal(max(g["size"]["B"], 1)) / np.sqrt(max(c["K"], 1))).astype(np.float32)
    bias = rng.standard_normal(c["N"]).astype(np.float32) if c["bias"] else None
    return A, B, bias


def gen_reference(c, A, B, bias):
    g = gen_geometry(c)
    kw = dict(batch1=c["batch"][0], batch2=c["batch"][1], sA=g["st"]["A"], sB=g["st"]["B"], sC=g["st"]["C"], c_size=g["size"]["C"])
    args = (A, B, c["M"], c["N"], c["K"], g["lda"], g["ldb"], g["ldc"], g["akm"], g["bkm"], c["alpha"])
    return gemm64(*args, bias=bias, **kw), gemm64(*args, absolute=True, **kw)


def L(op, M, N, K, tags, off=None):
    return dict(op=op, M=M, N=N, K=K, tags=list(tags), off=dict(off or {}))


def gen_id(c):
    return f"{c['M']}x{c['N']}x{c['K']}-{route_id(gen_route(c))}-{'+'.join(c['tags'])}"


def lin_id(c):
    return f"{c['op']}-{c['M']}x{c['N']}x{c['K']}-{route_id(lin_route(c['op'], c['M'], c['N'], c['K'], c['off']))}-{'+'.join(c['tags'])}"


def _kb(K):
    return (2, 1) if K <= 64 else (1, 1)


KSWEEP = (8, 24, 32, 36, 40, 64, 72, 96, 104, 136)
LAYOUTS = ("kk", "ko", "ok", "oo")
BIG = (264, 1032)                        # 3 x 9 = 27 tiles: too many for gemm_small, few enough for split-K from K = 256

# ---- classic kernel, no split: the general entries
CLASSIC_GEN = (
    # 4 layouts x {vec, scalar}: K = 72 is two whole k-tiles and an 8-wide tail; K = 76 is not a multiple of 8
    [G(*BIG, 72, lay, [f"classic-{lay}-vec"], entry="f32") for lay in LAYOUTS] +
    [G(*BIG, 76, lay, [f"classic-{lay}-scalar"], entry="f32") for lay in LAYOUTS] +
    # the K sweep: 0..4 whole k-tiles with and without a tail, K < 32, K % 8 != 0; nine tile rows in the second layout (gsz = 1 in the last group)
    # (K <= 64 with at most 512 tiles of 32 x 32 -- 264 x 1032 has 297 -- belongs to gemm_small: those K run as a batch of two)
    [G(*BIG, K, "kk", [f"classic-K{K}"], batch=_kb(K), entry="f32") for K in KSWEEP] +
    [G(1032, 264, K, "oo", [f"classic-K{K}", "tiles_m9"], batch=_kb(K), entry="f32") for K in KSWEEP] +
    # vec off, one switch at a time
    [G(*BIG, 72, "kk", ["vecoff-A-4B"], off=dict(A=1)), G(*BIG, 72, "oo", ["vecoff-B-4B"], off=dict(B=1)),
     G(*BIG, 72, "kk", ["vecoff-ld"], pad=(1, 0, 0)), G(*BIG, 72, "ok", ["vecoff-ld"], pad=(0, 1, 0)),
     G(262, 1032, 72, "ok", ["vecoff-outer"]), G(264, 1030, 72, "oo", ["vecoff-outer"]),
     G(100, 132, 72, "kk", ["vecoff-stride"], batch=(2, 1), odd="A", entry="f32")] +
    # cvec off, one switch at a time (the loads stay vectorised): N % 4 (k-major B: its rows are still aligned), ldc, C, bias, sC
    [G(264, 1030, 72, "kk", ["cvecoff-N"]), G(*BIG, 72, "kk", ["cvecoff-ldc"], pad=(0, 0, 1)), G(*BIG, 72, "kk", ["cvecoff-C-4B"], off=dict(C=1)),
     G(*BIG, 72, "kk", ["cvecoff-bias-4B"], off=dict(bias=1)), G(100, 132, 72, "kk", ["cvecoff-stride"], batch=(2, 1), odd="C", entry="f32")] +
    # padded leading dimensions (multiples of 4: the float4 paths stay on), batches, a shared B, alpha
    [G(*BIG, 72, lay, ["padded-ld"], pad=(4, 8, 12)) for lay in ("kk", "oo")] + [G(*BIG, 76, "ko", ["padded-ld"], pad=(3, 5, 7))] +
    [G(100, 132, 72, lay, ["batch2x3"], batch=(2, 3)) for lay in ("kk", "oo")] + [G(100, 132, 36, "ko", ["batch2x3"], batch=(2, 3), pad=(0, 0, 4))] +
    [G(100, 132, 72, "kk", ["shared-B"], batch=(2, 3), share_b=True), G(4, 100, 40, "ok", ["shared-B"], batch=(3, 1), share_b=True, entry="f32")] +
    [G(*BIG, 72, "kk", ["alpha"], alpha=0.125), G(*BIG, 76, "oo", ["alpha"], alpha=-3.0), G(1100, 1100, 72, "ko", ["alpha", "tiles81"], alpha=-3.0),
     G(*BIG, 72, "ok", ["no-bias"], bias=False)])

# ---- classic kernel, no split: the Linear entries (every epilogue x float4 / scalar epilogue; CS instances)
EPI_OPS = ("fwd_add", "act1", "act2", "act3", "swish_z", "swish_d", "dx_add", "dx_d1", "dx_d1_ip", "dx_d2", "dx_d3", "dx_d3_ip")
CLASSIC_LIN = (
    [L(op, *BIG, 72, [f"epi-{op}-cvec"]) for op in EPI_OPS] + [L(op, 264, 1030, 72, [f"epi-{op}-cscalar"]) for op in EPI_OPS] +
    [L("fwd_add", *BIG, 72, ["cvecoff-addend-4B"], off=dict(addend=1)), L("dx_d1", *BIG, 72, ["cvecoff-dact-4B"], off=dict(dact=1)),
     L("swish_z", *BIG, 72, ["cvecoff-preact-4B"], off=dict(preact=1))] +
    [L("dw", *BIG, 72, ["cs-vec"]), L("dw", *BIG, 76, ["cs-scalar"]), L("dw", 1032, 264, 104, ["cs-vec", "tiles_m9"]),
     L("dw", 262, 1032, 72, ["cs-scalar"]), L("dw_nodb", *BIG, 72, ["classic-oo-vec"])])

# ---- split-K: 264 x 1032 (27 tiles: `few`, s = min(18, K / 64, 32)) and 100 x 100 with K > 2048 (one tile: 32 splits asked for)
SPLIT_GEN = [
    G(*BIG, 264, "kk", ["split3", "reduce-rem3", "rvec"]),               # 3 splits of 96, the last 72
    G(*BIG, 256, "oo", ["split4", "reduce-rem0", "rvec"]),               # 4 x 64
    G(*BIG, 320, "ko", ["split5", "reduce-rem1", "rvec"]),               # 5 x 64: one whole group of four slabs, then one
    G(*BIG, 392, "kk", ["split5", "short-last-split"]),                  # 4 x 96 + 8: the last split has no whole k-tile
    G(*BIG, 512, "ok", ["split8", "grid-multiple-of-8"]),                # 27 tiles x 8 splits = 216 blocks
    G(100, 100, 2056, "kk", ["split22", "reduce-rem2"]),                 # 22 splits of 96
    G(100, 100, 3072, "oo", ["split32"]),                                # 32 x 96
    G(*BIG, 248, "kk", ["nosplit-K248"]),                                # K < 256: not `few`
    G(8192, 128, 512, "ko", ["tiles64-split"]), G(8320, 128, 512, "ko", ["tiles65-nosplit"]),
    # the tile limit: 191 | 192 tile rows (24 row groups, the last with 7 | 8) at K = 1024 (two slabs: no group of four, remainder 2 | unsplit)
    # and at K = 512 (neither splits: more than 64 tiles)
    G(191 * 128, 128, 1024, "ko", ["split2", "tiles191-split", "rvec"]), G(192 * 128, 128, 1024, "ko", ["tiles192-nosplit"]),
    G(191 * 128, 126, 1024, "ko", ["split2", "split2-rscalar"], alpha=0.125),            # N % 4: the scalar reduce loop over two slabs, alpha and bias in finish()
    G(191 * 128, 128, 512, "ko", ["tiles191-K512-nosplit"]), G(192 * 128, 128, 512, "ko", ["tiles192-K512-nosplit"]),
    G(*BIG, 264, "kk", ["rvecoff-ldc"], pad=(0, 0, 1)), G(*BIG, 264, "kk", ["rvecoff-C-4B"], off=dict(C=1)),
    G(264, 1030, 264, "kk", ["rscalar-N"]),                              # N % 4: scalar slab stores and the scalar reduce loop
    G(*BIG, 264, "kk", ["split-alpha"], alpha=-3.0), G(*BIG, 264, "oo", ["split-alpha"], alpha=0.125, pad=(0, 0, 4)),
    G(264, 1030, 264, "ko", ["split-alpha", "rscalar-N"], alpha=-3.0),  # alpha in finish() on the scalar loop too
    G(*BIG, 264, "ko", ["split-scalar-loads"], off=dict(A=1)),
]
SPLIT_LIN = ([L(op, *BIG, 264, [f"reduce-{op}-rvec"]) for op in ("fwd",) + EPI_OPS] +
             [L(op, 264, 1030, 264, [f"reduce-{op}-rscalar"]) for op in ("fwd",) + EPI_OPS] +
             [L("fwd_add", *BIG, 264, ["rvecoff-addend-4B"], off=dict(addend=1)), L("dx_d3", *BIG, 264, ["rvecoff-dact-4B"], off=dict(dact=1)),
              L("dw", 260, 1032, 264, ["reduce-asum-2blocks"]), L("dw", 260, 1030, 392, ["reduce-asum-2blocks", "short-last-split"])])

# ---- uneven two-way split (by route only: the two neighbours that fall back)
UNEVEN = dict(M=2052, N=1924, K=4096)    # 17 x 16 = 272 tiles

# ---- grouped dW: jobs (M = out, N = in, K = rows)
GROUP_K = (4096, 4104, 8200)
GROUP_REFUSED = [(132, 132, 4088), (130, 132, 4096)]

# ---- lockstep: the smallest square-ish shape whose unsplit k-loop has 64 whole tiles (tiles >= 192 so that K = 2048 is not split)
LOCKSTEP = G(1800, 1800, 2048, "kk", ["lockstep"], entry="f32")

# ---- bf16x3: the route-distinct classic / split cases again, and the K at which ITS vectorised fetch starts (16, not 32)
BF3_GEN = ([G(*BIG, 72, lay, [f"bf3-{lay}-vec"]) for lay in LAYOUTS] + [G(*BIG, 76, lay, [f"bf3-{lay}-scalar"]) for lay in LAYOUTS] +
           [G(*BIG, 16, "kk", ["bf3-K16-vec"], batch=(2, 1)), G(*BIG, 24, "oo", ["bf3-K24-vec"], batch=(2, 1)), G(*BIG, 8, "kk", ["bf3-K8-scalar"], batch=(2, 1)),
            G(*BIG, 264, "kk", ["bf3-split3"]), G(100, 100, 2056, "oo", ["bf3-split22"]), G(264, 1030, 392, "ko", ["bf3-split-rscalar"]),
            G(33, 100, 17, "kk", ["bf3-small-stays-small"])])
BF3_LIN = [L("dw", *BIG, 72, ["bf3-cs-vec"]), L("dw", *BIG, 76, ["bf3-cs-scalar"]), L("dw", 260, 1032, 264, ["bf3-cs-split"]),
           L("swish_d", *BIG, 72, ["bf3-epilogue"]), L("dx_d2", 264, 1030, 264, ["bf3-epilogue"])]

# ---- gemm_small: 4 layouts x K (NW 4 | NW 8 | U16 | scalar) over M, N in {1, 15, 16, 17, 33, 100}
SMALL_K = (1, 15, 16, 17, 112, 113, 1024, 1028, 2047, 2048)
_MN = ((1, 100), (15, 17), (16, 16), (17, 33), (33, 15), (100, 1), (100, 100), (33, 100), (16, 100), (15, 1))


def _small_tag(K, lay, off=None, pad=(0, 0, 0)):
    c = G(1, 1, K, lay, [], off=off, pad=pad)
    r = gen_route(c)
    return f"small-nw{r['nw']}" + ("-u16" if r["u16"] else "") + ("-vec" if r["vec"] else "-scalar")


SMALL_GEN = ([G(*_MN[(i + 3 * j) % len(_MN)], K, lay, [_small_tag(K, lay), f"small-{lay}"]) for i, K in enumerate(SMALL_K) for j, lay in enumerate(LAYOUTS)] +
             [G(33, 100, 1028, "kk", ["small-scalar-by-ld", "small-nw8-scalar"], pad=(1, 0, 0)),
              G(33, 100, 112, "ko", ["small-scalar-by-4B", "small-nw4-scalar"], off=dict(A=1)),
              G(33, 100, 2048, "kk", ["small-scalar-by-4B", "small-nw8-scalar"], off=dict(B=1)),
              G(17, 33, 116, "kk", ["small-padded", "small-nw8-vec"], pad=(4, 8, 3), alpha=0.125),
              G(256, 512, 72, "kk", ["small-8tiles"]), G(260, 512, 72, "kk", ["classic-12tiles"]),
              G(512, 1024, 64, "ko", ["small-K64-512tiles32"]), G(512, 1024, 72, "ko", ["classic-K72-512tiles32"]),
              G(100, 100, 2048, "kk", ["small-K2048", "small-nw8-u16-vec"]), G(100, 100, 2056, "kk", ["classic-K2056"])])
SMALL_LIN = ([L(op, 33, 100, 17, [f"small-epi-{op}"]) for op in ("fwd",) + EPI_OPS + ("dw", "dw_nodb")] +
             [L(op, 17, 33, 1028, [f"small-epi-{op}"]) for op in ("act2", "swish_d", "dx_d2", "dw")])
# the pair kernel: (rows, in, out)
PAIR_SHAPES = [(37, 50, 33), (5, 16, 1),                                  # gemm_small_pair_kernel<4 waves, scalar dO loads>
               (20, 24, 16), (130, 48, 15), (130, 48, 16)]                # <4, float4> (out % 4 == 0), <8, scalar> (9 k-groups of rows), <8, float4>
PAIR_VARIANTS = ("all", "no_db", "addend", "act1", "act2", "act3")
PAIR_FALLBACK = (4096, 16, 16)           # dX (4096 x 16, K = 16) is small-wanted, dW (K = 4096 > 2048) is not

# ---- gemm_pst: M is computed from the device's slot count (512 on MI355X: 8320 rows x 8 tile columns = 520 tiles)
PST_N = (1000, 1001)
PST_CASES = [  # (op or 'gen-<layout>', K on the persistent kernel, K one k-tile below it: the classic kernel)
    ("fwd", 96, 64), ("gen-ko", 96, 64), ("act1", 128, 96), ("swish_z", 128, 96), ("swish_d", 128, 96),
    ("dx_d1", 160, 128), ("dx_d1_ip", 160, 128), ("dx_d3", 160, 128), ("dx_d3_ip", 160, 128)]
PST_EPI = {"fwd": 0, "gen-ko": 0, "act1": 1, "swish_z": 1, "swish_d": 3, "dx_d1": 2, "dx_d1_ip": 2, "dx_d3": 4, "dx_d3_ip": 4}
# N = 1001 only where B is k-major: an outer-major B (the dX epilogues 2 and 4) has ldb = N, and the kernel wants ldb % 4 == 0
PST_LIN = [(op, K, Kc, N) for op, K, Kc in PST_CASES if not op.startswith("gen") for N in PST_N if N % 4 == 0 or LIN_OPS[op][0] == "kk"]
PST_GEN = [dict(pad=(4, 0, 0), alpha=1.0, tag="pst-padded-lda"), dict(pad=(0, 0, 8), alpha=1.0, tag="pst-padded-ldc"),
           dict(pad=(0, 0, 0), alpha=0.125, tag="pst-alpha")]


def pst_rows(slots, N=1000):
    """The smallest M % 128 == 0 whose grid has more tiles than the device has resident slots."""
    return (slots // ceil_div(N, 128) + 1) * 128


# ---- special values: (route name, M, N, K) -- the forward ops take (rows, out, in) = (M, N, K), the dX ops (rows, in, out)
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 88.0, -88.0, 104.0, -104.0, 1e-38], np.float32)
SPECIAL_ROUTES = [("small", 33, 100, 17), ("classic-cvec", 264, 1032, 72), ("classic-cscalar", 264, 1030, 72), ("reduce", 264, 1032, 264)]
SPECIAL_OPS = ("act2", "act3", "act1", "swish_z", "swish_d", "fwd_add", "dx_d1", "dx_d2", "dx_d3")
SPECIAL_PST_OPS = ("act1", "swish_z", "swish_d", "dx_d1", "dx_d3")           # the persistent kernel has no ReLU / sigmoid / mask-2 epilogue


# ==================================================================================================== branches
def _classic(r, split=False):
    return r["kind"] == "classic" and r["family"] == 0 and (r["splitk"] > 1) == split


def _one_switch(c, key, **undo):
    """`key` is off for the case and on again once the single named cause is taken away."""
    return _classic(gen_route(c)) and not gen_route(c)[key] and gen_route(c, **undo)[key]


def _lin_switch(c, key, name):
    r0, r1 = lin_route(c["op"], c["M"], c["N"], c["K"], c["off"]), lin_route(c["op"], c["M"], c["N"], c["K"], {})
    return not r0[key] and r1[key] and list(c["off"]) == [name]


def _kt(r):
    return r["ktiles"]


BRANCHES = {}
for _lay in LAYOUTS:
    BRANCHES[f"classic-{_lay}-vec"] = lambda c, r, l=_lay: _classic(r) and r["layout"] == l and r["vec"] and not r["cs"]
    BRANCHES[f"classic-{_lay}-scalar"] = lambda c, r, l=_lay: _classic(r) and r["layout"] == l and not r["vec"] and not r["cs"]
    BRANCHES[f"bf3-{_lay}-vec"] = lambda c, r, l=_lay: r["family"] == 3 and r["layout"] == l and r["vec"] and r["splitk"] == 1
    BRANCHES[f"bf3-{_lay}-scalar"] = lambda c, r, l=_lay: r["family"] == 3 and r["layout"] == l and not r["vec"] and r["splitk"] == 1
    BRANCHES[f"small-{_lay}"] = lambda c, r, l=_lay: r["kind"] == "small" and c["lay"] == l
for _K in KSWEEP:
    BRANCHES[f"classic-K{_K}"] = lambda c, r, K=_K: (_classic(r) and _kt(r) == [(K // 32, K % 32)] and r["vec"] == (K % 8 == 0 and K >= 32))
BRANCHES.update({
    "tiles_m9": lambda c, r: r["tiles_m"] == 9,                          # a second row group of ONE tile row (gsz = 1 < GM = 8)
    "tiles81": lambda c, r: r["tiles_m"] * r["tiles_n"] == 81 and _classic(r),
    "vecoff-A-4B": lambda c, r: _one_switch(c, "vec", off={}), "vecoff-B-4B": lambda c, r: _one_switch(c, "vec", off={}),
    "vecoff-ld": lambda c, r: _one_switch(c, "vec", pad=(0, 0, 0)),
    "vecoff-outer": lambda c, r: _one_switch(c, "vec", M=264, N=1032),
    "vecoff-stride": lambda c, r: _one_switch(c, "vec", odd=None) and gen_route(c)["cvec"],
    "cvecoff-N": lambda c, r: _one_switch(c, "cvec", N=1032) and r["vec"],
    "cvecoff-ldc": lambda c, r: _one_switch(c, "cvec", pad=(0, 0, 0)) and r["vec"],
    "cvecoff-C-4B": lambda c, r: _one_switch(c, "cvec", off={}) and r["vec"],
    "cvecoff-bias-4B": lambda c, r: _one_switch(c, "cvec", off={}) and r["vec"],
    "cvecoff-stride": lambda c, r: _one_switch(c, "cvec", odd=None) and r["vec"],
    "cvecoff-addend-4B": lambda c, r: _classic(r) and _lin_switch(c, "cvec", "addend"),
    "cvecoff-dact-4B": lambda c, r: _classic(r) and _lin_switch(c, "cvec", "dact"),
    "cvecoff-preact-4B": lambda c, r: _classic(r) and _lin_switch(c, "cvec", "preact"),
    "padded-ld": lambda c, r: _classic(r) and all(c["pad"]),
    "batch2x3": lambda c, r: _classic(r) and c["batch"] == (2, 3) and not c["share_b"],
    "shared-B": lambda c, r: _classic(r) and c["share_b"] and c["batch"][0] > 1,
    "alpha": lambda c, r: _classic(r) and c["alpha"] != 1.0,
    "no-bias": lambda c, r: _classic(r) and not c["bias"],
    "cs-vec": lambda c, r: _classic(r) and r["cs"] and r["vec"] and r["layout"] == "oo",
    "cs-scalar": lambda c, r: _classic(r) and r["cs"] and not r["vec"],
    # split-K
    "split3": lambda c, r: _classic(r, True) and r["splitk"] == 3, "split4": lambda c, r: _classic(r, True) and r["splitk"] == 4,
    "split5": lambda c, r: _classic(r, True) and r["splitk"] == 5, "split8": lambda c, r: _classic(r, True) and r["splitk"] == 8,
    "split22": lambda c, r: _classic(r, True) and r["splitk"] == 22, "split32": lambda c, r: _classic(r, True) and r["splitk"] == 32,
    "reduce-rem0": lambda c, r: r["splitk"] > 1 and r["splitk"] % 4 == 0, "reduce-rem1": lambda c, r: r["splitk"] % 4 == 1 and r["splitk"] > 4,
    "reduce-rem2": lambda c, r: r["splitk"] % 4 == 2 and r["splitk"] > 4, "reduce-rem3": lambda c, r: r["splitk"] == 3,
    "rvec": lambda c, r: r["splitk"] > 1 and r["rvec"] and r["vec"],
    "short-last-split": lambda c, r: r["splitk"] > 1 and _kt(r)[-1][0] == 0 and 0 < _kt(r)[-1][1] < 32,
    "grid-multiple-of-8": lambda c, r: (r["tiles_m"] * r["tiles_n"] * r["splitk"]) % 8 == 0 and (r["tiles_m"] * r["tiles_n"]) % 8 != 0,
    "nosplit-K248": lambda c, r: _classic(r) and gen_route(c, K=256)["splitk"] == 4,
    "tiles64-split": lambda c, r: _classic(r, True) and r["tiles_m"] * r["tiles_n"] == 64,
    "tiles65-nosplit": lambda c, r: _classic(r) and r["tiles_m"] * r["tiles_n"] == 65,
    "split2": lambda c, r: _classic(r, True) and r["splitk"] == 2 and r["tiles_m"] == 191 and r["ktiles"] == [(16, 0), (16, 0)],
    "tiles191-split": lambda c, r: _classic(r, True) and r["tiles_m"] * r["tiles_n"] == 191 and r["vec"],
    "tiles192-nosplit": lambda c, r: _classic(r) and r["tiles_m"] * r["tiles_n"] == 192 and c["K"] == 1024,
    "split2-rscalar": lambda c, r: _classic(r, True) and r["splitk"] == 2 and not r["rvec"] and not r["cvec"] and c["alpha"] != 1.0 and c["bias"],
    "tiles191-K512-nosplit": lambda c, r: _classic(r) and r["tiles_m"] == 191 and c["K"] == 512,
    "tiles192-K512-nosplit": lambda c, r: _classic(r) and r["tiles_m"] == 192 and c["K"] == 512,
    "rvecoff-ldc": lambda c, r: _classic(r, True) and r["cvec"] and not r["rvec"] and gen_route(c, pad=(0, 0, 0))["rvec"],
    "rvecoff-C-4B": lambda c, r: _classic(r, True) and r["cvec"] and not r["rvec"] and gen_route(c, off={})["rvec"],
    "rvecoff-addend-4B": lambda c, r: _classic(r, True) and r["cvec"] and _lin_switch(c, "rvec", "addend"),
    "rvecoff-dact-4B": lambda c, r: _classic(r, True) and r["cvec"] and _lin_switch(c, "rvec", "dact"),
    "rscalar-N": lambda c, r: _classic(r, True) and not r["cvec"] and not r["rvec"],
    "split-alpha": lambda c, r: _classic(r, True) and c["alpha"] != 1.0,
    "split-scalar-loads": lambda c, r: _classic(r, True) and not r["vec"],
    "reduce-asum-2blocks": lambda c, r: _classic(r, True) and r["cs"] and ceil_div(c["M"], 256) == 2,
    "lockstep": lambda c, r: _classic(r) and r["layout"] == "kk" and r["vec"] and _kt(r)[0][0] >= 64,
    # bf16x3
    "bf3-K16-vec": lambda c, r: r["family"] == 3 and r["vec"] and c["K"] == 16, "bf3-K24-vec": lambda c, r: r["family"] == 3 and r["vec"] and c["K"] == 24,
    "bf3-K8-scalar": lambda c, r: r["family"] == 3 and not r["vec"] and c["K"] == 8,
    "bf3-split3": lambda c, r: r["family"] == 3 and r["splitk"] == 3, "bf3-split22": lambda c, r: r["family"] == 3 and r["splitk"] == 22,
    "bf3-split-rscalar": lambda c, r: r["family"] == 3 and r["splitk"] > 1 and not r["rvec"],
    "bf3-small-stays-small": lambda c, r: r["family"] == 2,
    "bf3-cs-vec": lambda c, r: r["family"] == 3 and r["cs"] and r["vec"], "bf3-cs-scalar": lambda c, r: r["family"] == 3 and r["cs"] and not r["vec"],
    "bf3-cs-split": lambda c, r: r["family"] == 3 and r["cs"] and r["splitk"] > 1,
    "bf3-epilogue": lambda c, r: r["family"] == 3 and r["kind"] == "classic",
    # gemm_small
    "small-nw4-vec": lambda c, r: r["kind"] == "small" and (r["nw"], r["u16"], r["vec"]) == (4, False, True),
    "small-nw4-scalar": lambda c, r: r["kind"] == "small" and (r["nw"], r["u16"], r["vec"]) == (4, False, False),
    "small-nw8-vec": lambda c, r: r["kind"] == "small" and (r["nw"], r["u16"], r["vec"]) == (8, False, True),
    "small-nw8-scalar": lambda c, r: r["kind"] == "small" and (r["nw"], r["u16"], r["vec"]) == (8, False, False),
    "small-nw8-u16-vec": lambda c, r: r["kind"] == "small" and (r["nw"], r["u16"], r["vec"]) == (8, True, True),
    "small-scalar-by-ld": lambda c, r: r["kind"] == "small" and not r["vec"] and gen_route(c, pad=(0, 0, 0))["vec"],
    "small-scalar-by-4B": lambda c, r: r["kind"] == "small" and not r["vec"] and gen_route(c, off={})["vec"],
    "small-padded": lambda c, r: r["kind"] == "small" and all(c["pad"]),
    "small-8tiles": lambda c, r: r["kind"] == "small", "classic-12tiles": lambda c, r: _classic(r),
    "small-K64-512tiles32": lambda c, r: r["kind"] == "small", "classic-K72-512tiles32": lambda c, r: _classic(r),
    "small-K2048": lambda c, r: r["kind"] == "small", "classic-K2056": lambda c, r: _classic(r, True),
})
for _op in EPI_OPS:
    BRANCHES[f"epi-{_op}-cvec"] = lambda c, r, o=_op: _classic(r) and r["cvec"] and c["op"] == o
    BRANCHES[f"epi-{_op}-cscalar"] = lambda c, r, o=_op: _classic(r) and not r["cvec"] and c["op"] == o
for _op in ("fwd",) + EPI_OPS:
    BRANCHES[f"reduce-{_op}-rvec"] = lambda c, r, o=_op: _classic(r, True) and r["rvec"] and c["op"] == o
    BRANCHES[f"reduce-{_op}-rscalar"] = lambda c, r, o=_op: _classic(r, True) and not r["rvec"] and c["op"] == o
for _op in ("fwd",) + EPI_OPS + ("dw", "dw_nodb"):
    BRANCHES[f"small-epi-{_op}"] = lambda c, r, o=_op: r["kind"] == "small" and c["op"] == o

GEN_TABLES = dict(classic=CLASSIC_GEN, split=SPLIT_GEN, small=SMALL_GEN, lockstep=[LOCKSTEP])
LIN_TABLES = dict(classic=CLASSIC_LIN, split=SPLIT_LIN, small=SMALL_LIN)


def test_tables_cover_branches():
    seen = set()
    for mode, gens, lins in ((0, GEN_TABLES.values(), LIN_TABLES.values()), (1, [BF3_GEN], [BF3_LIN])):
        for table in gens:
            for c in table:
                r = gen_route(c, mode=mode)
                for t in c["tags"]:
                    assert BRANCHES[t](c, r), (t, gen_id(c), r)
                    seen.add(t)
        for table in lins:
            for c in table:
                r = lin_route(c["op"], c["M"], c["N"], c["K"], c["off"], mode=mode)
                for t in c["tags"]:
                    assert BRANCHES[t](c, r), (t, lin_id(c), r)
                    seen.add(t)
    assert seen == set(BRANCHES), (sorted(set(BRANCHES) - seen), sorted(seen - set(BRANCHES)))


def test_case_ids_are_unique():
    for table in list(GEN_TABLES.values()) + [BF3_GEN]:
        ids = [gen_id(c) for c in table]
        assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    for table in list(LIN_TABLES.values()) + [BF3_LIN]:
        ids = [lin_id(c) for c in table]
        assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]


def test_no_big_case_fits_the_small_kernel():
    for table in (CLASSIC_GEN, SPLIT_GEN):
        for c in table:
            assert gen_route(c)["kind"] == "classic", gen_id(c)
    for table in (CLASSIC_LIN, SPLIT_LIN):
        for c in table:
            assert lin_route(c["op"], c["M"], c["N"], c["K"], c["off"])["kind"] == "classic", lin_id(c)
    for c in SMALL_LIN:
        assert lin_route(c["op"], c["M"], c["N"], c["K"], c["off"])["kind"] == "small", lin_id(c)


# ==================================================================================================== gemm_route at its thresholds
def R(M, N, K, lay="kk", **kw):
    return gen_route(G(M, N, K, lay, [], **kw))


def test_small_thresholds():
    assert [small_wanted(100, 100, K, 1, K, K, True, True) for K in (0, 1, 2048, 2049, 2056)] == [False, True, True, False, False]
    assert small_wanted(256, 512, 72, 1, 72, 72, True, True) and not small_wanted(260, 512, 72, 1, 72, 72, True, True)      # 8 | 12 tiles of 128
    assert small_wanted(1024, 128, 72, 1, 72, 72, True, True) and not small_wanted(1028, 128, 72, 1, 72, 72, True, True)    # 8 | 9
    assert small_wanted(512, 1024, 64, 1, 64, 64, True, True) and not small_wanted(512, 1024, 65, 1, 65, 65, True, True)    # K <= 64 clause
    assert small_wanted(512, 1024, 64, 1, 64, 64, True, True) and not small_wanted(516, 1024, 64, 1, 64, 64, True, True)    # 512 | 544 tiles of 32
    assert not small_wanted(100, 100, 72, 2, 72, 72, True, True)                                                            # batched: never
    assert [R(33, 100, K)["nw"] for K in (96, 112, 113, 128)] == [4, 4, 8, 8]                                               # groups >= 8
    assert [R(33, 100, K)["u16"] for K in (1024, 1028, 2048)] == [False, True, True]                                        # 64 < groups <= 128
    assert not R(33, 100, 1028, "ko")["u16"] and not R(33, 100, 1028, pad=(1, 0, 0))["u16"] and not R(33, 100, 2047)["u16"]
    assert R(33, 100, 16, "oo")["vec"] is False and R(33, 100, 16, "ko")["vec"] and not R(33, 100, 18, "ko")["vec"]
    # tiles32 <= 256 is implied by tiles128 <= 8
    assert all(ceil_div(m, 32) * ceil_div(n, 32) <= 128 for m in range(1, 1025, 7) for n in range(1, 1025, 7) if ceil_div(m, 128) * ceil_div(n, 128) <= 8)


def test_splitk_thresholds():
    assert [R(*BIG, K)["splitk"] for K in (248, 256, 264, 320, 392, 512)] == [1, 4, 3, 5, 5, 8]
    assert R(*BIG, 264)["ktiles"] == [(3, 0), (3, 0), (2, 8)] and R(*BIG, 392)["ktiles"][-1] == (0, 8)
    assert R(100, 100, 2056)["splitk"] == 22 and R(100, 100, 2056)["k_per_split"] == 96 and R(100, 100, 3072)["splitk"] == 32
    # few: tiles 64 | 65 at K = 512; the tile limit 191 | 192 at K = 512 (neither splits: not `few`) and at K = 1024
    assert R(8192, 128, 512, "ko")["splitk"] == 8 and R(8320, 128, 512, "ko")["splitk"] == 1
    assert R(191 * 128, 128, 512, "ko")["splitk"] == 1 and R(192 * 128, 128, 512, "ko")["splitk"] == 1
    assert R(191 * 128, 128, 1024, "ko")["splitk"] == 2 and R(192 * 128, 128, 1024, "ko")["splitk"] == 1
    assert R(171 * 128, 128, 1024, "ko")["splitk"] == 2 and R(170 * 128, 128, 1024, "ko")["splitk"] == 3      # 512 / tiles: 2 | 3
    assert R(1100, 1100, 1024, "ko")["splitk"] == 4 and R(1100, 1100, 1016, "ko")["splitk"] == 1             # 81 tiles: K >= 1024 only
    assert R(100, 132, 512, batch=(2, 1))["splitk"] == 1                                                     # batched: never
    # the three caps on s: slots / tiles, K / 64 (few) or K / 256, 32
    assert R(*BIG, 4096)["splitk"] == 16 and R(100, 100, 65536)["splitk"] == 32 and R(1100, 1100, 4096, "ko")["splitk"] == 6
    # rvec: C's own alignment and ldc, not the bias's
    assert R(*BIG, 264)["rvec"] and not R(*BIG, 264, pad=(0, 0, 1))["rvec"] and not R(*BIG, 264, off=dict(C=1))["rvec"]
    assert R(*BIG, 264, off=dict(bias=1))["rvec"] and not R(264, 1030, 264)["rvec"]


def test_splitk_bailout_is_unreachable():
    """`if (few && K < 1024 && s < 4) s = 1` (gemm.hip): with the default 512 slots, few = 64 tiles and 64 rows of k per split, s >= 4
    whenever `few` holds, so no shape stands on the far side of it -- the GPU tables have no case for it."""
    for tiles in range(1, 65):
        for K in range(256, 1024):
            assert min(512 // tiles, K // 64, 32) >= 4


def test_vec_thresholds():
    assert [R(*BIG, K, batch=(2, 1))["vec"] for K in (24, 32, 36, 40)] == [False, True, False, True]
    assert [R(*BIG, K)["kind"] for K in (64, 65)] == ["small", "classic"]                  # 297 tiles of 32: K <= 64 belongs to gemm_small
    assert [gen_route(G(*BIG, K, "kk", [], batch=(2, 1)), mode=1)["vec"] for K in (8, 16, 24, 36)] == [False, True, True, False]
    for lay in LAYOUTS:
        assert R(*BIG, 72, lay)["vec"] and R(*BIG, 72, lay)["cvec"]
    assert not R(262, 1032, 72, "ok")["vec"] and R(262, 1032, 72, "kk")["vec"]        # the outer extent only counts for an outer-major operand
    assert not R(*BIG, 72, off=dict(bias=1))["cvec"] and R(*BIG, 72, off=dict(bias=1), bias=False)["cvec"]


def test_uneven_thresholds():
    u = gemm_route(2052, 1924, 4096, 2052, 1924, 1924, False, False)
    assert u["kind"] == "uneven" and u["K1"] == 2112
    asum = gemm_route(2052, 1924, 4096, 2052, 1924, 1924, False, False, epi=dict(asum=1))
    assert asum["kind"] == "uneven"
    assert gemm_route(2048, 2048, 4096, 2048, 2048, 2048, False, False)["kind"] == "classic"                  # t = 256
    assert gemm_route(2052, 2048, 4096, 2052, 2048, 2048, False, False)["kind"] == "uneven"                   # t = 272
    assert gemm_route(31 * 128, 16 * 128, 4096, 31 * 128, 2048, 2048, False, False)["kind"] == "uneven"       # t = 496
    assert gemm_route(71 * 128, 7 * 128, 4096, 71 * 128, 896, 896, False, False)["kind"] == "classic"         # t = 497
    for change in (dict(K=4088), dict(epi=dict(bias=1)), dict(epi=dict(alpha=2.0)), dict(a_kmajor=True), dict(off=dict(A=1))):
        kw = dict(M=2052, N=1924, K=4096, lda=2052, ldb=1924, ldc=1924, a_kmajor=False, b_kmajor=False)
        kw.update(change)
        if kw["a_kmajor"]:
            kw["lda"] = kw["K"]
        assert gemm_route(**kw)["kind"] == "classic", change


def test_group_thresholds():
    assert [wgrad_route(132, 132, K)["chunk"] for K in GROUP_K] == [1024, 1056, 2080]
    assert wgrad_route(132, 132, 4104)["ktiles"] == [(33, 0)] * 3 + [(29, 8)] and wgrad_route(132, 132, 8200)["ktiles"][-1] == (61, 8)
    assert all(wgrad_route(132, 132, K)["splitk"] == 4 and wgrad_route(132, 132, K)["group"] for K in GROUP_K)
    assert not any(wgrad_route(*s)["group"] for s in GROUP_REFUSED)
    assert not wgrad_route(132, 132, 4100)["group"] and not wgrad_route(132, 132, 4096, (0, 1, 0))["group"]
    assert wgrad_route(2048, 2048, 4096)["group"] and not wgrad_route(2052, 2048, 4096)["group"]              # 256 | 272 tiles
    assert [group_launches(n) for n in (1, 3, 8, 9, 16, 17)] == [1, 1, 1, 2, 2, 3]


def test_pst_thresholds():
    rows = pst_rows(512)
    assert rows == 8320
    for op, K, Kc in PST_CASES:
        if op.startswith("gen"):
            on, below = R(rows, 1000, K, "ko"), R(rows, 1000, Kc, "ko")
        else:
            on = lin_route(op, rows, 1000, K)
            below = lin_route(op, rows, 1000, Kc)
        assert on["kind"] == "pst" and on["epi"] == PST_EPI[op] and below["kind"] == "classic", (op, on, below)
    for op, K, Kc, N in PST_LIN:
        assert lin_route(op, pst_rows(512, N), N, K)["kind"] == "pst" and lin_route(op, pst_rows(512, N), N, Kc)["kind"] == "classic", (op, N)
    assert lin_route("dx_d1", rows, 1001, 160)["kind"] == "classic" and lin_route("act1", rows, 1001, 128)["kind"] == "pst"
    assert lin_route("fwd", rows - 128, 1000, 96)["kind"] == "classic"                                        # 512 tiles: not MORE than the slots
    assert lin_route("fwd", rows, 1000, 1024)["kind"] == "pst" and lin_route("fwd", rows, 1000, 1056)["kind"] == "classic"
    assert lin_route("fwd", rows, 1000, 100)["kind"] == "classic" and lin_route("fwd", rows + 4, 1000, 96)["kind"] == "classic"
    for op in ("act2", "act3", "dx_d2", "fwd_add", "dx_add"):
        assert lin_route(op, rows, 1000, 160)["kind"] == "classic", op
    assert lin_route("fwd", rows, 1000, 96, off=dict(A=1))["kind"] == "classic" and lin_route("fwd", rows, 1000, 96, off=dict(C=1))["kind"] == "pst"
    assert lin_route("fwd", rows, 1000, 96, mode=1)["family"] == 3
    assert pst_rows(608) == 9856 and lin_route("fwd", 9856 - 128, 1000, 96, slots=608)["kind"] == "classic"
    for g in PST_GEN:
        assert R(rows, 1000, 96, "kk", pad=g["pad"], alpha=g["alpha"])["kind"] == "pst"


def test_pair_thresholds():
    for s in PAIR_SHAPES:
        assert pair_route(*s) == "pair"
    assert pair_route(*PAIR_FALLBACK) == "two"
    rows, inf, outf = PAIR_FALLBACK
    assert small_wanted(rows, inf, outf, 1, outf, inf, True, False) and not small_wanted(outf, inf, rows, 1, outf, inf, False, False)
    assert pair_route(37, 50, 33, have_dw=False) == "two" and pair_route(37, 50, 33, mode=1) == "two" and pair_route(37, 50, 33, addend=True, dact=1) == "two"
    assert [pair_instance(r, o) for r, _, o in PAIR_SHAPES] == [dict(nw=4, vec=False), dict(nw=4, vec=False), dict(nw=4, vec=True),
                                                                dict(nw=8, vec=False), dict(nw=8, vec=True)]
    assert pair_instance(112, 16)["nw"] == 4 and pair_instance(113, 16)["nw"] == 8 and pair_instance(5, 113)["nw"] == 8 and not pair_instance(5, 16, 1)["vec"]


# ==================================================================================================== the restatements
def flat_linear(g):
    X, W = g["X"].reshape(-1, g["X"].shape[-1]), g["W"]
    dO = g["dO" if "dO" in g else "dY"]
    return X, W, dO.reshape(-1, dO.shape[-1])


def linear_by_gemm64(X, W, b, dO, alpha_after_bias=False, flip_layout=False, drop_last_kgroup=False, asum_axis_wrong=False):
    """Forward O, dX, dW, db of a Linear from FLAT buffers through gemm64 / asum64, exactly as linear.hip lays the three GEMMs out --
    with four switches that each break one rule (what the comparisons below must reject)."""
    rows, inf = X.shape
    outf = W.shape[0]
    x, w, do = X.reshape(-1), W.reshape(-1), dO.reshape(-1)
    K = inf - (inf % 8 or 8) if drop_last_kgroup else inf               # the partial tile's last k-group never multiplied
    if alpha_after_bias:
        o = 0.5 * gemm64(x, w, rows, outf, K, inf, inf, outf, True, True, 1.0, 2 * b if b is not None else None)
    else:
        o = gemm64(x, w, rows, outf, K, inf, inf, outf, True, True, 0.5, b)
        o = o + gemm64(x, w, rows, outf, K, inf, inf, outf, True, True, 0.5)              # two halves: alpha is really used
    if flip_layout:
        assert inf * outf == w.size
        dx = gemm64(do, w, rows, inf, outf, outf, outf, inf, True, True)                  # W read as [in, out]
    else:
        dx = gemm64(do, w, rows, inf, outf, outf, inf, inf, True, False)
    dw = gemm64(do, x, outf, inf, rows, outf, inf, inf, False, False)
    db = operand(do, 0, rows, outf, outf, True).sum(1)[:outf] if asum_axis_wrong else asum64(do, outf, rows, outf)
    return o.reshape(rows, outf), dx.reshape(rows, inf), dw.reshape(outf, inf), db


WRONG = ("alpha_after_bias", "flip_layout", "drop_last_kgroup", "asum_axis_wrong")
BROKEN_OUTPUT = dict(alpha_after_bias=0, flip_layout=1, drop_last_kgroup=0, asum_axis_wrong=3)


def _close(a, b, tol):
    return a.shape == np.shape(b) and np.allclose(a, b, **tol)


@pytest.mark.parametrize("name", ["linear_2d", "linear_3d", "linear_nobias"])
def test_gemm64_reproduces_the_linear_goldens(golden, name):
    g = golden(name)
    X, W, dO = flat_linear(g)
    b = g.get("b")
    o, dx, dw, db = linear_by_gemm64(X, W, None if b is None else b.reshape(-1), dO)
    np.testing.assert_allclose(o, g["O"].reshape(o.shape), **TOL)
    np.testing.assert_allclose(dx, g["dX"].reshape(dx.shape), **TOL)
    np.testing.assert_allclose(dw, g["dW"], **GTOL)
    if b is not None:
        np.testing.assert_allclose(db, g["db"].reshape(-1), **GTOL)
    want = (g["O"].reshape(o.shape), g["dX"].reshape(dx.shape), g["dW"], g["db"].reshape(-1) if b is not None else None)
    for wrong in WRONG:
        i = BROKEN_OUTPUT[wrong]
        if want[i] is None or (wrong == "alpha_after_bias" and b is None):
            continue
        if wrong == "asum_axis_wrong" and X.shape[0] < W.shape[0]:
            continue                                                    # (16 rows, 40 outputs: the wrong axis has another length -- rejected by shape below)
        got = linear_by_gemm64(X, W, None if b is None else b.reshape(-1), dO, **{wrong: True})[i]
        assert not _close(got, want[i], GTOL if i >= 2 else TOL), wrong


def test_asum_over_the_wrong_axis_is_rejected_by_shape_or_value(golden):
    g = golden("linear_2d")
    X, W, dO = flat_linear(g)
    good = asum64(dO.reshape(-1), W.shape[0], X.shape[0], W.shape[0])
    wrong = dO.astype(np.float64).sum(1)
    assert good.shape == (40,) and wrong.shape == (16,)
    np.testing.assert_allclose(good, g["db"].reshape(-1), **GTOL)
    sq = np.random.default_rng(3).standard_normal((24, 24)).astype(np.float32)         # square: only the values can tell
    assert not np.allclose(asum64(sq.reshape(-1), 24, 24, 24), sq.astype(np.float64).sum(1), **GTOL)
    np.testing.assert_allclose(asum64(sq.reshape(-1), 24, 24, 24), sq.astype(np.float64).sum(0), **GTOL)


def test_epilogue64_reproduces_the_linear_swish_golden(golden):
    g = golden("linear_swish")
    beta = float(g["beta"])
    X, W, dY = flat_linear(g)
    z = gemm64(X.reshape(-1), W.reshape(-1), 16, 40, 24, 24, 24, 40, True, True, bias=g["b"].reshape(-1)).reshape(16, 40)
    y, zz = epilogue64(z, act=ACT_SWISH, beta=beta)
    np.testing.assert_allclose(y, g["Y"], **TOL)
    np.testing.assert_array_equal(zz, z)
    y2, d = epilogue64(z, act=ACT_SWISH_D, beta=beta)
    np.testing.assert_array_equal(y2, y)
    dz = dY * d                                                         # the saved derivative is all the backward needs
    _, dx, dw, db = linear_by_gemm64(X, W, None, dz.astype(np.float32))
    np.testing.assert_allclose(dx, g["dX"], **GTOL)
    np.testing.assert_allclose(dw, g["dW"], **GTOL)
    np.testing.assert_allclose(db, g["db"].reshape(-1), **GTOL)
    # dact 1 on an identity product is the Swish backward itself; dact 3 the multiply by the saved derivative
    np.testing.assert_allclose(epilogue64(dY, dact=1, dact_arg=z, beta=beta)[0], O.swish_backward(z, dY.astype(np.float64), beta), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(epilogue64(dY, dact=3, dact_arg=d)[0], dz, rtol=1e-12, atol=1e-12)
    assert not np.allclose(epilogue64(z, act=ACT_SWISH, beta=1.0)[0], g["Y"], **TOL)                          # beta is used


@pytest.mark.parametrize("op", sorted(LIN_OPS))
def test_lin_reference_matches_the_oracle(op):
    """lin_reference (what both GPU files compare with) against oracle/neunet_oracle.py on the input maker's own data."""
    M, N, K = 9, 14, 11
    d = lin_inputs(op, M, N, K)
    c, pre, asum, mag, v = lin_reference(op, d)
    a, b = d["a"].astype(np.float64), d["b"].astype(np.float64)
    lay, epi = LIN_OPS[op]
    if lay == "kk":
        z = O.linear_forward(a, b, d["bias"].astype(np.float64).reshape(1, -1))
        if "addend" in d:
            z = z + d["addend"]
        want = {ACT_NONE: z, ACT_SWISH: O.swish_forward(z, BETA), ACT_SWISH_D: O.swish_forward(z, BETA), ACT_RELU: O.relu_forward(z),
                ACT_SIGMOID: O.sigmoid_forward(z)}[epi.get("act", ACT_NONE)]
        np.testing.assert_allclose(c, want, rtol=1e-12, atol=1e-12)
        if epi.get("act") == ACT_SWISH:
            np.testing.assert_allclose(pre, z, rtol=1e-12, atol=1e-12)
        if epi.get("act") == ACT_SWISH_D:
            np.testing.assert_allclose(pre, O.swish_backward(z, np.ones_like(z), BETA), rtol=1e-12, atol=1e-12)
    elif lay == "ko":                                                   # a = dO [rows, out], b^T = W [out, in]
        dx = O.linear_backward(np.zeros((M, N)), b.T, None, a)[0]
        if "addend" in d:
            dx = dx + d["addend"]
        x = d["dact"].astype(np.float64) if "dact" in d else None
        want = {0: dx, 1: O.swish_backward(x, dx, BETA) if x is not None else None, 2: O.relu_backward(x, dx) if x is not None else None,
                3: dx * x if x is not None else None}[epi.get("dact", 0)]
        np.testing.assert_allclose(c, want, rtol=1e-12, atol=1e-12)
    else:                                                               # a^T = dO [rows, out], b^T = X [rows, in]
        _, dw, db = O.linear_backward(b.T, np.zeros((M, N)), np.zeros((1, M)), a.T)
        np.testing.assert_allclose(c, dw, rtol=1e-12, atol=1e-12)
        if asum is not None:
            np.testing.assert_allclose(asum, db.reshape(-1), rtol=1e-12, atol=1e-12)
    assert mag.shape == c.shape and np.all(mag >= np.abs(a @ b.T) - 1e-12)


def test_relu_and_masks_are_the_references_on_special_values():
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-38, -1e-38, 2.5, -2.5])
    y, _ = epilogue64(x, act=ACT_RELU)
    assert np.isnan(y[0]) and np.array_equal(y[1:], [np.inf, 0, 0, 0, 1e-38, 0, 2.5, 0])                     # np.maximum(0, x): NaN stays
    assert np.array_equal(epilogue64(np.ones(9), dact=2, dact_arg=x)[0], [0, 1, 0, 0, 0, 1, 0, 1, 0])           # (f > 0): NaN and -0 are not
    s, _ = epilogue64(x, act=ACT_SIGMOID)
    assert np.isnan(s[0]) and s[1] == 1 and s[2] == 0 and s[3] == 0.5
    w, dd = epilogue64(x, act=ACT_SWISH_D)
    assert np.isnan(w[0]) and w[1] == np.inf and np.isnan(w[2]) and np.isnan(dd[1]) and np.isnan(dd[2]) and dd[3] == 0.5


def test_gemm64_addresses_batches_strides_and_padding():
    """The flat-buffer addressing against an explicit loop: a 2 x 3 batch with independent strides, a shared B, padded leading dimensions in
    all four layouts; gaps and padding columns of C stay NaN."""
    for lay in LAYOUTS:
        c = G(5, 6, 7, lay, [], pad=(1, 2, 3), batch=(2, 3), alpha=-3.0)
        g = gen_geometry(c)
        A, B, bias = gen_inputs(c)
        ref, mag = gen_reference(c, A, B, bias)
        want = np.full(g["size"]["C"], np.nan)
        for z1 in range(2):
            for z2 in range(3):
                oa, ob, oc = (z1 * g["st"][n][0] + z2 * g["st"][n][1] for n in "ABC")
                for m in range(5):
                    for n in range(6):
                        s = 0.0
                        for k in range(7):
                            av = A[oa + (m * g["lda"] + k if g["akm"] else k * g["lda"] + m)]
                            bv = B[ob + (n * g["ldb"] + k if g["bkm"] else k * g["ldb"] + n)]
                            s += float(av) * float(bv)
                        want[oc + m * g["ldc"] + n] = -3.0 * s + float(bias[n])
        np.testing.assert_allclose(ref, want, rtol=1e-13, atol=1e-13)
        assert np.isnan(ref).sum() == g["size"]["C"] - 2 * 3 * 5 * 6 and np.array_equal(np.isnan(ref), np.isnan(mag))
    shared = G(5, 6, 7, "kk", [], batch=(2, 3), share_b=True)
    assert gen_geometry(shared)["st"]["B"] == (0, 0)
