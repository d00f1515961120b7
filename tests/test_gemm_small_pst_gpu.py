"""GPU: the two GEMM kernels beside the 128x128-tile one -- csrc/gemm_small.{h,hip} (16x16 tiles, the block's waves split K: NW 4 / NW 8,
the 16-groups-in-flight instance for K in 1025..2048, float4 / scalar loads, 4 layouts, every epilogue, and the pair kernel that does
both gradients of a small Linear in one launch) and csrc/gemm_pst.hip (the persistent kernel of grids with more tiles than resident
slots, epilogues 0..4) -- then special values through every family's epilogue, and the argument handling of nnhipGemmF32[Ex].

Tables, routes and branch names: tests/test_gemm_ref.py.  Helpers, bounds and the family-by-launch-count rule: tests/test_gemm_tiers_gpu.py
(its docstring states every bound used here).  Bit equality is asserted where the project promises it: the persistent kernel against the
classic one on row chunks under the slot count (gemm_pst.hip: same k order, same fmaf chain).

Special values.  {NaN, +inf, -inf, +0, -0, +-88, +-104, 1e-38} go into the bias (so that whole columns of z carry them), into the addend
and into the activation-gradient argument; two rows of X are zero, which makes z = bias EXACTLY there.  Every output is compared element
by element with the float64 restatement: NaN exactly where it has NaN, infinities equal, the rest within the epilogue bound.  The ReLU
epilogue is np.maximum(0, z) (neunet/nn/activations.py:55): before this file the four fused copies used fmaxf and returned 0 for a NaN
pre-activation while nnhipReLUForward returned NaN."""
import numpy as np
import pytest

from gemm_ref import gemm64, pair_route
from test_gemm_ref import (BETA, PAIR_FALLBACK, PAIR_SHAPES, PAIR_VARIANTS, PST_EPI, PST_GEN, PST_LIN, SMALL_GEN, SMALL_LIN,
                           SPECIAL_OPS, SPECIAL_PST_OPS, SPECIAL_ROUTES, SPECIALS, gen_id, lin_id, lin_inputs, lin_reference, lin_route, pst_rows)
from test_gemm_tiers_gpu import (Buf, call, check, check_gen, check_lin, counts, dot_bound_of, epilogue_bound, hip, lin_case, run_gen,  # noqa: F401
                                 run_lin, status)
from test_hip_parity import U24

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, EALIGN = -1, -2


# ==================================================================================================== gemm_small
@pytest.mark.parametrize("c", SMALL_GEN, ids=gen_id)
def test_small_general_entries(hip, c):
    """gemm_small_kernel through nnhipGemmF32Ex: 4 layouts x K in {1, 15, 16, 17, 112 | 113 (NW 4 | 8), 1024 | 1028 (U16 from 65 groups),
    2047 (scalar), 2048} over M, N in {1, 15, 16, 17, 33, 100}; scalar loads by a leading dimension and by a pointer 4 bytes off; padded
    leading dimensions with alpha; and the dispatch thresholds from both sides (8 | 12 tiles of 128, K = 64 | 72 at 512 tiles of 32,
    K = 2048 | 2056) -- the family is asserted from the launch counters."""
    got, inputs = run_gen(c)
    check_gen(c, got, inputs)
    print()


@pytest.mark.parametrize("c", SMALL_LIN, ids=lin_id)
def test_small_linear_epilogues(hip, c):
    """Every epilogue of sg_tile16 (gemm_small.h): bias, addend, the three masks in and out of place, four activations, both `preact`
    contents, the row sums -- with 4 waves (K = 17) and on the U16 / NW 8 instances (K = 1028)."""
    out, d = lin_case(c)
    check_lin(lin_id(c), c["op"], out, d)


def pair_call(variant, rows, inf, outf, seed=0):
    rng = np.random.default_rng(rows * 1000 + inf * 10 + outf + seed)
    X = rng.standard_normal((rows, inf)).astype(np.float32)
    W = (rng.standard_normal((outf, inf)) / np.sqrt(inf)).astype(np.float32)
    dO = rng.standard_normal((rows, outf)).astype(np.float32)
    E = (rng.standard_normal((rows, inf)) * 2).astype(np.float32)       # the addend, or the activation-gradient argument
    if variant == "act2":
        E = np.maximum(E, 0)
    x, w, g, e = Buf(X), Buf(W), Buf(dO), Buf(E)
    dx, dw = Buf(rows * inf), Buf(outf * inf)
    db = None if variant == "no_db" else Buf(outf)
    n0 = counts()
    if variant in ("all", "no_db"):
        call("nnhipLinearModuleBackward", x.t, w.t, g.t, dx.t, dw.t, db.t if db else None, rows, inf, outf)
    elif variant == "addend":
        call("nnhipLinearModuleBackwardEx", x.t, w.t, g.t, e.t, dx.t, dw.t, db.t, rows, inf, outf)
    else:
        call("nnhipLinearModuleBackwardAct", x.t, w.t, g.t, e.t, int(variant[-1]), BETA, dx.t, dw.t, db.t, rows, inf, outf)
    dn = counts() - n0
    for b in (x, w, g, e, dx, dw, db):
        assert b is None or b.intact()
    # float64
    a64, w64, x64 = dO.astype(np.float64), W.astype(np.float64), X.astype(np.float64)
    op = dict(all="dx", no_db="dx", addend="dx_add", act1="dx_d1", act2="dx_d2", act3="dx_d3")[variant]
    d = dict(a=dO, b=np.ascontiguousarray(W.T))
    if variant == "addend":
        d["addend"] = E
    elif variant.startswith("act"):
        d["dact"] = E
    c, _, _, mag, v = lin_reference(op, d)
    tag = f"pair {variant} {rows}x{inf}x{outf}"
    check(tag + " dX", dx.host(), c, epilogue_bound(op, d, c, None, mag, v)[0])
    ref = a64.T @ x64
    check(tag + " dW", dw.host(), ref, dot_bound_of(np.abs(a64).T @ np.abs(x64), ref))
    if db is not None:
        check(tag + " db", db.host(), a64.sum(0), 32 * U24 * np.abs(a64).sum(0) + 4 * U24 * np.abs(a64.sum(0)))
    print()
    return dn


@pytest.mark.parametrize("variant", PAIR_VARIANTS)
@pytest.mark.parametrize("rows,inf,outf", PAIR_SHAPES, ids=lambda v: str(v))
def test_small_pair_kernel(hip, rows, inf, outf, variant):
    """gemm_small_pair_kernel through nnhipLinearModuleBackward[Ex|Act]: dX, dW and db from one launch -- with db null, with dX_addend, with
    each activation gradient -- at 37 x 50 x 33 and 5 x 16 x 1.  The pair launch belongs to no counted family: no counter moves."""
    assert pair_route(rows, inf, outf, addend=variant == "addend", dact=int(variant[-1]) if variant.startswith("act") else 0) == "pair"
    dn = pair_call(variant, rows, inf, outf)
    assert np.array_equal(dn, [0, 0, 0, 0]), dn


def test_small_pair_falls_back_when_one_gemm_is_not_small(hip):
    """4096 x 16 -> 16: the dX GEMM (K = 16) is small-wanted, the dW GEMM (K = 4096 > 2048) is not, so the call runs two launches: one on
    gemm_small (family 2), one on the 128x128 kernel with split-K (family 0)."""
    assert pair_route(*PAIR_FALLBACK) == "two"
    dn = pair_call("all", *PAIR_FALLBACK)
    assert np.array_equal(dn, [1, 0, 1, 0]), dn


# ==================================================================================================== gemm_pst
@pytest.fixture(scope="module")
def slots(hip):
    """Resident blocks of the persistent kernel: two per CU (its LDS admits two for every variant), rounded down to the 8 XCDs."""
    return (torch.cuda.get_device_properties(0).multi_processor_count * 2) & ~7


def halves(rows):
    t = rows // 128
    return [(0, (t + 1) // 2 * 128), ((t + 1) // 2 * 128, rows)]


def slice_rows(d, r0, r1):
    return {k: (v[r0:r1] if k in ("a", "addend", "dact") else v) for k, v in d.items()}


@pytest.mark.parametrize("op,K,Kc,N", PST_LIN, ids=lambda v: str(v))
def test_pst_linear_entries(hip, slots, op, K, Kc, N):
    """The smallest grid above the slot count (8320 x 1000: 65 x 8 = 520 tiles on 512 slots; computed from the device), N = 1000 and 1001
    (a scalar store tail): epilogue 0 at K = 96, 1 and 3 at K = 128, 2 and 4 at K = 160 in and out of place -- family 1 by launch count,
    against float64, and bit-identical to the classic kernel on two row chunks under the slot count.  One k-tile fewer: the classic kernel."""
    M = pst_rows(slots, N)
    r = lin_route(op, M, N, K, slots=slots)
    assert r["kind"] == "pst" and r["epi"] == PST_EPI[op] and lin_route(op, M, N, Kc, slots=slots)["kind"] == "classic"
    out, d = run_lin(op, M, N, K, family=1)
    check_lin(f"pst {op} N={N} K={K}", op, out, d)
    parts = [run_lin(op, r1 - r0, N, K, d=slice_rows(d, r0, r1), family=0)[0] for r0, r1 in halves(M)]
    for k in ("C", "pre"):
        if out[k] is not None:
            assert np.array_equal(out[k], np.concatenate([p[k] for p in parts]), equal_nan=True), f"{k}: persistent != classic"
    run_lin(op, M, N, Kc, family=0)                                     # (its values: the K sweep of test_gemm_tiers_gpu.py)


def ex_call(A2, B2, bias, M, N, K, akm, bkm, ldc, alpha):
    """nnhipGemmF32Ex on 2-D operands whose row pitch is their leading dimension; returns (C [M, ldc] with its padding, launch delta)."""
    a, b, bb, c = Buf(A2), Buf(B2), Buf(bias), Buf(M * ldc)
    n0 = counts()
    call("nnhipGemmF32Ex", a.t, b.t, c.t, bb.t, M, N, K, A2.shape[1], B2.shape[1], ldc, int(akm), int(bkm), 1, 0, 0, 0, 1, 0, 0, 0, alpha)
    assert c.intact()
    return c.host((M, ldc)), counts() - n0


@pytest.mark.parametrize("g", PST_GEN + [dict(pad=(0, 0, 0), alpha=1.0, tag="pst-ko")], ids=lambda g: g["tag"])
def test_pst_general_entry(hip, slots, g):
    """nnhipGemmF32Ex on the persistent kernel (epilogue 0 only): a padded lda, a padded ldc (whose padding columns keep their NaN),
    alpha = 0.125, and the outer-major B instance."""
    N, K = 1000, 96
    M = pst_rows(slots, N)
    bkm = g["tag"] != "pst-ko"
    rng = np.random.default_rng(len(g["tag"]))
    A2 = rng.standard_normal((M, K + g["pad"][0])).astype(np.float32)
    B2 = (rng.standard_normal((N, K) if bkm else (K, N)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    ldc = N + g["pad"][2]
    got, dn = ex_call(A2, B2, bias, M, N, K, True, bkm, ldc, g["alpha"])
    assert np.array_equal(dn, [0, 1, 0, 0]), dn
    args = (A2.reshape(-1), B2.reshape(-1), M, N, K, A2.shape[1], B2.shape[1], ldc, True, bkm, g["alpha"])
    ref, mag = gemm64(*args, bias=bias, c_size=M * ldc), gemm64(*args, absolute=True, c_size=M * ldc)
    assert np.array_equal(np.isnan(got.reshape(-1)), np.isnan(ref)), "the padding columns of ldc were written"
    w = ~np.isnan(ref)
    check(g["tag"], got.reshape(-1)[w], ref[w], dot_bound_of(mag[w], ref[w]))
    parts = []
    for r0, r1 in halves(M):
        p, dn = ex_call(A2[r0:r1], B2, bias, r1 - r0, N, K, True, bkm, ldc, g["alpha"])
        assert np.array_equal(dn, [1, 0, 0, 0]), dn
        parts.append(p)
    assert np.array_equal(got, np.concatenate(parts), equal_nan=True), "persistent != classic"
    print()


# ==================================================================================================== special values
def with_specials(d):
    """Plant SPECIALS in the bias (whole columns of z), the addend and the activation-gradient argument; zero the first and the last row of a."""
    d = {k: v.copy() for k, v in d.items()}
    n = len(SPECIALS)
    M, N = d["a"].shape[0], d["b"].shape[0]
    d["a"][0] = 0
    d["a"][M - 1] = 0
    if "bias" in d:
        d["bias"][:n] = SPECIALS
    for k in ("addend", "dact"):
        if k in d:
            d[k][0, :n] = SPECIALS
            d[k][1, 20:20 + n] = SPECIALS
            d[k][M - 2, N - n:] = SPECIALS
    return d


def special_case(tag, op, M, N, K, family):
    d = with_specials(lin_inputs(op, M, N, K, seed=1))
    out, _ = run_lin(op, M, N, K, d=d, family=family)
    check_lin(tag, op, out, d)
    if op == "swish_z":                                                 # a zero row of X: z = bias, exactly
        for row in (0, M - 1):
            assert np.array_equal(out["pre"][row], d["bias"], equal_nan=True), f"{tag}: z != bias in the zero row {row}"
    if op == "fwd_add":
        for row in (0, M - 1):
            with np.errstate(invalid="ignore"):
                assert np.array_equal(out["C"][row], d["bias"] + d["addend"][row], equal_nan=True), f"{tag}: z != bias + addend in the zero row {row}"


@pytest.mark.parametrize("op", SPECIAL_OPS)
@pytest.mark.parametrize("name,M,N,K", SPECIAL_ROUTES, ids=[r[0] for r in SPECIAL_ROUTES])
def test_special_values(hip, name, M, N, K, op):
    """ReLU, sigmoid, Swish, Swish with z and with the derivative saved, the addend and the three masks on the small kernel, the 128x128
    kernel's float4 and scalar epilogues and the split-K reduce's finish()."""
    r = lin_route(op, M, N, K)
    want = dict(small=("small", 1), reduce=("classic", None)).get(name, ("classic", 1))
    assert r["kind"] == want[0] and (name != "reduce" or r["splitk"] > 1) and (not name.startswith("classic") or r["cvec"] == (name == "classic-cvec"))
    special_case(f"special {name} {op}", op, M, N, K, r["family"])


@pytest.mark.parametrize("op", SPECIAL_PST_OPS)
def test_special_values_persistent(hip, slots, op):
    """The same on the persistent kernel's four Swish epilogues (it has no ReLU, sigmoid or mask-2 epilogue: those requests take gemm.hip)."""
    K = 160 if op.startswith("dx") else 128
    M = pst_rows(slots)
    assert lin_route(op, M, 1000, K, slots=slots)["kind"] == "pst"
    special_case(f"special pst {op}", op, M, 1000, K, 1)


# ==================================================================================================== nnhipGemmF32[Ex]: arguments
def gemm_args(entry, A, B, C, bias, M, N, K, batch=1, batch2=1):
    base = [A, B, C, bias, M, N, K, max(K, 1), max(K, 1), max(N, 1), 1, 1]
    if entry == "nnhipGemmF32":
        return base + [batch, M * K, N * K, M * N]
    return base + [batch, batch2 * M * K, batch2 * N * K, batch2 * M * N, batch2, M * K, N * K, M * N, 1.0]


@pytest.mark.parametrize("entry", ["nnhipGemmF32", "nnhipGemmF32Ex"])
def test_gemm_entry_arguments(hip, entry):
    """M, N or batch = 0 writes nothing and returns 0; K = 0 gives C = bias (or 0); null operands, negative sizes, batch1 * batch2 = 65536,
    batch2 = 0 and a pointer 2 bytes off return their status without a launch (no counter moves) and leave the output untouched."""
    M, N, K = 5, 7, 3
    rng = np.random.default_rng(5)
    a, b, bias = Buf(rng.standard_normal(2 * M * K)), Buf(rng.standard_normal(2 * N * K)), Buf(rng.standard_normal(N))
    c = Buf(2 * M * N)
    untouched = lambda: c.intact() and bool(torch.isnan(c.t).all())
    n0 = counts()
    for m, n, k, bt in ((0, N, K, 1), (M, 0, K, 1), (M, N, K, 0), (0, 0, 0, 0)):
        assert status(entry, *gemm_args(entry, a.t, b.t, c.t, bias.t, m, n, k, bt)) == 0 and untouched()
    refusals = [(gemm_args(entry, None, b.t, c.t, bias.t, M, N, K), EINVAL), (gemm_args(entry, a.t, None, c.t, bias.t, M, N, K), EINVAL),
                (gemm_args(entry, a.t, b.t, None, bias.t, M, N, K), EINVAL), (gemm_args(entry, a.t, b.t, c.t, bias.t, -1, N, K), EINVAL),
                (gemm_args(entry, a.t, b.t, c.t, bias.t, M, -1, K), EINVAL), (gemm_args(entry, a.t, b.t, c.t, bias.t, M, N, -1), EINVAL),
                (gemm_args(entry, a.t, b.t, c.t, bias.t, M, N, K, -1), EINVAL), (gemm_args(entry, a.t, b.t, c.t, bias.t, M, N, K, 65536), EINVAL),
                (gemm_args(entry, a.t.data_ptr() + 2, b.t, c.t, bias.t, M, N, K), EALIGN), (gemm_args(entry, a.t, b.t.data_ptr() + 2, c.t, bias.t, M, N, K), EALIGN),
                (gemm_args(entry, a.t, b.t, c.t.data_ptr() + 2, bias.t, M, N, K), EALIGN)]
    if entry == "nnhipGemmF32Ex":
        refusals += [(gemm_args(entry, a.t, b.t, c.t, bias.t, M, N, K, 256, 256), EINVAL), (gemm_args(entry, a.t, b.t, c.t, bias.t, M, N, K, 2, 0), EINVAL),
                     (gemm_args(entry, a.t, b.t, c.t, bias.t, M, N, K, 2, -1), EINVAL)]
    for args, want in refusals:
        assert status(entry, *args) == want and untouched(), (args[4:], want)
    assert np.array_equal(counts(), n0), "a refused or empty call launched a kernel"
    # K = 0: C = bias, or 0 without one (one launch on the 128x128 kernel: gemm_small wants K >= 1)
    for bb in (bias, None):
        c0 = Buf(M * N)
        n0 = counts()
        assert status(entry, *gemm_args(entry, a.t, b.t, c0.t, bb.t if bb else None, M, N, 0)) == 0
        assert np.array_equal(counts() - n0, [1, 0, 0, 0]) and c0.intact()
        want = np.broadcast_to(bb.host() if bb else np.zeros(N, np.float32), (M, N))
        assert np.array_equal(c0.host((M, N)), want)
