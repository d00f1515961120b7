"""GPU: every kernel instance and dispatch branch of the 128x128-tile GEMMs -- csrc/gemm.hip (gemm_f32_kernel: 4 layouts x float4 / scalar
loads x row sums, split-K with its reduce kernel, the uneven two-way split, the grouped dW launch, lock-step mode) and csrc/gemm_bf3.hip
(the same routes in split-bf16 mode) -- through the C ABI: nnhipGemmF32, nnhipGemmF32Ex and the Linear entries of csrc/linear.hip (the
only public way to an addend, an activation, `preact`, an activation-gradient mask or the row sums), against the float64 restatements
of tests/gemm_ref.py.  tests/test_gemm_small_pst_gpu.py does the same for gemm_small, gemm_pst, special values and argument handling.

The case tables live in tests/test_gemm_ref.py, which also proves on the CPU that each case's ROUTE (gemm_ref.gemm_route, a restatement
of the dispatcher) is the branch the case is named after.  Here every case
  * asserts the kernel family it ran on from the difference of nnhipGemmLaunchCount(0..3) around the call, against that route;
  * keeps every output in an allocation with NaN on both sides (Buf) and asserts that nothing outside the output -- and, with a padded
    ldc or between batches, nothing between its rows -- was written;
  * prints its largest error / bound ratio before it asserts (run with -s; one run's figures are in EXPERIMENTS.md 5.22).

Bounds (none new).  A GEMM output, db included: tests/test_hip_parity.py's dot bound with c = 32, |got - float64| <= 32 2^-24 sum|a||b| +
4 2^-24 |ref| per element.  An epilogue output: that bound on z carried through the epilogue's derivative plus a few ulp of the
evaluation -- the expressions of test_gemm_persistent_swish, test_linear_swish_saved_derivative, test_gemm_persistent_input_grad and
test_linear_backward_act (epilogue_bound below restates them; where they have none -- sigmoid, whose slope is at most 1/4 -- the same
construction).  One absolute term is added for the special-value cases, and written down here: TINY (1 + |z|), TINY = 2^-126, the
smallest normal float32 -- v_exp_f32 / v_rcp_f32 return 0 for results below it, so a sigmoid of less than TINY may come back as 0.
bf16x3: the bound of test_bf16x3_gemm_is_fp32_accurate (largest error relative to the largest entry below 2e-6, and within 2.5 x the
exact-fp32 kernel's own + 3e-7).  Bit equality only where the project promises it: run to run, lock-step on / off, a grouped job
against its company."""
import numpy as np
import pytest

from gemm_ref import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SWISH, ACT_SWISH_D, group_launches, sigmoid, swish_grad, wgrad_route
from test_gemm_ref import (BETA, BF3_GEN, BF3_LIN, CLASSIC_GEN, CLASSIC_LIN, GROUP_K, GROUP_REFUSED, LIN_OPS, LOCKSTEP, SPLIT_GEN, SPLIT_LIN, UNEVEN,
                           gen_geometry, gen_id, gen_inputs, gen_reference, gen_route, lin_id, lin_inputs, lin_reference, lin_route)
from test_hip_parity import U24, assert_within

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN = float("nan")
PAD = 4                                # floats of NaN in front of an operand (16 bytes: the operand itself stays 16-byte aligned)
TINY = 2.0 ** -126


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def stream():
    from neunet_hip._lib import get_current_stream_ptr
    return get_current_stream_ptr()


def call(name, *args):
    from neunet_hip._lib import call_hip_function
    return call_hip_function(name, *args, stream())


def status(name, *args):
    """The entry's own return value (call() raises on a non-zero one)."""
    from neunet_hip._lib import load_hip_function, to_pointer
    return int(load_hip_function(name)(*[to_pointer(a) for a in args], stream()))


def counts():
    from neunet_hip._lib import load_hip_function
    f = load_hip_function("nnhipGemmLaunchCount")
    return np.array([int(f(i)) for i in range(4)])


def host(t):
    return t.detach().cpu().numpy()


class Buf:
    """A flat float operand inside its own allocation: PAD NaN floats, `off` more (off = 1: the operand starts 4 bytes past a 16-byte
    boundary), the operand (`value`, or NaN when only a size is given), and NaN to the end."""

    def __init__(self, value, off=0):
        n = int(value) if np.isscalar(value) else int(np.size(value))
        self.whole = torch.full((PAD + off + n + PAD + 3,), NAN, device="cuda", dtype=torch.float32)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.whole[self.lo:self.hi]
        if not np.isscalar(value):
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(value, np.float32)).reshape(-1)))
        assert self.t.data_ptr() % 16 == 4 * off

    def intact(self):
        """Nothing outside the operand was written."""
        return bool(torch.isnan(self.whole[:self.lo]).all()) and bool(torch.isnan(self.whole[self.hi:]).all())

    def host(self, shape=None):
        a = host(self.t)
        return a if shape is None else a.reshape(shape)


@pytest.fixture
def gemm_mode():
    """Sets the GEMM mode for one test and restores exact fp32."""
    def set_mode(m):
        from neunet_hip._lib import call_hip_function
        call_hip_function("nnhipSetGemmMode", m)
    yield set_mode
    set_mode(0)


# ==================================================================================================== comparing
def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0


def check(tag, got, ref, bound):
    """got against the float64 ref element by element: NaN where (and only where) ref is NaN, infinities equal, everything else within
    `bound` -- and where the reference is finite but the bound is not a finite number (z itself is infinite: relu(-inf) = 0,
    sigmoid(-inf) = 0, sigmoid(+inf) = 1), EQUAL to the reference: those results are exact.  Returns the largest error / bound ratio over
    the bounded entries (printed by the caller's summary line)."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        bound = np.asarray(bound, np.float64).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (tag, got.shape, ref.shape, bound.shape)
    fin = np.isfinite(ref)
    bad = ~fin & ~((np.isnan(ref) & np.isnan(got)) | (ref == got))
    assert not bad.any(), f"{tag}: {int(bad.sum())} non-finite entries differ, first at {int(np.argmax(bad))}: got {got[bad][0]}, want {ref[bad][0]}"
    ok = fin & np.isfinite(bound)
    exact = fin & ~ok
    assert np.array_equal(got[exact], ref[exact]), (f"{tag}: {int((got[exact] != ref[exact]).sum())} of {int(exact.sum())} entries with an infinite "
                                                    f"pre-activation differ from their exact value, first: got {got[exact][got[exact] != ref[exact]][:1]}")
    r = ratio(got[ok], ref[ok], bound[ok])
    print(f"[{tag}] error / bound {r:.3f}", end="; ")
    assert_within(got[ok], ref[ok], bound[ok], tag)
    return r


def dot_bound_of(mag, v, c=32.0):
    with np.errstate(invalid="ignore"):
        return c * U24 * mag + 4 * U24 * np.abs(v)


def epilogue_bound(op, d, c, pre, mag, v):
    """Bounds on (C, preact) of a Linear op: the dot bound on v = a b^T + bias carried through the epilogue."""
    epi = LIN_OPS[op][1]
    act, dact = epi.get("act", ACT_NONE), epi.get("dact", 0)
    with np.errstate(invalid="ignore", over="ignore"):
        zb = dot_bound_of(mag, v)
        z = v
        if "addend" in d:
            z = v + d["addend"].astype(np.float64)
            zb = zb + 4 * U24 * np.abs(z)
        if dact:
            x = d["dact"].astype(np.float64)
            if dact == 2:
                return zb * (x > 0), None
            if dact == 3:
                return zb * np.abs(x) + 8 * U24 * np.abs(c) + TINY, None                # test_linear_swish_saved_derivative
            s = sigmoid(BETA * x)
            f = x * s
            spmag = np.abs(BETA * f) + s * (1 + np.abs(BETA * f))                        # test_gemm_persistent_input_grad
            return zb * np.abs(swish_grad(x, BETA)) + 16 * U24 * np.abs(v) * spmag + TINY * (1 + np.abs(v)) * (1 + np.abs(x)), None
        if act in (ACT_SWISH, ACT_SWISH_D):
            s = sigmoid(BETA * z)
            cb = zb * (np.abs(s) + np.abs(BETA * z * s * (1 - s))) + 16 * U24 * np.abs(z * s) + TINY * (1 + np.abs(z))   # test_gemm_persistent_swish
            if act == ACT_SWISH:
                return cb, zb
            return cb, zb * BETA * (1 + np.abs(BETA * z)) + 32 * U24 * (1 + np.abs(pre)) + TINY * (1 + np.abs(z))         # ..._saved_derivative
        if act == ACT_RELU:
            return zb, None
        if act == ACT_SIGMOID:
            s = sigmoid(z)
            return zb * 0.25 + 16 * U24 * s * (1 + np.abs(z) * (1 - s)) + TINY, None
        return zb, None


# ==================================================================================================== running
def run_gen(c, check_family=True, mode=0):
    """One call of a general entry on a table case.  Returns (C flat, the Buf of C)."""
    g = gen_geometry(c)
    A, B, bias = gen_inputs(c)
    a, b, cc = Buf(A[:max(g["size"]["A"], 1)], c["off"].get("A", 0)), Buf(B[:max(g["size"]["B"], 1)], c["off"].get("B", 0)), Buf(g["size"]["C"], c["off"].get("C", 0))
    bb = Buf(bias, c["off"].get("bias", 0)) if bias is not None else None
    (sA1, sA2), (sB1, sB2), (sC1, sC2) = g["st"]["A"], g["st"]["B"], g["st"]["C"]
    n0 = counts()
    if c["entry"] == "f32":
        assert c["batch"][1] == 1 and c["alpha"] == 1.0
        call("nnhipGemmF32", a.t, b.t, cc.t, bb.t if bb else None, c["M"], c["N"], c["K"], g["lda"], g["ldb"], g["ldc"], int(g["akm"]), int(g["bkm"]),
             c["batch"][0], sA1, sB1, sC1)
    else:
        call("nnhipGemmF32Ex", a.t, b.t, cc.t, bb.t if bb else None, c["M"], c["N"], c["K"], g["lda"], g["ldb"], g["ldc"], int(g["akm"]), int(g["bkm"]),
             c["batch"][0], sA1, sB1, sC1, c["batch"][1], sA2, sB2, sC2, c["alpha"])
    got = cc.host()
    if check_family:
        want = np.zeros(4, int)
        fam = gen_route(c, mode=mode)["family"]
        if fam is not None:
            want[fam] = 1
        assert np.array_equal(counts() - n0, want), (gen_id(c), counts() - n0, want)
    assert cc.intact() and a.intact() and b.intact() and np.array_equal(a.host(), A[:max(g["size"]["A"], 1)]), gen_id(c)
    return got, (A, B, bias)


def check_gen(c, got, inputs, tag=None):
    ref, mag = gen_reference(c, *inputs)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{gen_id(c)}: written where nothing belongs (padding of ldc, gaps between batches) or not written"
    w = ~np.isnan(ref)
    return check(tag or gen_id(c), got[w], ref[w], dot_bound_of(mag[w], ref[w]))


def run_lin(op, M, N, K, off=None, d=None, family=None):
    """One call of the Linear entry behind `op` (test_gemm_ref.LIN_OPS).  Returns (dict of host outputs, inputs)."""
    off = off or {}
    d = d if d is not None else lin_inputs(op, M, N, K)
    lay, epi = LIN_OPS[op]
    A = Buf(d["a"] if lay[0] == "k" else d["a"].T, off.get("A", 0))
    B = Buf(d["b"] if lay[1] == "k" else d["b"].T, off.get("B", 0))
    C = Buf(M * N, off.get("C", 0))
    bias = Buf(d["bias"], off.get("bias", 0)) if "bias" in d else None
    add = Buf(d["addend"], off.get("addend", 0)) if "addend" in d else None
    inplace = op.endswith("_ip")
    if inplace:
        C = Buf(d["dact"], off.get("C", 0))
        arg = C
    else:
        arg = Buf(d["dact"], off.get("dact", 0)) if "dact" in d else None
    pre = Buf(M * N, off.get("preact", 0)) if epi.get("preact") else None
    asum = Buf(M) if epi.get("asum") else None
    n0 = counts()
    if op in ("fwd", "fwd_add"):
        call("nnhipLinearModuleForwardEx", A.t, B.t, bias.t, add.t if add else None, C.t, M, K, N)
    elif op in ("act1", "act2", "act3"):
        call("nnhipLinearActivationForward", A.t, B.t, bias.t, C.t, M, K, N, int(op[-1]), BETA)
    elif op in ("swish_z", "swish_d"):
        call("nnhipLinearSwishForward", A.t, B.t, bias.t, C.t, pre.t, M, K, N, BETA, 1 if op == "swish_z" else 2)
    elif op == "dx":
        call("nnhipLinearModuleBackward", B.t, B.t, A.t, C.t, None, None, M, N, K)             # X is not read without dW
    elif op == "dx_add":
        call("nnhipLinearModuleBackwardEx", B.t, B.t, A.t, add.t, C.t, None, None, M, N, K)
    elif op in ("dx_d1", "dx_d1_ip"):
        call("nnhipLinearInputGradSwish", A.t, B.t, arg.t, C.t, M, N, K, BETA)
    elif op == "dx_d2":
        call("nnhipLinearInputGradReLU", A.t, B.t, arg.t, C.t, M, N, K)
    elif op in ("dx_d3", "dx_d3_ip"):
        call("nnhipLinearInputGradScaled", A.t, B.t, arg.t, C.t, M, N, K)
    else:
        assert op in ("dw", "dw_nodb")
        call("nnhipLinearModuleBackward", B.t, B.t, A.t, None, C.t, asum.t if asum else None, K, N, M)   # W is not read without dX
    out = dict(C=C.host((M, N)), pre=pre.host((M, N)) if pre else None, asum=asum.host() if asum else None)
    if family is not None:
        want = np.zeros(4, int)
        want[family] = 1
        assert np.array_equal(counts() - n0, want), (op, M, N, K, counts() - n0, want)
    for buf in (A, B, C, bias, add, arg, pre, asum):
        assert buf is None or buf.intact(), (op, M, N, K)
    return out, d


def check_lin(tag, op, out, d):
    c, pre, asum, mag, v = lin_reference(op, d)
    cb, pb = epilogue_bound(op, d, c, pre, mag, v)
    r = [check(tag + " C", out["C"], c, cb)]
    if out["pre"] is not None:                                          # (act 1 through nnhipLinearActivationForward saves no z)
        r.append(check(tag + " preact", out["pre"], pre, pb))
    if asum is not None:
        a = d["a"].astype(np.float64)
        r.append(check(tag + " asum", out["asum"], asum, 32 * U24 * np.abs(a).sum(1) + 4 * U24 * np.abs(asum)))
    print()
    return max(r)


def lin_case(c, mode=0):
    r = lin_route(c["op"], c["M"], c["N"], c["K"], c["off"], mode=mode)
    out, d = run_lin(c["op"], c["M"], c["N"], c["K"], c["off"], family=r["family"])
    return out, d


# ==================================================================================================== classic, no split
@pytest.mark.parametrize("c", CLASSIC_GEN, ids=gen_id)
def test_classic_general_entries(hip, c):
    """nnhipGemmF32 / nnhipGemmF32Ex on the unsplit 128x128 kernel: layouts, k-tile counts and tails, each off-switch of the float4 loads
    and of the float4 epilogue alone, padded leading dimensions, two batch levels, a shared operand, alpha."""
    got, inputs = run_gen(c)
    check_gen(c, got, inputs)
    print()


@pytest.mark.parametrize("c", CLASSIC_LIN, ids=lin_id)
def test_classic_linear_epilogues(hip, c):
    """Every epilogue of gemm_epilogue (addend, the three masks in and out of place, four activations, both `preact` contents) in its float4
    and its scalar copy, each epilogue operand 4 bytes off in turn, and the row-sum (CS) instances with float4 and scalar loads."""
    out, d = lin_case(c)
    check_lin(lin_id(c), c["op"], out, d)


# ==================================================================================================== split-K
@pytest.mark.parametrize("c", SPLIT_GEN, ids=gen_id)
def test_splitk_general_entries(hip, c):
    """Split-K through the general entries: 3 / 4 / 5 / 8 / 22 / 32 slabs (both loops of the reduce, remainders 0..3), a last split
    without a whole k-tile, both sides of `few` (64 | 65 tiles at K = 512, K = 248 | 256), the float4 and the scalar reduce, alpha in
    finish().  Deterministic: a second run gives the same bits."""
    got, inputs = run_gen(c)
    check_gen(c, got, inputs)
    again, _ = run_gen(c)
    assert np.array_equal(got, again, equal_nan=True), "split-K is not run-to-run deterministic"
    print()


@pytest.mark.parametrize("c", SPLIT_LIN, ids=lin_id)
def test_splitk_reduce_epilogues(hip, c):
    """finish() of splitk_reduce_body -- the second copy of the whole epilogue -- on the float4 and on the scalar loop; the row-sum
    partials with two tail blocks (M = 260)."""
    out, d = lin_case(c)
    check_lin(lin_id(c), c["op"], out, d)
    again, _ = lin_case(c)
    for k in out:
        assert out[k] is None or np.array_equal(out[k], again[k], equal_nan=True), k


# ==================================================================================================== uneven two-way split
@pytest.fixture(scope="module")
def uneven_data():
    M, N, K = UNEVEN["M"], UNEVEN["N"], UNEVEN["K"]
    rng = np.random.default_rng(2052)
    dO = rng.standard_normal((K, M)).astype(np.float32)                 # A, outer-major: [rows, out]
    X = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)   # B, outer-major: [rows, in]
    a, b = dO.astype(np.float64), X.astype(np.float64)
    return dO, X, a.T @ b, np.abs(a).T @ np.abs(b), a.sum(0), np.abs(a).sum(0)


@pytest.mark.parametrize("with_asum", [False, True], ids=["plain", "asum"])
def test_uneven_two_way_split(hip, uneven_data, with_asum):
    """2052 x 1924 x 4096, both operands outer-major: 17 x 16 = 272 tiles, one under-filled generation, so the reduction of every tile is
    cut at K1 = 2112 into a long and a short job of one grouped launch and the two slabs meet in the reduce (gemm_f32_uneven_split).
    Family 0 by launch count; the route (and its neighbours t = 256 and t = 497, which fall back) is pinned in test_gemm_ref.py.  The whole
    output against float64."""
    M, N, K = UNEVEN["M"], UNEVEN["N"], UNEVEN["K"]
    dO, X, ref, mag, db, dbmag = uneven_data
    a, b, c = Buf(dO), Buf(X), Buf(M * N)
    s = Buf(M) if with_asum else None
    n0 = counts()
    if with_asum:
        call("nnhipLinearModuleBackward", b.t, b.t, a.t, None, c.t, s.t, K, N, M)
    else:
        call("nnhipGemmF32", a.t, b.t, c.t, None, M, N, K, M, N, N, 0, 0, 1, 0, 0, 0)
    assert np.array_equal(counts() - n0, [1, 0, 0, 0]) and c.intact() and (s is None or s.intact())
    check("uneven C", c.host(), ref, dot_bound_of(mag, ref))
    if with_asum:
        check("uneven asum", s.host(), db, 32 * U24 * dbmag + 4 * U24 * np.abs(db))
    print()


# ==================================================================================================== grouped dW
def group_jobs():
    """Nine jobs 132 x 132 x K, three of each K of GROUP_K: (K, dO [K, 132], X [K, 132])."""
    jobs = []
    for i in range(9):
        K = GROUP_K[i % 3]
        rng = np.random.default_rng(100 + i)
        jobs.append((K, rng.standard_normal((K, 132)).astype(np.float32), (rng.standard_normal((K, 132)) / np.sqrt(K)).astype(np.float32)))
    return jobs


def run_group(jobs):
    """Queue the jobs' dW (+ db) GEMMs with deferral on, flush once; returns [(dW, db)] and the launch-count difference."""
    bufs = []
    n0 = counts()
    call("nnhipWeightGradDefer", 1)
    try:
        for K, dO, X in jobs:
            a, b, dw, db = Buf(dO), Buf(X), Buf(132 * 132), Buf(132)
            bufs.append((a, b, dw, db))
            call("nnhipLinearModuleBackward", b.t, b.t, a.t, None, dw.t, db.t, K, 132, 132)
        from neunet_hip._lib import load_hip_function
        assert load_hip_function("nnhipWeightGradPending")() == len(jobs)
        assert np.array_equal(counts(), n0), "a queued job was launched before the flush"
        call("nnhipWeightGradFlush")
        assert load_hip_function("nnhipWeightGradPending")() == 0
    finally:
        call("nnhipWeightGradDefer", 0)
    torch.cuda.synchronize()
    for a, b, dw, db in bufs:
        assert dw.intact() and db.intact()
    return [(dw.host((132, 132)), db.host()) for _, _, dw, db in bufs], counts() - n0


def test_grouped_dw_bits_do_not_depend_on_the_company(hip):
    """nnhipWeightGradDefer(1) + the backward entries + nnhipWeightGradFlush: jobs of 132 x 132 x K, K in {4096, 4104, 8200} (chunks of
    1024; 1056 with a last chunk of 936 = 29 k-tiles + 8; 2080).  The header's promise (ABI 204): a job's bits do not depend on what it is
    launched with -- each of three jobs alone, with two others, and as one of nine (more than GEMM_GROUP_MAX = 8: two launches) gives
    the same dW and db bit for bit; every job against float64; nothing pending afterwards.  K = 4104 and 8200 lie beyond the K <= 4096
    the c = 32 of the dot bound was measured for: their ratios are printed like the others and held to the same bound."""
    jobs = group_jobs()
    for j in jobs:
        assert wgrad_route(132, 132, j[0])["group"]
    nine, dn = run_group(jobs)
    assert np.array_equal(dn, [9, 0, 0, 0]) and group_launches(9) == 2
    three, dn = run_group(jobs[:3])
    assert np.array_equal(dn, [3, 0, 0, 0])
    for i in range(3):
        alone, dn = run_group(jobs[i:i + 1])
        assert np.array_equal(dn, [1, 0, 0, 0])
        for other in (three[i], nine[i]):
            assert np.array_equal(alone[0][0], other[0]) and np.array_equal(alone[0][1], other[1]), f"job {i} (K = {jobs[i][0]}) depends on its company"
    for i, (K, dO, X) in enumerate(jobs):
        a, b = dO.astype(np.float64), X.astype(np.float64)
        ref, db = a.T @ b, a.sum(0)
        check(f"group job {i} K={K} dW", nine[i][0], ref, dot_bound_of(np.abs(a).T @ np.abs(b), ref))
        check(f"group job {i} K={K} db", nine[i][1], db, 32 * U24 * np.abs(a).sum(0) + 4 * U24 * np.abs(db))
        print()


@pytest.mark.parametrize("M,N,K", GROUP_REFUSED, ids=lambda v: str(v))
def test_grouped_dw_refuses_and_computes_in_place(hip, M, N, K):
    """K = 4088 (below 4096) and M = 130 (not a multiple of 4) are refused by gemm_f32_wgrad_group_ok: with deferral on, the backward entry
    launches the dW GEMM itself (the launch counter moves at the call, nothing is pending) and the result is there without a flush."""
    from neunet_hip._lib import load_hip_function
    assert not wgrad_route(M, N, K)["group"]
    d = lin_inputs("dw", M, N, K)
    call("nnhipWeightGradDefer", 1)
    try:
        out, d = run_lin("dw", M, N, K, d=d, family=0)
        assert load_hip_function("nnhipWeightGradPending")() == 0
    finally:
        call("nnhipWeightGradDefer", 0)
    check_lin(f"refused {M}x{N}x{K}", "dw", out, d)


# ==================================================================================================== split-bf16 mode
def bf3_errors(got3, got1, ref, tag):
    w = np.isfinite(ref)
    e3, e1 = (float(np.abs(g[w] - ref[w]).max() / np.abs(ref[w]).max()) for g in (np.asarray(got3, np.float64), np.asarray(got1, np.float64)))
    print(f"[{tag}] bf16x3 error {e3:.2e} of the largest entry (limit 2e-6), exact-fp32 kernel {e1:.2e}", end="; ")
    assert e3 < 2e-6, (tag, e3)
    assert e3 <= 2.5 * e1 + 3e-7, (tag, e3, e1)


@pytest.mark.parametrize("c", BF3_GEN, ids=gen_id)
def test_bf16x3_general_entries(hip, gemm_mode, c):
    """nnhipSetGemmMode(1): the route-distinct classic and split-K cases on gemm_bf3_kernel (family 3 by launch count), K = 16 and 24
    where ITS float4 fetch starts, and a small-wanted problem, which stays on gemm_small (family 2) in either mode."""
    gemm_mode(1)
    got3, inputs = run_gen(c, mode=1)
    gemm_mode(0)
    got1, _ = run_gen(c, mode=0)
    ref, _ = gen_reference(c, *inputs)
    assert np.array_equal(np.isnan(got3), np.isnan(ref))
    bf3_errors(got3, got1, ref, gen_id(c))
    if gen_route(c, mode=1)["family"] == 2:
        assert np.array_equal(got3, got1, equal_nan=True)
    print()


@pytest.mark.parametrize("c", BF3_LIN, ids=lin_id)
def test_bf16x3_linear_entries(hip, gemm_mode, c):
    """The row-sum instances, the split-K reduce with row sums and two epilogues on gemm_bf3_kernel."""
    gemm_mode(1)
    out3, d = lin_case(c, mode=1)
    gemm_mode(0)
    out1, _ = lin_case(c, mode=0)
    cref, pre, asum, mag, v = lin_reference(c["op"], d)
    bf3_errors(out3["C"], out1["C"], cref, lin_id(c) + " C")
    if pre is not None:
        bf3_errors(out3["pre"], out1["pre"], pre, lin_id(c) + " preact")
    if asum is not None:
        bf3_errors(out3["asum"], out1["asum"], asum, lin_id(c) + " asum")
    print()


def test_bf16x3_grouped_dw(hip, gemm_mode):
    """The grouped dW launch of gemm_bf3.hip: three jobs, one of each K, counted on family 3."""
    jobs = group_jobs()[:3]
    gemm_mode(1)
    got3, dn = run_group(jobs)
    assert np.array_equal(dn, [0, 0, 0, 3])
    gemm_mode(0)
    got1, _ = run_group(jobs)
    for i, (K, dO, X) in enumerate(jobs):
        a, b = dO.astype(np.float64), X.astype(np.float64)
        bf3_errors(got3[i][0], got1[i][0], a.T @ b, f"bf3 group K={K} dW")
        bf3_errors(got3[i][1], got1[i][1], a.sum(0), f"bf3 group K={K} db")
    print()


# ==================================================================================================== lock-step mode
def test_lockstep_smallest_shape_is_bit_identical(hip):
    """nnhipSetGemmLockstep(1) changes issue priorities only where a block's k-loop has at least 64 whole k-tiles and both operands have the
    same layout: 1800 x 1800 x 2048 (225 tiles, so K = 2048 is not split) is the smallest such shape.  Bit-identical to lock-step off; a
    sample of rows against float64."""
    from neunet_hip._lib import call_hip_function
    c = LOCKSTEP
    got, inputs = run_gen(c)
    call_hip_function("nnhipSetGemmLockstep", 1)
    try:
        locked, _ = run_gen(c)
    finally:
        call_hip_function("nnhipSetGemmLockstep", 0)
    assert np.array_equal(got, locked)
    A, B, bias = inputs
    M, N, K = c["M"], c["N"], c["K"]
    rows = np.r_[0:8, 127:130, 1020:1030, M - 8:M]
    a, b = A.reshape(M, K)[rows].astype(np.float64), B.reshape(N, K).astype(np.float64)
    ref = a @ b.T + bias
    check("lockstep rows", got.reshape(M, N)[rows], ref, dot_bound_of(np.abs(a) @ np.abs(b).T, ref))
    print()
