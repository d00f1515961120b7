"""Float64 restatements of the GEMM family (csrc/gemm.hip, gemm_common.h, gemm_small.{h,hip}, gemm_pst.hip, gemm_bf3.hip and the Linear
entries of linear.hip): what a call computes, element by element from flat buffers, and which kernel it is sent to.  NumPy only.

    gemm64        C[b] = alpha op(A[b]) op(B[b]) + bias from FLAT operands: leading dimensions, both layout flags and the two-level
                  batch strides are applied here, so a test of a padded / strided / shared operand checks the addressing too
    epilogue64    what follows the product, in the order of GemmParams (gemm_common.h): addend, the activation-gradient masks
                  dact 1 / 2 / 3, the activations swish / relu / sigmoid / swish-with-derivative and the `preact` output
    asum64        row sums of an outer-major A (Linear: db = column sums of dO, riding in the dW GEMM)
    gemm_route    the dispatcher gemm_f32_ex restated (with gemm_small_wanted, gemm_pst_wanted / pst_epi and the uneven-split
                  condition); wgrad_route restates wgrad_chunk / gemm_f32_wgrad_group_ok, pair_route the one-launch Linear backward

ReLU and its mask are the reference's (neunet/nn/activations.py:55 `maximum(0, x)`, :44-45 `grad * (f_x > 0)`), Swish and its derivative
activations.py:225-230 / :212-216, the sigmoid :21 -- not the kernels' expressions."""
import numpy as np

ACT_NONE, ACT_SWISH, ACT_RELU, ACT_SIGMOID, ACT_SWISH_D = 0, 1, 2, 3, 4
BM = BN = 128
BK = 32
GEMM_GROUP_MAX = 8
FAMILY_CLASSIC, FAMILY_PST, FAMILY_SMALL, FAMILY_BF3 = 0, 1, 2, 3


def ceil_div(a, b):
    return -(-a // b)


# ==================================================================================================== values
def operand(P, off, rows, k, ld, kmajor):
    """op(P)[r, k] of a flat buffer: P[off + r ld + k] when the reduction dim is contiguous (k-major), P[off + k ld + r] otherwise."""
    P = np.asarray(P, np.float64).reshape(-1)
    if rows == 0 or k == 0:
        return np.zeros((rows, k))
    last = off + ((rows - 1) * ld + k - 1 if kmajor else (k - 1) * ld + rows - 1)
    assert 0 <= off and last < P.size, "operand window outside its buffer"
    st = P.strides[0]
    return np.lib.stride_tricks.as_strided(P[off:], (rows, k), (ld * st, st) if kmajor else (st, ld * st), writeable=False)


def gemm64(A, B, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, alpha=1.0, bias=None, batch1=1, batch2=1, sA=(0, 0), sB=(0, 0), sC=(0, 0),
           c_size=None, absolute=False):
    """The flat float64 C buffer (NaN where the call writes nothing: padding columns of ldc > N, gaps between batches).
    absolute = True: |alpha| |op(A)| |op(B)| instead (no bias) -- the sum the rounding error of a dot product is proportional to."""
    size = c_size if c_size is not None else (batch1 - 1) * sC[0] + (batch2 - 1) * sC[1] + max(M - 1, 0) * ldc + N
    C = np.full(max(size, 0), np.nan)
    for z1 in range(batch1):
        for z2 in range(batch2):
            a = operand(A, z1 * sA[0] + z2 * sA[1], M, K, lda, a_kmajor)
            b = operand(B, z1 * sB[0] + z2 * sB[1], N, K, ldb, b_kmajor)
            if absolute:
                v = abs(alpha) * (np.abs(a) @ np.abs(b).T)
            else:
                v = alpha * (a @ b.T)
                if bias is not None:
                    v = v + np.asarray(bias, np.float64).reshape(1, N)
            off = z1 * sC[0] + z2 * sC[1]
            for m in range(M):
                C[off + m * ldc: off + m * ldc + N] = v[m]
    return C


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-np.asarray(x, np.float64)))


def swish(x, beta=1.0):
    with np.errstate(invalid="ignore"):
        return x * sigmoid(beta * x)


def swish_grad(x, beta=1.0):
    with np.errstate(invalid="ignore"):
        f = swish(x, beta)
        return beta * f + sigmoid(beta * x) * (1 - beta * f)


def relu(x):
    return np.maximum(0, x)


def relu_mask(f):
    return np.asarray(f) > 0


def epilogue64(v, addend=None, dact=0, dact_arg=None, act=ACT_NONE, beta=1.0):
    """(C, preact) from v = alpha A B + bias.  preact is z for ACT_SWISH, swish'(z) for ACT_SWISH_D, None otherwise."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if addend is not None:
            v = v + np.asarray(addend, np.float64)
        if dact_arg is not None:
            x = np.asarray(dact_arg, np.float64)
            if dact == 2:
                v = v * relu_mask(x)
            elif dact == 3:
                v = v * x
            else:
                assert dact == 1
                v = v * swish_grad(x, beta)
        if act == ACT_SWISH:
            return swish(v, beta), v
        if act == ACT_SWISH_D:
            return swish(v, beta), swish_grad(v, beta)
        if act == ACT_RELU:
            return relu(v), None
        if act == ACT_SIGMOID:
            return sigmoid(v), None
        assert act == ACT_NONE
        return v, None


def asum64(A, M, K, lda):
    """asum[m] = sum_k A[k lda + m]: row sums of an outer-major A."""
    return operand(A, 0, M, K, lda, False).sum(axis=1)


# ==================================================================================================== dispatch
def small_wanted(M, N, K, batch, lda, ldb, a_kmajor, b_kmajor):
    """gemm_small_wanted (gemm_small.hip)."""
    if batch != 1 or M <= 0 or N <= 0 or K <= 0 or K > 2048:
        return False
    ea = (M - 1) * lda + K if a_kmajor else (K - 1) * lda + M
    eb = (N - 1) * ldb + K if b_kmajor else (K - 1) * ldb + N
    if ea * 4 >= 1 << 31 or eb * 4 >= 1 << 31:
        return False
    tiles128, tiles32 = ceil_div(M, 128) * ceil_div(N, 128), ceil_div(M, 32) * ceil_div(N, 32)
    return (tiles128 <= 8 and tiles32 <= 256) or (K <= 64 and tiles32 <= 512)


def small_instance(K, lda, ldb, a_kmajor, b_kmajor, offA=0, offB=0):
    """gemm_small(): waves per block, the 16-groups-in-flight instance, float4 loads."""
    vec = ((a_kmajor or b_kmajor) and K % 4 == 0 and (not a_kmajor or (offA % 4 == 0 and lda % 4 == 0))
           and (not b_kmajor or (offB % 4 == 0 and ldb % 4 == 0)))
    groups = (K + 15) >> 4
    nw = 8 if groups >= 8 else 4
    u16 = nw == 8 and vec and a_kmajor and b_kmajor and 64 < groups <= 128
    return dict(nw=nw, u16=bool(u16), vec=bool(vec))


def pst_epi(b_kmajor, act, preact, dact_arg, dact):
    """pst_epi (gemm_pst.hip): the persistent kernel's epilogue variant, or -1."""
    if dact_arg:
        return (2 if dact == 1 else 4) if (not b_kmajor and act == ACT_NONE and not preact and dact in (1, 3)) else -1
    if act == ACT_SWISH:
        return 1 if b_kmajor else -1
    if act == ACT_SWISH_D:
        return 3 if (b_kmajor and preact) else -1
    return 0 if (act == ACT_NONE and not preact) else -1


def pst_wanted(M, N, K, lda, ldb, b_kmajor, offA, offB, epi, slots):
    """gemm_pst_wanted (the 32-bit window conditions are far from any shape used here and left out)."""
    if epi < 0 or K > 1024:
        return False
    if K % 32 or K < (5 if epi in (2, 4) else 4 if epi in (1, 3) else 3) * 32 or M % 128 or N <= 0:
        return False
    if offA % 4 or offB % 4 or lda % 4 or ldb % 4:
        return False
    return slots > 0 and (M // 128) * ceil_div(N, 128) > slots


def gemm_route(M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, batch1=1, batch2=1, strides=((0, 0), (0, 0), (0, 0)), off=None, epi=None, mode=0,
               slots=512):
    """gemm_f32_ex restated.  strides = ((sA1, sA2), (sB1, sB2), (sC1, sC2)) in floats; off = floats past a 16-byte boundary of
    {A, B, C, bias, addend, dact, preact} (absent = aligned); epi = {bias, addend, dact, act, preact, asum: present?, alpha}.
    Returns dict(family = 0 classic / 1 persistent / 2 small / 3 bf16x3 / None (no launch), kind = 'classic' | 'uneven' | 'small' | 'pst',
    and per kind: vec, cvec, splitk, k_per_split, rvec, ktiles = [(full k-tiles, tail) per split] | nw, u16, vec | epi)."""
    off = dict(off or {})
    epi = dict(epi or {})
    o = lambda name: off.get(name, 0) % 4
    has = lambda name: bool(epi.get(name))
    act, dact, alpha = epi.get("act", ACT_NONE), epi.get("dact", 0), epi.get("alpha", 1.0)
    (sA1, sA2), (sB1, sB2), (sC1, sC2) = strides
    batch = batch1 * batch2
    if M <= 0 or N <= 0 or batch <= 0:
        return dict(family=None, kind="nothing")
    assert not (has("addend") and dact), "addend and dact are mutually exclusive"
    assert not has("asum") or (not a_kmajor and batch == 1 and K > 0)
    if a_kmajor and batch == 1 and not has("asum") and not has("addend") and mode == 0:
        e = pst_epi(b_kmajor, act, has("preact"), dact != 0, dact)
        if pst_wanted(M, N, K, lda, ldb, b_kmajor, o("A"), o("B"), e, slots):
            return dict(family=FAMILY_PST, kind="pst", epi=e)
    if small_wanted(M, N, K, batch, lda, ldb, a_kmajor, b_kmajor):
        return dict(family=FAMILY_SMALL, kind="small", **small_instance(K, lda, ldb, a_kmajor, b_kmajor, o("A"), o("B")))
    big = FAMILY_BF3 if mode == 1 else FAMILY_CLASSIC
    tiles_m, tiles_n = ceil_div(M, BM), ceil_div(N, BN)
    t = tiles_m * tiles_n
    if (not a_kmajor and not b_kmajor and batch == 1 and not has("bias") and not has("preact") and not has("addend") and not dact
            and act == ACT_NONE and alpha == 1.0 and 256 < t <= 496 and K >= 4096 and K % 8 == 0 and M % 4 == 0 and N % 4 == 0
            and lda % 4 == 0 and ldb % 4 == 0 and o("A") == 0 and o("B") == 0):
        K1 = (K * t * 966 // (512 * 1000) + 31) // 32 * 32
        if K - K1 >= 256:
            return dict(family=big, kind="uneven", K1=K1, rvec=bool(ldc % 4 == 0 and o("C") == 0))
    splitk, kps = 1, ceil_div(K if K > 0 else 1, BK) * BK
    tiles = t * batch
    few = tiles <= 64 and K >= 256
    if batch == 1 and tiles < 192 and (K >= 1024 or few):
        s = min(slots_splitk() // tiles, K // 64 if few else K // 256, 32)
        if few and K < 1024 and s < 4:
            s = 1
        if s >= 2:
            kps2 = ceil_div(ceil_div(K, s), BK) * BK
            if ceil_div(K, kps2) >= 2:
                splitk, kps = ceil_div(K, kps2), kps2

    def vec_ok(name, ld, s1, s2, kmajor, outer):
        if o(name) or ld % 4 or (batch1 > 1 and s1 % 4) or (batch2 > 1 and s2 % 4):
            return False
        return K % 4 == 0 if kmajor else outer % 4 == 0

    vec_any = vec_ok("A", lda, sA1, sA2, a_kmajor, M) and vec_ok("B", ldb, sB1, sB2, b_kmajor, N)
    vec = vec_any and K % 8 == 0 and K >= (16 if mode == 1 else BK)
    if splitk > 1:
        cvec = N % 4 == 0
    else:
        cvec = (N % 4 == 0 and o("C") == 0 and ldc % 4 == 0 and (batch1 <= 1 or sC1 % 4 == 0) and (batch2 <= 1 or sC2 % 4 == 0)
                and not (has("bias") and o("bias")) and not (has("preact") and o("preact")) and not (has("addend") and o("addend"))
                and not (dact and o("dact")))
    r = dict(family=big, kind="classic", vec=bool(vec), cvec=bool(cvec), splitk=splitk, k_per_split=kps, cs=has("asum"),
             layout=("k" if a_kmajor else "o") + ("k" if b_kmajor else "o"), tiles_m=tiles_m, tiles_n=tiles_n)
    if splitk > 1:
        r["rvec"] = bool(cvec and ldc % 4 == 0 and o("C") == 0 and not (has("addend") and o("addend")) and not (has("preact") and o("preact"))
                         and not (dact and o("dact")))
    r["ktiles"] = [((min(K, (i + 1) * kps) - i * kps) // BK, (min(K, (i + 1) * kps) - i * kps) % BK) for i in range(splitk)]
    return r


def slots_splitk():
    """The split-K planner's slot count (gemm.hip: 512, two blocks on each of 256 CUs; a constant there, not a device query)."""
    return 512


def wgrad_chunk(K):
    c = ceil_div(ceil_div(K, 4), 32) * 32
    return max(c, 1024)


def wgrad_route(M, N, K, offs=(0, 0, 0)):
    """gemm_f32_wgrad_group_ok + wgrad_chunk: dict(group = queued by the deferred-dW queue?, chunk, splitk, ktiles)."""
    ok = (M > 0 and N > 0 and K >= 4096 and K % 8 == 0 and M % 4 == 0 and N % 4 == 0 and not any(x % 4 for x in offs)
          and ceil_div(M, BM) * ceil_div(N, BN) <= 256)
    c = wgrad_chunk(K)
    n = ceil_div(K, c)
    return dict(group=bool(ok), chunk=c, splitk=n, ktiles=[((min(K, (i + 1) * c) - i * c) // BK, (min(K, (i + 1) * c) - i * c) % BK) for i in range(n)])


def group_launches(n_jobs):
    """gemm_f32_wgrad_group: more than GEMM_GROUP_MAX jobs go out as several launches."""
    return ceil_div(n_jobs, GEMM_GROUP_MAX)


def pair_route(rows, inf, outf, have_dx=True, have_dw=True, addend=False, dact=0, mode=0):
    """linear_backward + gemm_f32_linear_backward_small: 'pair' (one launch, not counted by any family) or 'two' (the dX and dW GEMMs)."""
    if not (have_dx and have_dw) or (addend and dact) or mode != 0 or rows <= 0 or inf <= 0 or outf <= 0:
        return "two"
    dx_small = small_wanted(rows, inf, outf, 1, outf, inf, True, False)
    dw_small = small_wanted(outf, inf, rows, 1, outf, inf, False, False)
    return "pair" if dx_small and dw_small else "two"


def pair_instance(rows, outf, off_dO=0):
    g0, g1 = (outf + 15) >> 4, (rows + 15) >> 4
    return dict(nw=8 if (g0 >= 8 or g1 >= 8) else 4, vec=bool(outf % 4 == 0 and off_dO % 4 == 0))


def route_id(r):
    """A case id from a route: the kernel instance in words."""
    if r["kind"] == "small":
        return f"small-nw{r['nw']}" + ("-u16" if r["u16"] else "") + ("-vec" if r["vec"] else "-scalar")
    if r["kind"] == "pst":
        return f"pst-epi{r['epi']}"
    if r["kind"] == "uneven":
        return "uneven" + ("" if r["family"] == 0 else "-bf3")
    if r["kind"] == "nothing":
        return "nothing"
    s = ("bf3-" if r["family"] == FAMILY_BF3 else "classic-") + r["layout"] + ("-vec" if r["vec"] else "-scalar") + ("-cvec" if r["cvec"] else "-cscalar")
    if r["cs"]:
        s += "-cs"
    if r["splitk"] > 1:
        s += f"-split{r['splitk']}" + ("-rvec" if r["rvec"] else "-rscalar")
    return s
