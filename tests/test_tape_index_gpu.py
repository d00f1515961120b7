"""GPU: the indexing half of the Tensor tape (ABI 224: csrc/tensor_index.hip through neunet_hip/tensor_index.py AND through the C ABI)
against NumPy.  Copies, selects and comparisons are exact: every check is bit equality.  The one inexact family, the gradient of a
broadcast `where` operand, is held to the sum bound of tests/tape_ref.py.  Outputs handed to the C ABI are pre-filled with 0xFF bytes (a
NaN as float32, 255 as a byte), so an element a kernel never wrote shows; the tier a case is aimed at is read back from
nnhipTensorOpsLastTier.  Shapes are the smallest that can still go wrong: sizes around the 4-per-lane tier, broadcasting on either side,
pointers 4 bytes past a 16-byte boundary, every inner extent at which the gather changes tier."""
import ctypes

import numpy as np
import pytest

import index_ref as IR
import tape_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
TIER = IR.TIER
NP2T = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.bool_): torch.bool,
        np.dtype(np.uint8): torch.uint8}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def call(name, *args):
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    return call_hip_function(name, *args, get_current_stream_ptr())


def dev(a):
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(a.shape).cuda()      # (ascontiguousarray makes a 0-d array 1-d)


def host(t):
    return t.detach().cpu().numpy()


def T(a, **kw):
    """A device Tensor of exactly a's shape and dtype."""
    from neunet_hip import Tensor
    a = np.asarray(a)
    kw.setdefault("requires_grad", False)
    return Tensor(dev(a), device="cuda", dtype=a.dtype, **kw)


def i64(v):
    return (ctypes.c_int64 * max(len(v), 1))(*[int(x) for x in v])


def last_tier():
    from neunet_hip import _lib
    seg = ctypes.c_int64(0)
    return _lib.load_hip_function("nnhipTensorOpsLastTier")(ctypes.byref(seg)), seg.value


class Buf:
    """An operand inside its own allocation of 0xFF bytes: 64 bytes, `off` more (off = 4: the operand starts 4 bytes past a 16-byte
    boundary), the operand (`value`, or 0xFF when only (shape, dtype) is given), 64 bytes."""

    def __init__(self, value, off=0, dtype=None):
        if dtype is not None:
            shape, dt = tuple(value), np.dtype(dtype)
        else:
            value = np.asarray(value)
            shape, dt = value.shape, value.dtype
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        self.whole = torch.full((64 + off + nbytes + 64,), 255, device="cuda", dtype=torch.uint8)
        self.lo, self.hi = 64 + off, 64 + off + nbytes
        self.t = self.whole[self.lo:self.hi].view(NP2T[dt]).view(shape)
        if dtype is None:
            self.t.copy_(dev(value))
        assert self.t.data_ptr() % 16 == off % 16 and self.t.is_contiguous()

    def intact(self):
        w = host(self.whole)
        return bool((w[:self.lo] == 255).all() and (w[self.hi:] == 255).all())

    def host(self):
        return host(self.t)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.bool_ else a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    np.testing.assert_array_equal(bits(got), bits(ref), err_msg=str(what))


def strides_of(shape, out_shape):
    return R.element_strides(shape, out_shape)


def f32_values(rng, shape):
    """Halves (plenty of ties) with the specials of the issue sprinkled in: NaN, +-0, +-inf, denormals."""
    a = (np.round(rng.standard_normal(shape) * 2) / 2).astype(np.float32)
    flat = a.reshape(-1)
    pos = rng.permutation(flat.size)[:min(flat.size, len(IR.F32_SPECIALS))]
    flat[pos] = IR.F32_SPECIALS[:len(pos)]
    return a


# ===================================================================================================== comparisons
@pytest.mark.parametrize("off", [0, 4], ids=["aligned", "off4"])
@pytest.mark.parametrize("n", IR.COMPARE_SIZES)
def test_compare_same_shape_every_kind(hip, n, off):
    """C ABI, float32, two tensors and a scalar on either side: four results per lane when n % 4 == 0 and the inputs are 16-byte
    aligned, the general tier otherwise.  Both operands hold the specials at the same positions in places (NaN against NaN, -0 against 0)."""
    rng = np.random.default_rng(n)
    a, b = f32_values(rng, (n,)), f32_values(rng, (n,))
    b[: n // 2] = a[: n // 2]
    if n >= 4:
        a[1], b[1] = np.float32(-0.0), np.float32(0.0)
        a[2], b[2] = np.float32(np.nan), np.float32(np.nan)
    A, B = Buf(a, off), Buf(b, off)
    want = TIER["vec4"] if (n % 4 == 0 and off == 0) else TIER["general"]
    with np.errstate(invalid="ignore"):
        for kind, op in enumerate(IR.COMPARE):
            out = Buf((n,), 0, np.bool_)
            call("nnhipCompare", kind, out.t, A.t, B.t, 0.0, 0, 0, 0, 1, i64([n]), i64([1]), i64([1]))
            assert last_tier()[0] == want and out.intact()
            same_bits(out.host(), IR.NP_COMPARE[op](a, b), f"{op} n={n}")
            for s in (0.5, 0.0, float("nan"), 0.1):         # 0.1 is rounded to float32 first (NumPy 2)
                out = Buf((n,), 0, np.bool_)
                call("nnhipCompare", kind, out.t, A.t, None, s, 0, 0, 0, 1, i64([n]), i64([1]), None)
                assert last_tier()[0] == want and out.intact()
                same_bits(out.host(), IR.NP_COMPARE[op](a, np.float32(s)), f"{op} tensor-scalar {s}")
                out = Buf((n,), 0, np.bool_)
                call("nnhipCompare", kind, out.t, None, A.t, s, 0, 0, 0, 1, i64([n]), None, i64([1]))
                same_bits(out.host(), IR.NP_COMPARE[op](np.float32(s), a), f"{op} scalar-tensor {s}")
    assert A.intact() and B.intact() and np.array_equal(bits(A.host()), bits(a))


@pytest.mark.parametrize("sa,sb", IR.COMPARE_BROADCAST, ids=[f"{a}o{b}" for a, b in IR.COMPARE_BROADCAST])
def test_compare_and_logical_broadcast_through_the_tape(hip, sa, sb):
    rng = np.random.default_rng(len(sa) * 7 + len(sb))
    a, b = f32_values(rng, sa), f32_values(rng, sb)
    ta, tb = T(a), T(b)
    with np.errstate(invalid="ignore"):
        for op in IR.COMPARE:
            y = getattr(ta, op)(tb)
            assert last_tier()[0] == TIER["general"]
            assert y.dtype == np.bool_ and y.data.dtype == torch.bool and y.requires_grad is False and y.args is None and y.op == op
            same_bits(host(y.data), IR.NP_COMPARE[op](a, b), op)
        same_bits(host((ta == tb).data), a == b)
        same_bits(host((ta != tb).data), a != b)
        same_bits(host((ta < tb).data), a < b)
        same_bits(host((0.5 < ta).data), 0.5 < a)             # reflected: Tensor.__gt__
        same_bits(host((ta <= 0.1).data), a <= np.float32(0.1))
        same_bits(host(ta.logical_and(tb).data), np.logical_and(a, b))          # a NaN is true, -0.0 is false
        same_bits(host(ta.logical_or(tb).data), np.logical_or(a, b))
        same_bits(host(((ta > 0) & (tb <= 0)).data), (a > 0) & (b <= 0))
        same_bits(host(((ta > 0) | ~(tb <= 0)).data), (a > 0) | ~(b <= 0))
        same_bits(host(hip.logical_not(ta).data), np.logical_not(a))


def test_compare_integer_and_bool_tensors(hip):
    """int32 at +-(2^31 - 1) against Python ints inside and outside int32 (compared in int64) and against a Python float (compared in
    double); int64 at 2^53 + 1 against the Python ints 2^53 and 2^53 + 1 (exact) and the float 2.0^53 (NumPy converts the tensor to
    double: equal); bool against bool, int and float."""
    big = 2 ** 31 - 1
    i = np.array([big, -big, -big - 1, 0, 1, -1, 7, big - 1], np.int32)
    ti = T(i)
    for op in IR.COMPARE:
        f = IR.NP_COMPARE[op]
        for s in (big, -big, big + 1, -big - 2, 2 ** 40, 0, 1):
            same_bits(host(getattr(ti, op)(s).data), f(i, s), f"{op} int32 vs {s}")
        assert last_tier()[0] == TIER["vec4"]
        for s in (0.5, -0.5, float(big), 2.0 ** 31, float("nan")):
            same_bits(host(getattr(ti, op)(s).data), f(i, s), f"{op} int32 vs {s}")
        same_bits(host(getattr(ti, op)(T(i[::-1].copy())).data), f(i, i[::-1]), op)
    p = 2 ** 53
    l = np.array([p + 1, p, p - 1, -(p + 1), 2 ** 62 + 1, 0, 3], np.int64)
    tl = T(l)
    for op in IR.COMPARE:
        f = IR.NP_COMPARE[op]
        for s in (p + 1, p, 2 ** 62 + 1, 2 ** 62):
            same_bits(host(getattr(tl, op)(s).data), f(l, s), f"{op} int64 vs {s}")
        same_bits(host(getattr(tl, op)(2.0 ** 53).data), f(l, 2.0 ** 53), f"{op} int64 vs 2.0^53")
        same_bits(host(getattr(tl, op)(T(l[::-1].copy())).data), f(l, l[::-1]), op)
    assert last_tier()[0] == TIER["general"]                   # 7 elements
    assert not host((tl == p).data)[0] and host((tl == p + 1).data)[0] and host((tl == 2.0 ** 53).data)[0]
    m, k = np.array([True, False, True, True]), np.array([True, True, False, True])
    tm, tk = T(m), T(k)
    for op in IR.COMPARE:
        f = IR.NP_COMPARE[op]
        same_bits(host(getattr(tm, op)(tk).data), f(m, k), op)
        same_bits(host(getattr(tm, op)(True).data), f(m, True), op)
        same_bits(host(getattr(tm, op)(1).data), f(m, 1), op)
        same_bits(host(getattr(tm, op)(0.5).data), f(m, 0.5), op)
    same_bits(host((tm & tk).data), m & k)
    same_bits(host((tm | tk).data), m | k)
    same_bits(host((~tm).data), ~m)
    same_bits(host(tm.logical_and(ti[:4]).data), np.logical_and(m, i[:4]))       # operands of different dtypes
    for s in (np.int64(big), np.int64(2 ** 40), np.int8(-1), np.float32(0.5), np.float64(-0.5), np.bool_(True)):      # NumPy scalars promote
        same_bits(host((ti >= s).data), i >= s, f"int32 vs {type(s).__name__}")
    f = np.array([0.1, 0.5, 16777216.0, -1.0], np.float32)
    for s in (np.float32(0.1), np.int16(-1), np.bool_(True)):
        same_bits(host((T(f) == s).data), f == s, f"float32 vs {type(s).__name__}")
    with pytest.raises(NotImplementedError):
        T(f) == np.float64(0.1)                                 # NumPy would compare in float64: a mixed-dtype comparison
    with pytest.raises(NotImplementedError, match="different dtypes"):
        ti == T(i.astype(np.float32))
    with pytest.raises(NotImplementedError, match="different dtypes"):
        tl > ti
    assert (ti == None) is False and ti.equal("x") is NotImplemented and hash(ti) == object.__hash__(ti)     # noqa: E711


@pytest.mark.parametrize("n,off", [(4, 0), (257, 0), (1028, 0), (1028, 4)])
def test_logical_tiers_abi(hip, n, off):
    rng = np.random.default_rng(n + off)
    a = f32_values(rng, (n,))
    b = rng.integers(-1, 2, n).astype(np.int32)
    A, B = Buf(a, off), Buf(b, off)
    want = TIER["vec4"] if (n % 4 == 0 and off == 0) else TIER["general"]
    for kind, f in enumerate((np.logical_and, np.logical_or)):
        out = Buf((n,), 0, np.bool_)
        call("nnhipLogical", kind, out.t, A.t, B.t, 0, 1, 1, i64([n]), i64([1]), i64([1]))
        assert last_tier()[0] == want and out.intact()
        same_bits(out.host(), f(a, b))
    out = Buf((n,), 0, np.bool_)
    call("nnhipLogical", 2, out.t, A.t, None, 0, 0, 1, i64([n]), i64([1]), None)
    assert last_tier()[0] == want and out.intact()
    same_bits(out.host(), np.logical_not(a))


# ===================================================================================================== where
@pytest.mark.parametrize("cdt", [np.bool_, np.int32, np.float32], ids=["bool", "int32", "float32"])
@pytest.mark.parametrize("n", [1028, 1027])
def test_where_forward_same_shape(hip, n, cdt):
    rng = np.random.default_rng(n)
    a, b = f32_values(rng, (n,)), f32_values(rng, (n,))
    c = f32_values(rng, (n,)) if cdt == np.float32 else rng.integers(0, 2, n).astype(cdt)
    truth = c != 0
    for off in (0, 4):
        A, B, C, out = Buf(a, off), Buf(b, off), Buf(c, 0), Buf((n,), 0, np.float32)
        call("nnhipWhereForward", out.t, C.t, IR.DT[np.dtype(cdt)], A.t, B.t, 0.0, 0.0, 1, i64([n]), i64([1]), i64([1]), i64([1]))
        assert last_tier()[0] == (TIER["vec4"] if n % 4 == 0 and off == 0 else TIER["general"]) and out.intact()
        same_bits(out.host(), np.where(truth, a, b))
    for sa, sb in ((2.5, None), (None, -1e9), (2.5, -1e9)):
        out = Buf((n,), 0, np.float32)
        call("nnhipWhereForward", out.t, C.t, IR.DT[np.dtype(cdt)], A.t if sa is None else None, B.t if sb is None else None,
             sa or 0.0, sb or 0.0, 1, i64([n]), i64([1]), i64([1]), i64([1]))
        assert out.intact()
        same_bits(out.host(), np.where(truth, a if sa is None else np.float32(sa), b if sb is None else np.float32(sb)))


def test_where_broadcast_through_the_tape(hip):
    """cond [2,1,5,5] against [2,3,5,5] (the notebook's mask against the scores), both orders, the function form with scalars."""
    rng = np.random.default_rng(5)
    a, b = f32_values(rng, (2, 3, 5, 5)), f32_values(rng, (5,))
    m = rng.integers(0, 2, (2, 1, 5, 5)).astype(np.int32)
    ta, tb, tm = T(a), T(b), T(m)
    y = ta.where(tm == 0, tb)
    assert last_tier()[0] == TIER["general"] and y.dtype == np.float32 and y.op == "where" and y.requires_grad is False
    same_bits(host(y.data), np.where(m == 0, a, b))
    same_bits(host(hip.where(tm == 0, -1e9, ta).data), np.where(m == 0, np.float32(-1e9), a))
    same_bits(host(hip.where(tm, ta, 0.25).data), np.where(m != 0, a, np.float32(0.25)))
    same_bits(host(hip.where(tm, 1.0, 0.0).data), np.where(m != 0, np.float32(1), np.float32(0)))
    same_bits(host(hip.where(T(m.astype(np.float32) * np.float32(np.nan)), ta, 0.0).data), np.where(np.isnan(m * np.float32(np.nan)), a, np.float32(0)))
    with pytest.raises(NotImplementedError):
        ta.where(T(m.astype(np.int64)), tb)
    with pytest.raises(NotImplementedError):
        T(m).where(tm, tb)                                   # an int32 value operand


WHERE_OPERANDS = ["NF", "F", "N1", "1"]


@pytest.mark.parametrize("cdt", [np.bool_, np.int32, np.float32], ids=["bool", "int32", "float32"])
@pytest.mark.parametrize("N,F", IR.WHERE_BACKWARD_SHAPES)
def test_where_backward_operand_shapes(hip, N, F, cdt):
    """Each gradient in the operand's OWN shape, summed over its broadcast axes inside the launch; g holds inf and NaN exactly where the
    OTHER branch supplied the value, so any multiply in place of the select would leave a NaN."""
    rng = np.random.default_rng(N * F)
    shapes = {"NF": (N, F), "F": (F,), "N1": (N, 1), "1": (1,)}
    c = (rng.random((N, F)) < 0.5)
    c[:, 1] = True
    c[0, :] = False
    cond = c.astype(cdt) if cdt != np.float32 else np.where(c, np.float32(np.nan), np.float32(-0.0)).astype(np.float32)   # NaN is true, -0 false
    C = dev(cond)
    full, st = (N, F), lambda s: i64(strides_of(s, (N, F)))  # noqa: E731
    worst = 0.0
    for which in (0, 1):                                     # the gradient of a (taken where cond holds), then of b
        owns = c if which == 0 else ~c
        g = rng.standard_normal((N, F)).astype(np.float32)
        poison = ~owns & (rng.random((N, F)) < 0.3)
        g[poison] = np.where(rng.random(int(poison.sum())) < 0.5, np.float32(np.inf), np.float32(np.nan))
        G = dev(g)
        local = np.where(owns, g, np.float32(0))
        for name in WHERE_OPERANDS:
            s = shapes[name]
            out = Buf(s, 0, np.float32)
            args = (out.t, None) if which == 0 else (None, out.t)
            strides = (st(s), None) if which == 0 else (None, st(s))
            call("nnhipWhereBackward", *args, G, C, IR.DT[np.dtype(cdt)], 2, i64(full), st(full), *strides)
            got, axes = out.host(), IR.reduced_axes(s, full)
            assert out.intact() and np.isfinite(got).all(), (name, which)
            tier, seg = last_tier()
            if axes is None:
                assert tier == (TIER["ew-general"] if cdt == np.bool_ or F % 4 else TIER["ew-vec2d"]), (name, tier)
                same_bits(got, local, f"{name} exact")
                continue
            rt, S = R.route("reduce", shape=full, axis=axes)
            assert (tier, seg) == (TIER["red-" + rt], S), (name, tier, seg, rt, S)
            ref = R.f64(local).sum(axis=axes, keepdims=True).reshape(s)
            bound = R.sum_bound(local, axes, keepdims=True).reshape(s)
            err = np.abs(got.astype(np.float64) - ref) / bound
            worst = max(worst, float(err.max()))
            assert (err <= 1.0).all(), (name, which, float(err.max()))
    print(f"\n[where backward {N}x{F} {np.dtype(cdt)}] largest error / bound {worst:.3f}")


def test_where_backward_through_the_tape(hip):
    """a [4,1] and b [5] against a [4,5] condition through Tensor.where: each gradient in its operand's own shape, within the sum bound
    of the reduction that forms it (tests/tape_ref.py: sum_bound on the selected terms of the branch under test); then the function form
    with a scalar on the other side (no gradient for the scalar, a one-sided request)."""
    rng = np.random.default_rng(9)
    a, b, h = rng.standard_normal((4, 1)).astype(np.float32), rng.standard_normal((5,)).astype(np.float32), f32_values(rng, (4, 5))
    with np.errstate(invalid="ignore"):
        truth = h > 0
    g = rng.standard_normal((4, 5)).astype(np.float32)

    def check(grad, owns, shape, what):
        local = np.where(owns, g, np.float32(0))
        axes = IR.reduced_axes(shape, (4, 5))
        ref = R.f64(local).sum(axis=axes, keepdims=True).reshape(shape)
        bound = R.sum_bound(local, axes, keepdims=True).reshape(shape)
        got = host(grad)
        assert got.shape == tuple(shape), what
        err = np.abs(got.astype(np.float64) - ref) / bound
        assert (err <= 1.0).all(), (what, float(err.max()))
        return float(err.max())

    ta, tb = T(a, requires_grad=True), T(b, requires_grad=True)
    y = ta.where(T(h) > 0, tb)
    assert y.requires_grad and y.args[0] is ta and y.args[2] is tb
    y.backward(dev(g))
    r = [check(ta.grad, truth, a.shape, "dA [4,1]"), check(tb.grad, ~truth, b.shape, "dB [5]")]
    tc = T(a, requires_grad=True)
    z = hip.where(T(h) > 0, 2.0, tc)
    z.backward(dev(g))
    r.append(check(tc.grad, ~truth, a.shape, "dB [4,1] beside a scalar"))
    print(f"\n[where through the tape] error / bound: dA {r[0]:.3f}, dB {r[1]:.3f}, beside a scalar {r[2]:.3f}")


# ===================================================================================================== basic keys
BASIC = IR.basic_cases()


@pytest.mark.parametrize("shape,key", BASIC, ids=[f"{s}{IR.key_id(k)}" for s, k in BASIC])
def test_getitem_basic_forward_every_element_size(hip, shape, key):
    from neunet_hip.tensor_index import canonical_index
    rng = np.random.default_rng(len(shape))
    n = int(np.prod(shape))
    for dt in (np.float32, np.int32, np.int64, np.bool_):
        x = f32_values(rng, shape) if dt == np.float32 else (rng.integers(0, 2, shape).astype(dt) if dt == np.bool_ else
                                                              (rng.integers(-2 ** 30, 2 ** 30, shape) * (2 ** 31 + 1 if dt == np.int64 else 1)).astype(dt))
        y = T(x)[key]
        assert y.dtype == np.dtype(dt) and y.data.is_contiguous() and y.op == "getitem" and y.requires_grad is False
        same_bits(host(y.data), x[key], f"{np.dtype(dt)}")
        # the C ABI on an offset base, into a pre-filled output
        offset, out_shape, strides = canonical_index(shape, key)
        X, out = Buf(x, 0), Buf(out_shape, 0, dt)
        call("nnhipSliceForward", out.t, X.t, offset, IR.DT[np.dtype(dt)], len(out_shape), i64(out_shape), i64(strides))
        assert out.intact() and X.intact()
        if x[key].size:
            same_bits(out.host(), np.array(x[key]))
            tier = last_tier()[0]
            assert tier in ((TIER["ew-vec2d"], TIER["ew-general"]) if np.dtype(dt).itemsize == 4 else (TIER["general"],)), tier
        else:
            assert (host(out.whole) == 255).all()
    assert n > 0


@pytest.mark.parametrize("shape,key", BASIC, ids=[f"{s}{IR.key_id(k)}" for s, k in BASIC])
def test_getitem_basic_backward_writes_every_element_once(hip, shape, key):
    from neunet_hip.tensor_index import canonical_lattice
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape).astype(np.float32)
    sel = x[key]
    g = rng.standard_normal(sel.shape).astype(np.float32)
    ref = IR.getitem_backward(shape, key, g)
    start, step, count = canonical_lattice(shape, key)
    dX = Buf(shape, 0, np.float32)
    G = Buf(g, 0) if g.size else None
    call("nnhipSliceBackward", dX.t, G.t if G is not None else None, len(shape), i64(shape), i64(start), i64(step), i64(count))
    assert dX.intact() and last_tier()[0] in (TIER["slice-vec"], TIER["slice-scalar"])
    same_bits(dX.host(), ref)
    # through the tape: a second node on the same leaf accumulates into its gradient (apply_grad)
    t = T(x, requires_grad=True)
    y = t[key]
    assert y.requires_grad
    if g.size:
        y.backward(dev(g))
        same_bits(host(t.grad), ref)
        t[key].backward(dev(g))
        same_bits(host(t.grad), ref + ref)


def test_slice_backward_vector_tier_and_offsets(hip):
    """float4 stores when the innermost group is taken whole (x[1:-1], x[:, -1] of a 3-d tensor, x[::2] of rows of 8); one element per lane
    for x[:, ::2], for a last extent that is no multiple of 4 and for bases 4 bytes past a 16-byte boundary."""
    rng = np.random.default_rng(3)
    cases = [((6, 8), (slice(1, -1),), "slice-vec"), ((4, 5, 8), (slice(None), -1), "slice-vec"), ((6, 8), (slice(None, None, -2),), "slice-vec"),
             ((6, 8), (slice(None), slice(None, None, 2)), "slice-scalar"), ((6, 7), (slice(1, -1),), "slice-scalar"), ((5, 260), (slice(None), slice(3, 259)), "slice-scalar"),
             ((3, 260), (1,), "slice-vec")]
    from neunet_hip.tensor_index import canonical_lattice
    for shape, key, tier in cases:
        for off in (0, 4):
            g = rng.standard_normal(np.zeros(shape)[key].shape).astype(np.float32)
            dX, G = Buf(shape, off, np.float32), Buf(g, off)
            call("nnhipSliceBackward", dX.t, G.t, len(shape), i64(shape), *[i64(v) for v in canonical_lattice(shape, key)])
            assert last_tier()[0] == (TIER[tier] if off == 0 else TIER["slice-scalar"]), (shape, key, off)
            assert dX.intact()
            same_bits(dX.host(), IR.getitem_backward(shape, key, g))


def test_getitem_refusals(hip):
    x = T(np.zeros((3,) * 8, np.float32))
    with pytest.raises(ValueError, match="axis groups"):
        x[(slice(None, None, 2),) * 8]
    y = T(np.zeros((3, 4), np.float32))
    with pytest.raises(IndexError):
        y[3]
    with pytest.raises(IndexError):
        y[0, 0, 0]
    with pytest.raises(NotImplementedError, match="where"):
        y[y > 0]
    with pytest.raises(NotImplementedError, match="separated"):
        T(np.zeros((3, 4, 5), np.float32))[[0, 1], :, [0, 1]]
    with pytest.raises(IndexError, match="out of bounds"):
        y[[0, 3]]                                            # a host index array is range-checked before any launch
    with pytest.raises(IndexError, match="out of bounds"):
        y[:, [-5]]


# ===================================================================================================== flip
@pytest.mark.parametrize("axis", IR.FLIP_AXES, ids=str)
def test_flip_forward_backward(hip, axis):
    rng = np.random.default_rng(11)
    for shape in ((2, 3, 4), (5, 7, 8)):
        x = rng.standard_normal(shape).astype(np.float32)
        t = T(x, requires_grad=True)
        y = t.flip(axis)
        assert y.op == "flip" and y.requires_grad
        same_bits(host(y.data), np.ascontiguousarray(np.flip(x, axis)))
        g = rng.standard_normal(shape).astype(np.float32)
        y.backward(dev(g))
        same_bits(host(t.grad), np.ascontiguousarray(np.flip(g, axis)))
        same_bits(host(hip.flip(T(x.astype(np.int64) * 2 ** 33), axis).data), np.ascontiguousarray(np.flip(x.astype(np.int64) * 2 ** 33, axis)))
    with pytest.raises(ValueError):
        T(np.zeros((2, 3), np.float32)).flip((0, 0))
    with pytest.raises(ValueError):
        T(np.zeros((2, 3), np.float32)).flip(2)


# ===================================================================================================== integer-array indexing
GATHER_TIER = {1: "element", 5: "general", 16: "row-vec", 67: "row", 260: "row-vec"}


@pytest.mark.parametrize("idt", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("inner", IR.GATHER_INNER)
def test_gather_and_assign_tiers_one_and_two_arrays(hip, inner, idt):
    """x [2, 6, 5, inner] (inner == 1: [2, 6, 5]); k = 1: x[:, ids] on axis 1; k = 2: x[:, i, j] with a 2-d broadcast pair.  Device index
    tensors with negative entries and repeats; forward bit for bit, the backward assigns (last occurrence in C order) and writes every
    element of dX once."""
    rng = np.random.default_rng(inner)
    shape = (2, 6, 5) + (() if inner == 1 else (inner,))
    x = rng.standard_normal(shape).astype(np.float32)
    ids = np.array([5, -6, 2, 2, -1, 0, 2], idt)
    i2, j2 = np.array([[0], [-1], [3]], idt), np.array([[4, -5, 4, 1]], idt)
    for key_np, key_t in (((slice(None), ids), (slice(None), T(ids))), ((slice(None), i2, j2), (slice(None), T(i2), T(j2))),
                          ((slice(None), ids[:1]), (slice(None), T(ids[:1])))):                                       # M = 1
        t = T(x, requires_grad=True)
        y = t[key_t]
        k = len(key_np) - 1
        want = GATHER_TIER[inner] if k == 2 or inner > 1 else "general"        # k = 1 at inner == 1 leaves the 5-axis inside: inner = 5
        if k == 1 and inner > 1:
            want = "row-vec" if (5 * inner) % 4 == 0 else "row"
        assert last_tier()[0] == TIER[want], (inner, k, last_tier())
        same_bits(host(y.data), x[key_np])
        g = rng.standard_normal(y.shape).astype(np.float32)
        y.backward(dev(g))
        same_bits(host(t.grad), IR.getitem_backward(shape, key_np, g))
        # an int32 tensor through the same kernels (by bits), host index arrays
        xi = (x * 1000).astype(np.int32)
        same_bits(host(T(xi)[tuple(np.asarray(v) if isinstance(v, np.ndarray) else v for v in key_np)].data), xi[key_np])
    for dt in (np.int64, np.bool_):
        xv = (x * 1000).astype(np.int64) * 2 ** 20 if dt == np.int64 else x > 0
        same_bits(host(T(xv)[:, T(ids)].data), xv[:, ids])
        same_bits(host(T(xv)[:, T(i2), T(j2)].data), xv[:, i2, j2])


def test_gather_keys_of_the_notebooks(hip):
    rng = np.random.default_rng(2)
    w = rng.standard_normal((15, 64)).astype(np.float32)
    ids = rng.integers(0, 15, (3, 7))
    tw = T(w, requires_grad=True)
    y = tw[T(ids.astype(np.int32))]
    assert last_tier()[0] == TIER["row-vec"] and y.shape == (3, 7, 64)
    same_bits(host(y.data), w[ids])
    g = rng.standard_normal((3, 7, 64)).astype(np.float32)
    y.backward(dev(g))
    same_bits(host(tw.grad), IR.getitem_backward(w.shape, ids, g))
    logp = rng.standard_normal((33, 10)).astype(np.float32)
    lab = rng.integers(0, 10, 33)
    tl = T(logp, requires_grad=True)
    picked = tl[hip.arange(33, dtype=np.int64, device="cuda"), T(lab)]
    assert last_tier()[0] == TIER["element"]
    same_bits(host(picked.data), logp[np.arange(33), lab])
    picked.backward(dev(np.ones(33, np.float32)))
    same_bits(host(tl.grad), IR.getitem_backward(logp.shape, (np.arange(33), lab), np.ones(33, np.float32)))
    x = rng.standard_normal((3, 4, 5)).astype(np.float32)
    tx = T(x)
    for key in ((Ellipsis, [0, 0, 3]), (slice(None), [1, 3, 1]), (slice(1, None), [0, 2]), (1, [0, 2]), (slice(None), 2, [0, 4, -1]), ([2, 0, 2],),
                (slice(None, None, -1), slice(None), np.array([[1], [0]]))):
        same_bits(host(tx[key].data), x[key], IR.key_id(key))
    same_bits(host(tx[[]].data), x[[]])
    assert tx[:, []].shape == (3, 0, 5)


def test_index_assign_heavy_duplicates_and_stale_tables(hip):
    """64 indices into 3 rows: the last occurrence wins, identically over three reruns.  Then a large destination followed by a small
    one: the `last` table is refilled on every call, so no entry of the first call survives into the second."""
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 3, 64).astype(np.int32)
    g = rng.standard_normal((64, 20)).astype(np.float32)
    ref = IR.getitem_backward((3, 20), ids, g)
    ptr = lambda t: (ctypes.c_void_p * 4)(t.data_ptr(), 0, 0, 0)  # noqa: E731
    I, G = dev(ids), dev(g)
    first = None
    for _ in range(3):
        dX = Buf((3, 20), 0, np.float32)
        call("nnhipIndexAssign", dX.t, G, 0.0, 0, 0, 0, 1, ptr(I), 1, 1, i64([3]), 1, 64, 20)
        assert dX.intact() and last_tier()[0] == TIER["row-vec"]
        same_bits(dX.host(), ref)
        first = dX.host() if first is None else first
        same_bits(dX.host(), first)
    big_ids = dev(np.arange(5000, dtype=np.int32))
    big = Buf((5000, 1), 0, np.float32)
    call("nnhipIndexAssign", big.t, dev(np.ones((5000, 1), np.float32)), 0.0, 0, 0, 0, 1, ptr(big_ids), 1, 1, i64([5000]), 1, 5000, 1)
    assert last_tier()[0] == TIER["element"] and (big.host() == 1).all()
    small_ids = dev(np.array([2], np.int32))
    small = Buf((6, 1), 0, np.float32)
    call("nnhipIndexAssign", small.t, dev(np.full((1, 1), 7, np.float32)), 0.0, 0, 0, 0, 1, ptr(small_ids), 1, 1, i64([6]), 1, 1, 1)
    same_bits(small.host(), np.array([0, 0, 7, 0, 0, 0], np.float32).reshape(6, 1))
    # setitem form: untouched elements are left alone, a scalar value
    keep = Buf(np.arange(12, dtype=np.float32).reshape(6, 2), 0)
    call("nnhipIndexAssign", keep.t, None, 2.5, 0, 0, 0, 0, ptr(small_ids), 1, 1, i64([6]), 1, 1, 2)
    exp = np.arange(12, dtype=np.float32).reshape(6, 2)
    exp[2] = 2.5
    same_bits(keep.host(), exp)


def test_device_index_out_of_range_is_defined(hip):
    """A device index tensor is not range-checked (that would be a host read in the middle of a step): an element outside its axis reads
    as 0 and is skipped on the way back -- nnhipEmbeddingForward's rule, a bounds test inside the kernels."""
    rng = np.random.default_rng(6)
    for inner in (1, 5, 64):
        shape = (4,) + (() if inner == 1 else (inner,))
        x = rng.standard_normal(shape).astype(np.float32) + 3
        ids = np.array([1, 4, -5, 3, 100, -1], np.int64)
        ok = (ids >= -4) & (ids < 4)
        t = T(x, requires_grad=True)
        y = t[T(ids)]
        ref = np.zeros((6,) + shape[1:], np.float32)
        ref[ok] = x[ids[ok]]
        same_bits(host(y.data), ref)
        g = rng.standard_normal(y.shape).astype(np.float32)
        y.backward(dev(g))
        same_bits(host(t.grad), IR.getitem_backward(shape, ids[ok], g[ok]))
        z = T(x.copy())
        z[T(ids)] = 9.0
        exp = x.copy()
        exp[ids[ok]] = 9.0
        same_bits(host(z.data), exp)


# ===================================================================================================== __setitem__
def test_setitem_basic_keys_every_dtype(hip):
    rng = np.random.default_rng(8)
    for dt in (np.float32, np.int32, np.int64, np.bool_):
        mk = (lambda s: rng.standard_normal(s).astype(np.float32)) if dt == np.float32 else (lambda s: rng.integers(0, 2, s).astype(dt)) if dt == np.bool_ \
            else (lambda s: rng.integers(-1000, 1000, s).astype(dt))
        scalar = {np.float32: 2.5, np.int32: -7, np.int64: 2 ** 40 + 1, np.bool_: True}[dt]
        x = mk((5, 7, 4))
        t, ref = T(x), x.copy()
        for key, value in (((slice(None), slice(None, None, 2)), scalar), (1, mk((7, 4))), ((slice(None, None, -2), slice(1, 6, 3)), mk((4,))),
                           ((Ellipsis, 0), mk((5, 7))), ((slice(None), None, 2), mk((1, 4))), (slice(3, 3), scalar), ((-1, -1, -1), scalar),
                           ((slice(None), slice(1, 3)), mk((1, 5, 2, 4)))):
            t[key] = T(value) if isinstance(value, np.ndarray) else value
            assert last_tier()[0] == TIER["general"] or ref[key].size == 0
            ref[key] = value
            same_bits(host(t.data), ref, f"{np.dtype(dt)} {IR.key_id(key)}")
        v = mk((7, 4))
        t[0] = v.tolist()                                     # an array-like value
        ref[0] = v
        same_bits(host(t.data), ref, f"{np.dtype(dt)} list")
    pe = hip.zeros(6, 8, device="cuda")
    pos = hip.arange(0, 6, device="cuda")[:, None, ...]
    pe[:, 0::2] = (pos * 0.5).sin()
    pe[:, 1::2] = (pos * 0.5).cos()
    p = np.arange(6, dtype=np.float32)[:, None] * np.float32(0.5)
    assert np.allclose(host(pe.data)[:, 0::2], np.sin(p), atol=1e-6) and np.allclose(host(pe.data)[:, 1::2], np.cos(p), atol=1e-6)
    assert tuple(pe[None, ...][:, :4].shape) == (1, 4, 8)


def test_setitem_index_arrays_and_masks(hip):
    rng = np.random.default_rng(10)
    x = rng.standard_normal((5, 6, 4)).astype(np.float32)
    t, ref = T(x), x.copy()
    v = rng.standard_normal((4, 6, 4)).astype(np.float32)
    t[[0, 3, 0, 4]] = T(v)                                    # duplicates: the last occurrence stays
    ref[[0, 3, 0, 4]] = v
    same_bits(host(t.data), ref)
    t[:, T(np.array([5, 0, 5], np.int32))] = T(v[:3, :1].reshape(3, 1, 4)[:, 0])      # [3, 4] broadcast over the leading axis
    ref[:, [5, 0, 5]] = v[:3, 0]
    same_bits(host(t.data), ref)
    t[[1, 2], [0, 5]] = -1.0
    ref[[1, 2], [0, 5]] = -1.0
    same_bits(host(t.data), ref)
    m1 = rng.random(5) < 0.5
    m1[0], m1[1] = True, False
    t[T(m1)] = 0.0                                            # mask rank 1, a scalar
    ref[m1] = 0.0
    same_bits(host(t.data), ref)
    assert last_tier()[0] == TIER["general"]
    m2 = rng.random((5, 6)) < 0.5
    row = rng.standard_normal(4).astype(np.float32)
    t[T(m2)] = T(row)                                         # mask rank 2, a value that broadcasts to the unmasked axis
    ref[m2] = row
    same_bits(host(t.data), ref)
    t[t > 1.0] = 1.0                                          # a full-rank mask built on the device
    ref[ref > 1.0] = 1.0
    same_bits(host(t.data), ref)
    t[m1] = 3.0                                               # a host mask
    ref[m1] = 3.0
    same_bits(host(t.data), ref)
    ti, refi = T(np.arange(12, dtype=np.int64).reshape(3, 4) * 2 ** 33), np.arange(12, dtype=np.int64).reshape(3, 4) * 2 ** 33
    ti[ti > 2 ** 35] = -(2 ** 40) - 1
    refi[refi > 2 ** 35] = -(2 ** 40) - 1
    same_bits(host(ti.data), refi)
    with pytest.raises(NotImplementedError, match="number of selected"):
        t[T(m1)] = T(np.ones((int(m1.sum()), 6, 4), np.float32))
    with pytest.raises(IndexError):
        t[T(np.ones(4, np.bool_))] = 0.0
    with pytest.raises(RuntimeError, match="requires_grad=True"):
        T(x, requires_grad=True)[0] = 1.0
    with pytest.raises(NotImplementedError):
        t[0] = T(np.ones((6, 4), np.int32))                   # a value of another dtype
    with pytest.raises(ValueError, match="broadcast"):
        t[0] = T(np.ones((5, 4), np.float32))
    with pytest.raises(IndexError, match="out of bounds"):
        t[[0, 5]] = 1.0
    same_bits(host(t.data), ref)                              # the refusals changed nothing


# ===================================================================================================== argmin
ARGMIN_CASES = [((9, 37), 1), ((9, 37), 0), ((3, 5000), 1), ((2, 70001), 1), ((5, 4097), -1), ((4, 6, 5), 1), ((4, 6, 5), None), ((70001,), None),
                ((2, 3, 4), 0), ((1, 1), None)]


@pytest.mark.parametrize("shape,axis", ARGMIN_CASES, ids=[f"{s}ax{a}" for s, a in ARGMIN_CASES])
def test_argmin_mirrors_argmax(hip, shape, axis):
    """np.argmin on every path of the argmax kernels (a wave per row, a block per row, chunked long rows, the strided kernel): ties take
    the first index, a NaN wins, axis None and keepdims; and argmax itself still agrees with NumPy."""
    rng = np.random.default_rng(int(np.prod(shape)))
    x = np.round(rng.standard_normal(shape) * 3).astype(np.float32)          # integers: plenty of ties
    for variant in ("ties", "nan"):
        if variant == "nan":
            flat = x.reshape(-1)
            flat[rng.integers(0, flat.size, max(1, flat.size // 50))] = np.nan
        for keep in (False, True):
            got = hip.argmin(T(x), axis=axis, keepdims=keep)
            assert got.dtype == np.int32 and got.requires_grad is False
            same_bits(host(got.data), np.argmin(x, axis=axis, keepdims=keep).astype(np.int32), f"argmin {variant}")
            same_bits(host(hip.argmax(T(x), axis=axis, keepdims=keep).data), np.argmax(x, axis=axis, keepdims=keep).astype(np.int32), f"argmax {variant}")
    same_bits(host(hip.argmin(T(np.array([[np.inf, -np.inf, -np.inf], [0.0, -0.0, 0.0]], np.float32)), axis=1).data), np.array([1, 0], np.int32))


# ===================================================================================================== fixtures of the reference
def test_every_fixture_case_on_the_device(hip, golden):
    """The single ops bit for bit, gradients included (comparisons: the reference leaves float32 0 / 1, here bool); the two gradients of
    a broadcast `where` operand and the six compositions at the bound the existing tape compositions are held to (tests/tape_ref.py: FIX)."""
    g = golden(IR.FIX)
    cases = IR.tape_index_cases()
    worst = {}
    SUMMED = {("where_row", 2), ("where_col_scalar", 0)}       # the two single-op gradients that are SUMS: a broadcast `where` operand
    for tag in sorted(cases):
        specs, fn = cases[tag]
        ins = [g[f"{tag}/in{i}"] for i in range(len(specs))]
        ts = [T(a.copy(), requires_grad=s[1] == "f") for a, s in zip(ins, specs)]
        y = fn(hip, "cuda", *ts)
        ref = g[f"{tag}/Y"]
        got = host(y.data)
        assert got.shape == ref.shape, tag
        exact = tag not in IR.COMPOSITIONS
        if got.dtype == np.bool_:
            same_bits(got, ref != 0, tag)
        elif exact:
            same_bits(got, ref, tag)
        else:
            np.testing.assert_allclose(got, ref, err_msg=tag, **R.FIX)
        if f"{tag}/dY" not in g:
            assert not y.requires_grad, tag
            continue
        y.backward(dev(g[f"{tag}/dY"]))
        for i, t in enumerate(ts):
            if f"{tag}/d{i}" not in g:
                continue
            gg, gr = host(t.grad).reshape(ins[i].shape), g[f"{tag}/d{i}"]
            if exact and (tag, i) not in SUMMED:
                same_bits(gg, gr, f"{tag} d{i}")
            else:
                np.testing.assert_allclose(gg, gr, err_msg=f"{tag} d{i}", **R.FIX)
                worst[tag] = max(worst.get(tag, 0.0), float(np.max(np.abs(gg - gr) / (1e-5 + 1e-5 * np.abs(gr)))))
    print("\n[fixtures] largest gradient error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ===================================================================================================== one captured step
def test_captured_step_replays_bit_for_bit(hip):
    """A compare, a where forward + backward (with a broadcast operand: the reduction tier), a slice forward + backward and a
    duplicate-index gather backward (the `last` table in the library workspace, reserved beforehand) in ONE hipGraph; three replays on
    fresh inputs equal the eager results bit for bit.  A host read inside any of the entries would fail the capture."""
    from neunet_hip._lib import call_hip_function
    rng = np.random.default_rng(12)
    N, F = 40, 24
    xs = [rng.standard_normal((N, F)).astype(np.float32) for _ in range(4)]
    bs = [rng.standard_normal((F,)).astype(np.float32) for _ in range(4)]
    ids = rng.integers(0, N, 64).astype(np.int32)
    ids[:8] = 3
    x, b = T(xs[0], requires_grad=True), T(bs[0], requires_grad=True)
    tid = T(ids)

    def step():
        x.grad, b.grad = None, None
        mask = x > 0.25
        y = x.where(mask, b)                    # b [F] is broadcast over the rows: its gradient is a column reduction
        z = y[1:-1, ::2]                        # slice forward / backward
        rows = x[tid]                           # duplicate-index gather: last-wins assign on the way back
        loss = (z * z).sum() + (rows * 0.5).sum()
        loss.backward()
        return mask, y, z, rows, loss

    def snapshot(out):
        return [host(o.data).copy() for o in out] + [host(x.grad).copy(), host(b.grad).copy()]

    eager = []
    for s in range(1, 4):
        x.data.copy_(dev(xs[s]))
        b.data.copy_(dev(bs[s]))
        eager.append(snapshot(step()))
    call_hip_function("nnhipWorkspaceReserve", 1 << 20)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    x.data.copy_(dev(xs[0]))
    b.data.copy_(dev(bs[0]))
    torch.cuda.synchronize()
    call_hip_function("nnhipWorkspaceLock", 1)
    try:
        with torch.cuda.graph(graph, stream=side):
            out = step()
            gx, gb = x.grad, b.grad
        for s in range(1, 4):
            x.data.copy_(dev(xs[s]))
            b.data.copy_(dev(bs[s]))
            graph.replay()
            torch.cuda.synchronize()
            got = [host(o.data) for o in out] + [host(gx), host(gb)]
            for a, e in zip(got, eager[s - 1]):
                same_bits(a, e, f"replay {s}")
    finally:
        call_hip_function("nnhipWorkspaceLock", 0)
    ref_rows = IR.getitem_backward((N, F), ids, np.full((64, F), 0.5, np.float32))
    assert (ref_rows[3] == 0.5).all()
