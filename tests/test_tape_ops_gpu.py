"""GPU: the Tensor arithmetic of ABI 223 (csrc/tensor_ops.hip through neunet_hip/tensor_ops.py and the C ABI) against the float64
restatements of tests/tape_ref.py, at every tier route() names and at the extents where the code takes another path, and the
compositions against the reference's fixtures (tests/golden/tape_ops.npz).  The bounds are derived in tests/tape_ref.py.  Each test
prints its largest error / bound ratio before it asserts (run with -s)."""
import ctypes

import numpy as np
import pytest

import tape_ref as R
from test_rowops_ref import MAP_SIZES, SPECIALS, map_inputs
from test_rowops_tiers_gpu import Buf, call, close_bound, dev, hip, host, ratio  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
FIX = R.FIX
KIND = {k: i for i, k in enumerate(R.BINARY)}
RED = {k: i for i, k in enumerate(R.REDUCE)}
POSITIVE = ("div", "power")


def T(a, **kw):
    """A device Tensor of exactly a's shape (through a torch array: the constructor's NumPy path makes a 0-d array 1-d)."""
    from neunet_hip import Tensor
    a = np.asarray(a, np.float32)
    return Tensor(dev(a).reshape(a.shape), device="cuda", **kw)


def i64(v):
    return (ctypes.c_int64 * max(len(v), 1))(*[int(x) for x in v])


def i32(v):
    return (ctypes.c_int32 * max(len(v), 1))(*[int(x) for x in v])


def operands(op, sa, sb, seed=0):
    rng = np.random.default_rng(seed + 31 * len(sa) + len(sb) + int(np.prod(sa + sb + (1,))) % 1000)
    draw = (lambda s: rng.uniform(0.5, 2.5, s)) if op in POSITIVE else (lambda s: rng.standard_normal(s) * 2)
    a, b = draw(sa).astype(np.float32), draw(sb).astype(np.float32)
    if op in ("maximum", "minimum"):        # rounded to halves: plenty of ties, where both operands receive the gradient
        a, b = np.round(a * 2) / 2, np.round(b * 2) / 2
    return a, b


def within(got, ref, bound, what=""):
    """Largest |got - ref| / bound over the entries where `ref` is a number, ASSERTED here to be <= 1: a NaN in `got` where `ref` is
    finite (an element the kernel never wrote: the output buffers are pre-filled with NaN) fails the placement check, and a NaN
    ratio fails `<= 1`.  Returned for the summary line; the figure is in the assertion message when it fails."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN placement differs ({int(np.isnan(got).sum())} NaN against {int(np.isnan(ref).sum())})"
    ok = ~np.isnan(ref)
    r = ratio(got[ok], ref[ok], np.broadcast_to(np.asarray(bound, np.float64), ref.shape)[ok])
    assert r <= 1.0, f"{what}: error / bound {r}"
    return r


TIER = {"same": 1, "scalar": 2, "inner": 3, "outer": 3, "vec2d": 3, "general": 4, "tile": 5}
RED_TIER = {"row-wave": 10, "row-block": 11, "col": 12, "general": 13}


def last_tier():
    """(tier code, segments) of the library's most recent tensor-op launch (nnhipTensorOpsLastTier)."""
    from neunet_hip import _lib
    seg = ctypes.c_int64(0)
    return _lib.load_hip_function("nnhipTensorOpsLastTier")(ctypes.byref(seg)), seg.value


def forward_bound(op, ref):
    return (R.U * np.abs(ref) + 1e-45) if op in R.EXACT_BINARY else close_bound(ref, 1e-5, 1e-5)


def count_calls(monkeypatch):
    from neunet_hip import _lib
    counts, real = {}, _lib.call_hip_function

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(_lib, "call_hip_function", counting)
    return counts


def abi_binary_forward(op, a, b, off=0):
    """Through the C ABI with operands placed `off` floats past a 16-byte boundary."""
    from neunet_hip.tensor_ops import broadcast_strides
    out_shape = np.broadcast_shapes(a.shape, b.shape)
    A, B, O = Buf(a, off), Buf(b, off), Buf(tuple(out_shape) or (1,), off)
    call("nnhipBroadcastBinaryForward", KIND[op], O.t, A.t, B.t, 0.0, len(out_shape), i64(out_shape), i64(broadcast_strides(a.shape, out_shape)),
         i64(broadcast_strides(b.shape, out_shape)))
    assert O.intact()
    want = R.route("binary", sa=a.shape, sb=b.shape, aligned=off == 0)
    assert last_tier()[0] == TIER[want], (a.shape, b.shape, off, want, last_tier())        # the C code took the tier route() names
    return O.host().reshape(out_shape)


# ===================================================================================================== binary forward
@pytest.mark.parametrize("n", MAP_SIZES)
def test_binary_same_shape_sizes(hip, n, monkeypatch):
    x, _, z = map_inputs(n)
    worst = {}
    for op in R.BINARY:
        a, b = (np.abs(x) + 0.5, np.abs(z) + 0.5) if op in POSITIVE else (x, z)
        for off in (0, 1):
            got, ref = abi_binary_forward(op, a, b, off), R.binary_forward(op, a, b)
            worst[op] = max(worst.get(op, 0), within(got, ref, forward_bound(op, ref)))
    print(f"\n[same n = {n}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0
    # add on this tier is nnhipAdd's kernel: same bits, one launch
    A, B = dev(x), dev(z)
    want = torch.empty_like(A)
    call("nnhipAdd", want, A, B, n)
    tx, tz = T(x), T(z)
    counts = count_calls(monkeypatch)
    got = tx.add(tz)
    monkeypatch.undo()
    assert counts == {"nnhipAdd": 1}, counts                       # one launch, and not through the broadcasting entry
    assert torch.equal(got.data, want)
    from neunet_hip.tensor_ops import binary_forward
    assert torch.equal(binary_forward(KIND["add"], A, B), want)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("f", R.INNER_EXTENTS)
def test_binary_inner_outer_extents(hip, f, off):
    """[N, F] o [F] and [N, F] o [N, 1], the small operand on either side, N = 7 (odd, more than one float4 row apart)."""
    worst = {}
    for op in R.BINARY:
        for sa, sb in (((7, f), (f,)), ((7, f), (7, 1)), ((f,), (7, f)), ((7, 1), (7, f))):
            a, b = operands(op, sa, sb)
            got, ref = abi_binary_forward(op, a, b, off), R.binary_forward(op, a, b)
            worst[op] = max(worst.get(op, 0), within(got, ref, forward_bound(op, ref)))
    print(f"\n[inner/outer F = {f} off = {off}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("case", range(len(R.BINARY_CASES)), ids=[f"{a}o{b}".replace(" ", "") for a, b in R.BINARY_CASES])
def test_binary_case_table_forward_backward(hip, case):
    """Every tier of the table through the Tensor methods: forward, and both gradients against float64 (the gradient of a broadcast
    operand under the reduction bound)."""
    sa, sb = R.BINARY_CASES[case]
    worst = {}
    for op in R.BINARY:
        a, b = operands(op, sa, sb, seed=case)
        ta, tb = T(a), T(b)
        y = getattr(ta, op)(tb)
        if not (op == "add" and sa == sb):          # (same-shape add is Tensor.add's nnhipAdd fast path, not this entry)
            assert last_tier()[0] == TIER[R.BINARY_TIERS[case]], (sa, sb, last_tier())
        assert y.op == op and y.shape == np.broadcast_shapes(sa, sb)
        ref = R.binary_forward(op, a, b)
        g = np.random.default_rng(case).standard_normal(ref.shape).astype(np.float32)
        y.backward(dev(g))
        la, lb = R.binary_local_grads(op, a, b, g)
        r = [within(host(y.data), ref, forward_bound(op, ref))]
        for t, local, shape in ((ta, la, sa), (tb, lb, sb)):
            want = R.unbroadcast(local, shape)
            red_axes = tuple(range(local.ndim - len(shape))) + tuple(i + local.ndim - len(shape) for i, e in enumerate(shape) if e == 1 and local.shape[i + local.ndim - len(shape)] != 1)
            bound = R.sum_bound(local, red_axes, extra_rtol=1e-5).reshape(shape) if red_axes else close_bound(want, 1e-5, 1e-5)
            assert tuple(t.grad.shape) == tuple(shape)
            r.append(within(host(t.grad), want, bound))
        worst[op] = max(r)
    print(f"\n[{sa} o {sb}: {R.BINARY_TIERS[case]}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def test_binary_scalars_and_reflected_operators(hip):
    x = np.random.default_rng(5).uniform(0.5, 2.5, (5, 7)).astype(np.float32)
    x64 = x.astype(np.float64)
    one = T([1.5], requires_grad=False)
    zero_d = T(np.float32(1.5), requires_grad=False)
    cases = {"x+s": (lambda t: t + 1.5, x64 + 1.5), "s+x": (lambda t: 1.5 + t, 1.5 + x64), "x-s": (lambda t: t - 1.5, x64 - 1.5),
             "s-x": (lambda t: 1.5 - t, 1.5 - x64), "x*s": (lambda t: t * 1.5, x64 * 1.5), "s*x": (lambda t: 1.5 * t, 1.5 * x64),
             "x/s": (lambda t: t / 1.5, x64 / 1.5), "s/x": (lambda t: 1.5 / t, 1.5 / x64), "x**s": (lambda t: t ** 1.5, x64 ** 1.5),
             "s**x": (lambda t: 1.5 ** t, 1.5 ** x64), "np.float32*x": (lambda t: np.float32(1.5) * t, 1.5 * x64),
             "x-[1]": (lambda t: t - one, x64 - 1.5), "[1]-x": (lambda t: one - t, 1.5 - x64), "x/0d": (lambda t: t / zero_d, x64 / 1.5),
             "0d/x": (lambda t: zero_d / t, 1.5 / x64), "-x": (lambda t: -t, -x64), "+x": (lambda t: +t, x64)}
    grads = {"x+s": 1, "s+x": 1, "x-s": 1, "s-x": -1, "x*s": 1.5, "s*x": 1.5, "x/s": 1 / 1.5, "s/x": -1.5 / x64 ** 2, "x**s": 1.5 * x64 ** 0.5,
             "s**x": 1.5 ** x64 * np.log(1.5), "np.float32*x": 1.5, "x-[1]": 1, "[1]-x": -1, "x/0d": 1 / 1.5, "0d/x": -1.5 / x64 ** 2, "-x": -1, "+x": 1}
    worst = 0.0
    for tag, (f, ref) in cases.items():
        t = T(x)
        y = f(t)
        y.backward()
        worst = max(worst, within(host(y.data), ref, close_bound(ref, 1e-5, 1e-5)),
                    within(host(t.grad), np.broadcast_to(grads[tag], x.shape), close_bound(np.broadcast_to(grads[tag], x.shape), 1e-5, 1e-5)))
        np.testing.assert_allclose(host(y.data), ref, err_msg=tag, **FIX)
        np.testing.assert_allclose(host(t.grad), np.broadcast_to(grads[tag], x.shape), err_msg=tag, **FIX)
    print(f"\n[scalars] worst error / bound {worst:.3f}")
    # a scalar gets no gradient and does not make the result require one
    c = T(x, requires_grad=False)
    assert (c * 2.0).args is None and not (c * 2.0).requires_grad


@pytest.mark.parametrize("layout", ["same", "row", "col", "scalar", "general"])
def test_binary_specials_match_numpy_float32(hip, layout):
    """NaN / inf placement as NumPy's float32 arithmetic gives it, every pair of SPECIALS."""
    s = SPECIALS
    a = np.repeat(s, len(s)).reshape(len(s), len(s)).copy()
    shapes = {"same": a.T.copy(), "row": s.copy(), "col": s.reshape(-1, 1).copy(), "scalar": None, "general": None}
    with np.errstate(all="ignore"):
        for op in R.BINARY:
            npf = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "power": np.power, "maximum": np.maximum,
                   "minimum": np.minimum}[op]
            if layout == "scalar":
                pairs = [(a, np.float32(v)) for v in s]
            elif layout == "general":
                pairs = [(a[:, :5].copy(), s[:5].copy()), (a[:, None, :6].copy(), s[:7].reshape(7, 1).copy())]
            else:
                pairs = [(a, shapes[layout])]
            for x, y in pairs:
                got = host(getattr(T(x), op)(float(y) if np.ndim(y) == 0 else T(y)).data)
                want = npf(x, y).astype(np.float32)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (op, layout)
                assert np.array_equal(np.isinf(got), np.isinf(want)), (op, layout)
                fin = np.isfinite(want) & np.isfinite(got)
                np.testing.assert_allclose(got[fin], want[fin], rtol=1e-5, atol=1e-37, err_msg=f"{op} {layout}")
                if op in ("maximum", "minimum"):
                    np.testing.assert_array_equal(got, want)


def test_maximum_minimum_ties_give_both_gradients(hip):
    a = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], np.float32)
    b = np.array([1.0, 7.0, 3.0], np.float32)
    g = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]], np.float32)
    for op in ("maximum", "minimum"):
        ta, tb = T(a), T(b)
        getattr(ta, op)(tb).backward(dev(g))
        da, db = R.binary_backward(op, a, b, g)
        np.testing.assert_array_equal(host(ta.grad), da)
        np.testing.assert_array_equal(host(tb.grad), db)


def test_broadcast_backward_is_one_entry_without_a_full_temporary(hip, monkeypatch):
    """dB of [N, F] * [F] and of [N, F] * [N, 1]: one nnhipBroadcastBinaryBackward call, and the peak device memory over the backward
    stays below the inputs plus ONE full-shape buffer (dA, which is legitimate) -- the full-shape dB never exists."""
    N, F = 1024, 1024
    full = N * F * 4
    for sb in ((F,), (N, 1)):
        a, b = operands("mul", (N, F), sb)
        g = np.random.default_rng(1).standard_normal((N, F)).astype(np.float32)
        ta, tb, gd = T(a), T(b), dev(g)
        y = ta * tb
        counts = count_calls(monkeypatch)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y.grad_fn(*y.args, grad=gd)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        monkeypatch.undo()
        assert counts == {"nnhipBroadcastBinaryBackward": 1}, counts
        assert last_tier() == tuple([RED_TIER[R.route("reduce", shape=(N, F), axis=0 if sb == (F,) else 1)[0]], R.route("reduce", shape=(N, F), axis=0 if sb == (F,) else 1)[1]])
        print(f"\n[{(N, F)} * {sb}] backward peak {peak / full:.3f} full-shape buffers")
        assert peak < 1.5 * full
        la, lb = R.binary_local_grads("mul", a, b, g)
        np.testing.assert_allclose(host(ta.grad), la, **FIX)
        want = R.unbroadcast(lb, sb)
        bound = R.sum_bound(lb, 0 if sb == (F,) else 1, extra_rtol=1e-5).reshape(sb)
        print(f"    dB error / bound {within(host(tb.grad), want, bound):.3f}")
        assert within(host(tb.grad), want, bound) <= 1.0
        # only dB: no full-shape allocation at all
        ta2, tb2 = T(a, requires_grad=False), T(b)
        y2 = ta2 * tb2
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y2.grad_fn(*y2.args, grad=gd)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base < 0.1 * full and ta2.grad is None
        assert torch.equal(tb2.grad, tb.grad)


# ===================================================================================================== unary
@pytest.mark.parametrize("n", (5, 4097))
def test_unary_maps(hip, n):
    x, g, _ = map_inputs(n)
    worst = {}
    for op in R.UNARY:
        xx = (np.abs(x) + np.float32(0.05)) if op == "sqrt" else x
        t = T(xx)
        y = getattr(t, op)()
        assert y.op == op
        y.backward(dev(g))
        Yr, dXr = R.unary_forward(op, xx), R.unary_backward(op, xx, g)
        worst[op] = max(within(host(y.data), Yr, close_bound(Yr, 1e-5, 1e-5)), within(host(t.grad), dXr, close_bound(dXr, 1e-5, 1e-5)))
        np.testing.assert_allclose(host(y.data), Yr, err_msg=op, **FIX)
        np.testing.assert_allclose(host(t.grad), dXr, err_msg=op, **FIX)
    print(f"\n[unary n = {n}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    import neunet_hip
    assert torch.equal(neunet_hip.tanh(T(x)).data, T(x).tanh().data)


# ===================================================================================================== reductions
def reduce_input(shape, seed, big_mean=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    return (x + 1e4 if big_mean else x * 3).astype(np.float32)


@pytest.mark.parametrize("case", range(len(R.REDUCE_CASES)), ids=[f"{s}ax{a}".replace(" ", "") for s, a in R.REDUCE_CASES])
def test_reduce_case_table(hip, case):
    shape, axis = R.REDUCE_CASES[case]
    x = reduce_input(shape, case)
    worst = {}
    for keep in (False, True):
        for op in R.REDUCE:
            t = T(x)
            y = getattr(t, op)(axis=axis, keepdims=keep)
            tier, S = R.REDUCE_TIERS[case]
            assert last_tier() == (RED_TIER[tier], S), (shape, axis, last_tier())
            ref = R.reduce_forward(op, x, axis, keep)
            assert y.op == op and y.shape == ref.shape
            again = getattr(T(x), op)(axis=axis, keepdims=keep)
            assert torch.equal(y.data, again.data), f"{op}: reruns differ"
            bound = {"sum": R.sum_bound, "mean": R.mean_bound, "var": R.var_bound}.get(op, lambda *a: 0.0)(x, axis, keep)
            if op in ("max", "min"):
                np.testing.assert_array_equal(host(y.data), ref, err_msg=op)
                r = 0.0
            else:
                r = within(host(y.data), ref, bound)
            g = np.random.default_rng(case + 1).standard_normal(ref.shape).astype(np.float32)
            y.backward(dev(g))
            dref = R.reduce_backward(op, x, axis, g)
            if op in ("sum", "max", "min"):
                np.testing.assert_array_equal(host(t.grad), dref.astype(np.float32), err_msg=f"{op} backward")
            else:
                rb = within(host(t.grad), dref, close_bound(dref, 1e-5, 1e-5))
                r = max(r, rb)
            worst[op] = max(worst.get(op, 0.0), r)
    print(f"\n[{shape} axis {axis}: {R.REDUCE_TIERS[case]}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("shape,axis", [((3, 1000), 1), ((3, 4000), 1), ((2, 9000), 1), ((1000, 5), 0), ((2, 7, 3, 50), (0, 2, 3))],
                         ids=["row-wave", "row-block", "row-split", "col-split", "general"])
def test_var_with_mean_far_above_std(hip, shape, axis):
    """mean 1e4, std 1: the float64 value is well conditioned, a single-pass E[x^2] - E[x]^2 in float32 is off by O(1)."""
    x = reduce_input(shape, 7, big_mean=True)
    t = T(x)
    y = t.var(axis=axis, keepdims=True)
    ref, bound = R.reduce_forward("var", x, axis, True), R.var_bound(x, axis, True)
    print(f"\n[var {shape} axis {axis}: {R.route('reduce', shape=shape, axis=axis)}] error / bound {within(host(y.data), ref, bound):.3f}, "
          f"largest relative error {np.max(np.abs(host(y.data) - ref) / ref):.2e}")
    assert within(host(y.data), ref, bound) <= 1.0
    g = np.ones(ref.shape, np.float32)
    y.backward(dev(g))
    dref = R.reduce_backward("var", x, axis, g)
    n = x.size // ref.size
    # the backward reuses the forward's float32 mean: |d| error <= 2 / n * (|mean error| + rounding of x - mean)
    e = 2.0 / n * ((R.sum_depth(shape, axis) + 2) * R.U * np.abs(x).max() + 4 * R.U * np.abs(x.astype(np.float64) - x.mean()).max())
    assert within(host(t.grad), dref, e + 1e-5 * np.abs(dref)) <= 1.0


@pytest.mark.parametrize("shape,axis", [((4, 9), 1), ((9, 70), 0), ((3, 2000), 1), ((2, 3, 5, 7), (0, 2, 3))], ids=["row", "col", "block", "general"])
def test_max_min_nan_and_ties(hip, shape, axis):
    x = np.clip(np.round(reduce_input(shape, 3)), -2, 2).astype(np.float32)       # clipped: ties at both extremes
    if axis == 1:
        x[0, 1] = np.nan
    else:
        x.flat[5] = np.nan
    for op in ("max", "min"):
        t = T(x)
        y = getattr(t, op)(axis=axis, keepdims=True)
        with np.errstate(invalid="ignore"):
            ref = R.reduce_forward(op, x, axis, True)
        np.testing.assert_array_equal(host(y.data), ref)                     # NaN where NumPy has NaN
        assert np.isnan(ref).any()
        g = np.random.default_rng(0).standard_normal(ref.shape).astype(np.float32)
        y.backward(dev(g))
        want = (g.astype(np.float64) * (x == ref)).astype(np.float32)       # NaN == NaN is false: a zero gradient where the result is NaN
        np.testing.assert_array_equal(host(t.grad), want)
        ties = ((x == ref).sum(axis=axis) > 1).any()
        assert ties, "the case should contain ties"


def test_reduce_abi_strided_input_and_mean_output(hip):
    """The entry takes arbitrary input strides (here a transposed view), and var hands back its means."""
    x = reduce_input((6, 10), 2)
    X, out, mean = dev(x), torch.empty(10, device="cuda"), torch.empty(10, device="cuda")
    call("nnhipReduceAxesForward", RED["var"], out, mean, X, 2, i64((10, 6)), i64((1, 10)), i32((0, 1)))
    assert within(host(out), x.astype(np.float64).var(0), R.var_bound(x.T.copy(), 1)) <= 1.0
    np.testing.assert_allclose(host(mean), x.astype(np.float64).mean(0), rtol=1e-6, atol=1e-6)


# ===================================================================================================== copy / transpose
@pytest.mark.parametrize("r", R.TRANSPOSE_2D)
def test_transpose_2d(hip, r):
    for c in R.TRANSPOSE_2D:
        x = np.random.default_rng(r * 100 + c).standard_normal((r, c)).astype(np.float32)
        t = T(x)
        y = t.T
        assert last_tier()[0] == TIER[R.route("copy", shape=(c, r), strides=(1, c))], (r, c, last_tier())
        assert y.data.is_contiguous()
        np.testing.assert_array_equal(host(y.data), x.T)
        g = np.random.default_rng(1).standard_normal((c, r)).astype(np.float32)
        y.backward(dev(g))
        np.testing.assert_array_equal(host(t.grad), g.T)


def test_transpose_rank4_and_swapaxes(hip):
    for shape, perm in R.TRANSPOSE_4D + (((2, 3, 4), (1, 2, 0)),):
        x = np.random.default_rng(4).standard_normal(shape).astype(np.float32)
        t = T(x)
        y = t.transpose(*perm)
        np.testing.assert_array_equal(host(y.data), x.transpose(perm))
        g = np.random.default_rng(5).standard_normal(y.shape).astype(np.float32)
        y.backward(dev(g))
        np.testing.assert_array_equal(host(t.grad), g.transpose(np.argsort(perm)))       # the inverse permutation
    x = np.random.default_rng(6).standard_normal((3, 33, 5)).astype(np.float32)
    t = T(x)
    y = t.swapaxes(-1, 1)
    assert y.op == "swapaxes"
    np.testing.assert_array_equal(host(y.data), x.swapaxes(-1, 1))
    y.backward(dev(np.ones(y.shape, np.float32) * 2))
    np.testing.assert_array_equal(host(t.grad), np.full(x.shape, 2, np.float32))
    # the ABI's scale and a stride-0 source
    src, out = dev(np.arange(5, dtype=np.float32)), torch.empty((3, 5), device="cuda")
    call("nnhipStridedCopy", out, src, 0.5, 2, i64((3, 5)), i64((0, 1)))
    np.testing.assert_array_equal(host(out), np.broadcast_to(np.arange(5) * 0.5, (3, 5)))


# ===================================================================================================== matmul
MATMUL_CASES = [((5, 7), (7, 4)), ((2, 3, 5, 7), (2, 3, 7, 4)), ((2, 3, 5, 7), (7, 4)), ((7,), (7,)), ((7,), (7, 4)), ((5, 7), (7,)),
                ((33, 129), (129, 65)), ((3, 17, 31), (31, 9))]


@pytest.mark.parametrize("sa,sb", MATMUL_CASES, ids=[f"{a}@{b}".replace(" ", "") for a, b in MATMUL_CASES])
def test_matmul(hip, sa, sb):
    rng = np.random.default_rng(len(sa) * 10 + len(sb))
    a, b = rng.standard_normal(sa).astype(np.float32), rng.standard_normal(sb).astype(np.float32)
    ta, tb = T(a), T(b)
    y = ta @ tb
    ref = a.astype(np.float64) @ b.astype(np.float64)
    assert y.op == "matmul" and y.shape == ref.shape
    K = sa[-1]

    def bound(x, w, k):     # the GEMM tier tests' dot bound (tests/test_gemm_tiers_gpu.py): 32 u sum |x_i w_i| + 4 u |ref|
        return 32 * R.U * (np.abs(R.f64(x)) @ np.abs(R.f64(w))) + 4 * R.U * np.abs(R.f64(x) @ R.f64(w)) + 1e-30

    r = [within(host(y.data), ref, bound(a, b, K))]
    g = rng.standard_normal(ref.shape).astype(np.float32)
    y.backward(dev(g))
    da, db = R.matmul_backward(a, b, g)
    a2, b2, g2 = np.atleast_2d(a), (b.reshape(-1, 1) if b.ndim == 1 else b), np.reshape(g, np.atleast_2d(a).shape[:-1] + ((b.reshape(-1, 1) if b.ndim == 1 else b).shape[-1],))
    ba = bound(g2, np.swapaxes(b2, -1, -2), b2.shape[-1]).reshape(a.shape)
    if b2.ndim == 2 and a2.ndim > 2:      # the shared right operand: one GEMM over batch * M
        bb = bound(np.swapaxes(a2.reshape(-1, K), 0, 1), g2.reshape(-1, g2.shape[-1]), a2.size // K).reshape(b.shape)
    else:
        bb = bound(np.swapaxes(a2, -1, -2), g2, a2.shape[-2]).reshape(b.shape)
    r += [within(host(ta.grad), da, ba), within(host(tb.grad), db, bb)]
    print(f"\n[{sa} @ {sb}] error / bound: Y {r[0]:.3f}, dA {r[1]:.3f}, dB {r[2]:.3f}")
    assert tuple(ta.grad.shape) == sa and tuple(tb.grad.shape) == sb
    assert max(r) <= 1.0


def test_matmul_unsupported_broadcast(hip):
    with pytest.raises(NotImplementedError):
        T(np.ones((2, 3, 4))) @ T(np.ones((5, 4, 6)))
    with pytest.raises(NotImplementedError):
        T(np.ones((3, 4))) @ T(np.ones((2, 4, 6)))
    with pytest.raises(ValueError):
        T(np.ones((3, 4))) @ T(np.ones((5, 6)))
    with pytest.raises(ValueError, match="over the limit"):
        T(np.ones((1,) * 9)) + T(np.ones((2,)))


# ===================================================================================================== fixtures of the reference
def fixture_fn(tag):
    import neunet_hip  # noqa: F401
    head = tag.split("_")[0]
    if head in R.BINARY and tag.split("_")[-1] in ("row", "col", "rcol"):
        return lambda a, b: getattr(a, head)(b)
    if tag in R.UNARY:
        return lambda a: getattr(a, tag)()
    if head in R.REDUCE:
        axis, keep = {"all": (None, False), "ax1": (1, False), "ax02k": ((0, 2), True), "last": (-1, True)}[tag.split("_")[1]]
        return lambda x: getattr(x, head)(axis=axis, keepdims=keep)
    return {"scalars": lambda a: (2.0 - a) * 0.5 + 1.5 / (a + 3.0) - a ** 2 + 2.0 ** a + (-a),
            "transpose": lambda x: x.transpose(0, 2, 1), "swapaxes": lambda x: x.swapaxes(0, 2), "T": lambda a: a.T,
            "matmul": lambda a, b: a @ b,
            "layernorm": lambda x, w, b: (x - x.mean(-1, keepdims=True)) / (x.var(-1, keepdims=True) + 1e-5).sqrt() * w + b,
            "softmax": lambda x: (x - x.max(axis=1, keepdims=True)).exp() / (x - x.max(axis=1, keepdims=True)).exp().sum(axis=1, keepdims=True),
            "mse": lambda a, b: ((a - b) ** 2).mean(),
            "linear_tanh_sum": lambda x, w, b: (x @ w + b).tanh().sum(axis=0),
            "twice": lambda a, b: a * b + a / (b * b + 1.0) + a}[tag if head != "matmul" else "matmul"]


def test_every_fixture_case_forward_and_gradients(hip, golden):
    """Single ops and the compositions (hand-written layer norm, softmax with the maximum subtracted, MSE, Linear -> tanh -> sum, a
    tensor consumed three times) against what the reference's tape computed: forward and every gradient at FIX."""
    g = golden("tape_ops")
    worst, tags = {}, sorted({k.split("/")[0] for k in g})
    assert {"layernorm", "softmax", "mse", "linear_tanh_sum", "twice"} <= set(tags)
    for tag in tags:
        ins = [T(g[f"{tag}/in{i}"]) for i in range(4) if f"{tag}/in{i}" in g]
        y = fixture_fn(tag)(*ins)
        assert y.shape == g[f"{tag}/Y"].shape, tag
        y.backward(dev(g[f"{tag}/dY"]))
        r = [within(host(y.data), g[f"{tag}/Y"], close_bound(g[f"{tag}/Y"], 1e-5, 1e-5))]
        r += [within(host(t.grad), g[f"{tag}/d{i}"], close_bound(g[f"{tag}/d{i}"], 1e-5, 1e-5)) for i, t in enumerate(ins)]
        worst[tag] = max(r)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
    print("\n[fixtures] largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in top))
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, bad


# ===================================================================================================== one captured step
def test_captured_step_with_composed_loss(hip):
    """A small model whose loss is composed from the new ops (matmul, broadcast bias, tanh, a column reduction whose reduced extent
    is split over blocks -- partials in the library workspace, reserved by the warm-up step --, (pred - y) ** 2, mean) under
    GraphedTrainStep: replays equal eager steps bit for bit.  A host synchronisation inside the captured region would fail the capture."""
    import neunet_hip.nn as nn
    from neunet_hip import optim
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    rng = np.random.default_rng(3)
    Xs = rng.uniform(-1, 1, (4, 300, 16)).astype(np.float32)
    Ys = rng.uniform(-1, 1, (4, 300, 8)).astype(np.float32)
    assert R.route("reduce", shape=(300, 8), axis=0) == ("col", 5)

    def run(graphed):
        np.random.seed(5)
        lin = nn.Linear(16, 8)
        scale = T(np.ones(8, np.float32))
        ps = lin.parameters() + [scale]
        opt = optim.Adam(ps, lr=1e-3)
        x, y = T(Xs[0], requires_grad=False), T(Ys[0], requires_grad=False)

        def fb():
            pred = (lin(x) * scale).tanh()
            col = pred.sum(axis=0)
            loss = ((pred - y) ** 2).mean() + (col * col).mean() * 0.01
            loss.backward()
            return loss

        losses = []
        step = GraphedTrainStep(fb, opt, GradBucket(ps), warmup=1) if graphed else None
        for s in range(0 if not graphed else 1, 4):
            x.data.copy_(dev(Xs[s]))
            y.data.copy_(dev(Ys[s]))
            if graphed:
                losses.append(step().item())
            else:
                opt.zero_grad()
                loss = fb()
                opt.step()
                losses.append(loss.item())
        out = [host(p.data).copy() for p in ps]
        if graphed:
            step.release()
        return out, losses[-3:]

    pe, le = run(False)
    pg, lg = run(True)
    assert le == lg, (le, lg)
    for a, b in zip(pe, pg):
        np.testing.assert_array_equal(a, b)


# ===================================================================================================== examples/conway.py
def test_conway_example_composed_loss_matches_module(hip):
    """Three training steps of examples/conway.py with --loss composed (((y_pred - y) ** 2).mean() on the new ops) and with nn.MSELoss
    from the same initial weights: the losses agree at the MSE fixture bound, and so do the parameters after the steps; one epoch of
    training lowers the mean loss."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import conway
    game = conway.GameOfLife()
    X, Y = conway.dataset(game)
    assert X.shape == (512, 3, 3) and Y.shape == (512, 3, 3)
    # the rule itself, against the definition written out
    for x, y in zip(X[::37], Y[::37]):
        n = np.array([[sum(x[(i + di) % 3, (j + dj) % 3] for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)) for j in range(3)] for i in range(3)])
        np.testing.assert_array_equal(y, ((n == 3) | ((x == 1) & (n == 2))).astype(int))
    runs = {}
    for kind in ("module", "composed"):
        np.random.seed(11)
        model = conway.Net()
        losses = conway.train(model, X, Y, 1, kind, "adam", seed=0, max_steps=3)
        runs[kind] = (losses, [host(p.data).copy() for p in model.parameters()])
    print(f"\n[conway] losses module {runs['module'][0]}, composed {runs['composed'][0]}")
    np.testing.assert_allclose(runs["composed"][0], runs["module"][0], **FIX)
    for a, b in zip(runs["composed"][1], runs["module"][1]):
        np.testing.assert_allclose(a, b, **FIX)


def test_conway_example_short_run_learns_the_rule(hip, golden):
    """The short run the fixture's generator searched and recorded (tools/gen_golden.py: CONWAY_RUN -- the first seed and epoch count
    after which the REFERENCE's net gets none of the 512 cases wrong with every prediction at least 0.15 from the 0.5 threshold), run
    by examples/conway.py from the reference's initial parameters with the same permutations: zero disagreeing cases here too."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import conway
    g = golden("conway_steps")
    assert int(g["run_wrong"][-1]) == 0 and len(g["run_wrong"]) == int(g["run_epochs"])
    X, Y = conway.dataset(conway.GameOfLife())
    model = conway.Net()
    for n, p in zip(("W1", "b1", "W2", "b2"), (model.conv1.weight, model.conv1.bias, model.conv2.weight, model.conv2.bias)):
        p.data.copy_(dev(g[f"{n}_init"]).reshape(p.data.shape))
    losses = conway.train(model, X, Y, int(g["run_epochs"]), "module", "adam", seed=int(g["run_seed"]), log=lambda *_: None)
    wrong = conway.disagreements(model, X, Y)
    margin = min(float(np.abs(model.predict(x) - 0.5).min()) for x in X)
    print(f"\n[conway short run] seed {int(g['run_seed'])}, {int(g['run_epochs'])} epochs: {wrong} of 512 wrong (the reference: {int(g['run_wrong'][-1])}), "
          f"margin {margin:.3f} (the reference: {float(g['run_margin'][-1]):.3f}), last mean loss {np.mean(losses[-512:]):.5f}")
    assert wrong == 0


def test_conway_example_vs_reference_steps(hip, golden):
    """The dataset of examples/conway.py equals the notebook's 512 cases, and three training steps (each started from the reference's
    own parameters before that step, so a step is compared, not a trajectory) reproduce its prediction, loss, gradients and the
    parameters after Adam, with nn.MSELoss and with the composed loss -- at the bounds test_conv_classifier_golden holds its fixture
    to: |loss - ref| < 1e-6, prediction at rtol 1e-4 / atol 1e-5, gradients at 1e-4 of max(|ref|, the list's scale); a parameter whose
    gradient is below 1e-4 of that scale is rounding noise to Adam's sign-like first steps and may land up to 2 lr away (fewer than
    5 % of the elements may), every other one at rtol 1e-4 / atol 1e-5."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import conway
    from neunet_hip.optim import Adam
    from test_hip_parity import assert_close_scaled, grad_list_scale
    g = golden("conway_steps")
    X, Y = conway.dataset(conway.GameOfLife())
    np.testing.assert_array_equal(X, g["X"])
    np.testing.assert_array_equal(Y, g["Y"])
    names, lr = ("W1", "b1", "W2", "b2"), 0.01
    for kind in ("module", "composed"):
        model = conway.Net()
        ps = [model.conv1.weight, model.conv1.bias, model.conv2.weight, model.conv2.bias]
        opt = Adam(ps, lr=lr)
        criterion = conway.make_loss(kind)
        loose = total = 0
        for s, i in enumerate(g["cases"]):
            for n, p in zip(names, ps):          # Adam's moments carry over (they are the reference's to rounding); the parameters are reset
                p.data.copy_(dev(g[f"{n}_init"] if s == 0 else g[f"p{s - 1}_{n}"]).reshape(p.data.shape))
            opt.zero_grad()
            pred = model(T(conway.wrap4(X[i]), requires_grad=False))
            loss = criterion(pred, T(np.asarray(Y[i], np.float32)[None, None], requires_grad=False))
            loss.backward()
            assert abs(loss.item() - float(g[f"loss{s}"])) < 1e-6, (kind, s, loss.item(), float(g[f"loss{s}"]))
            np.testing.assert_allclose(host(pred.data), g[f"pred{s}"], rtol=1e-4, atol=1e-5)
            gscale = grad_list_scale([g[f"g{s}_{n}"] for n in names])
            for n, p in zip(names, ps):
                assert_close_scaled(host(p.grad).reshape(g[f"g{s}_{n}"].shape), g[f"g{s}_{n}"], err_msg=f"{kind} step {s} grad {n}", scale=gscale)
            opt.step()
            for n, p in zip(names, ps):
                got, ref, gr = host(p.data), g[f"p{s}_{n}"], np.abs(g[f"g{s}_{n}"])
                noise = gr < 1e-4 * gscale
                np.testing.assert_allclose(got[~noise], ref[~noise], rtol=1e-4, atol=1e-5, err_msg=f"{kind} step {s} {n}")
                assert np.all(np.abs(got[noise] - ref[noise]) <= 2 * lr + 1e-5)
                loose, total = loose + int(noise.sum() - (np.abs(got[noise] - ref[noise]) <= 1e-5).sum()), total + got.size
        print(f"\n[conway {kind}] {loose} of {total} parameter values on the 2 lr allowance")
        assert loose < 0.05 * total
