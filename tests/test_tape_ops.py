"""CPU: the Tensor arithmetic of ABI 223.  The float64 restatements of tests/tape_ref.py reproduce the reference's fixtures
(tests/golden/tape_ops.npz, written by tools/gen_golden.py: gen_tape_ops); the canonicalisation of neunet_hip/tensor_ops.py against
brute force over every shape of rank <= 4 with extents from {1, 2, 3} and a random sample of rank 5-8; the case tables reach every
tier route() names (here only as route() and the package's own restatement see it: that the C code takes that tier is asserted on the
GPU, tests/test_tape_ops_gpu.py reads nnhipTensorOpsLastTier after its calls); the documented errors; the ABI's argument checks as
status codes."""
import ctypes
import itertools

import numpy as np
import pytest

import tape_ref as R

FIX = R.FIX


@pytest.fixture(scope="module")
def lib():
    import neunet_hip
    from neunet_hip import _lib
    neunet_hip.load_library()
    return _lib


def fixture_cases(g):
    return sorted({k.split("/")[0] for k in g})


# ===================================================================================================== restatements vs fixtures
def restate(tag, ins):
    """(Y, grads) of fixture case `tag` from the float64 restatements, given its inputs and dY (a function of dY)."""
    head = tag.split("_")[0]
    if head in R.BINARY:
        return R.binary_forward(head, *ins), lambda dY: R.binary_backward(head, ins[0], ins[1], dY)
    if tag in R.UNARY:
        return R.unary_forward(tag, ins[0]), lambda dY: (R.unary_backward(tag, ins[0], dY),)
    if head in R.REDUCE:
        axis, keep = {"all": (None, False), "ax1": (1, False), "ax02k": ((0, 2), True), "last": (-1, True)}[tag.split("_")[1]]
        return R.reduce_forward(head, ins[0], axis, keep), lambda dY: (R.reduce_backward(head, ins[0], axis, dY),)
    if head == "matmul":
        return R.f64(ins[0]) @ R.f64(ins[1]), lambda dY: R.matmul_backward(ins[0], ins[1], dY)
    return None, None


def test_restatements_reproduce_reference_fixtures(golden):
    g = golden("tape_ops")
    seen = 0
    for tag in fixture_cases(g):
        ins = [g[f"{tag}/in{i}"] for i in range(4) if f"{tag}/in{i}" in g]
        Y, back = restate(tag, ins)
        if Y is None:
            continue
        seen += 1
        np.testing.assert_allclose(Y, g[f"{tag}/Y"], err_msg=tag, **FIX)
        for i, d in enumerate(back(g[f"{tag}/dY"])):
            np.testing.assert_allclose(np.reshape(d, ins[i].shape), g[f"{tag}/d{i}"], err_msg=f"{tag} d{i}", **FIX)
    assert seen >= 7 * 3 + 6 + 5 * 4 + 6


def test_transpose_fixtures_are_numpy_transposes(golden):
    g = golden("tape_ops")
    np.testing.assert_array_equal(g["transpose/Y"], g["transpose/in0"].transpose(0, 2, 1))
    np.testing.assert_array_equal(g["transpose/d0"], g["transpose/dY"].transpose(0, 2, 1))
    np.testing.assert_array_equal(g["swapaxes/Y"], g["swapaxes/in0"].swapaxes(0, 2))
    np.testing.assert_array_equal(g["T/d0"], g["T/dY"].T)


# ===================================================================================================== canonicalisation
def sample_shapes(seed=0, count=150):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        yield tuple(int(e) for e in rng.choice((1, 2, 3), size=int(rng.integers(5, 9)), p=(0.5, 0.3, 0.2)))


def offsets(ext, strides):
    """Offsets of every element, in C order over the collapsed groups."""
    off = np.zeros(ext, np.int64)
    for g, (e, s) in enumerate(zip(ext, strides)):
        shape = [1] * len(ext)
        shape[g] = e
        off = off + (np.arange(e, dtype=np.int64) * s).reshape(shape)
    return off.ravel()


def check_broadcast(sa, sb):
    from neunet_hip import tensor_ops as T
    try:
        want = np.broadcast_shapes(sa, sb)
    except ValueError:
        with pytest.raises(ValueError):
            T.canonical_broadcast(sa, sb)
        return
    try:
        out_shape, ext, ta, tb = T.canonical_broadcast(sa, sb)
    except ValueError as exc:                       # more groups than the kernels take: only with rank > 6 of alternating broadcasts
        assert "axis groups" in str(exc) and len(want) > T.MAX_GROUPS
        return
    assert out_shape == want and int(np.prod(ext)) == int(np.prod(want)) and len(ext) <= T.MAX_GROUPS and (all(e > 1 for e in ext) or ext == [1])
    for shape, st in ((sa, ta), (sb, tb)):
        flat = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
        np.testing.assert_array_equal(offsets(ext, st), np.broadcast_to(flat, want).ravel(), err_msg=f"{sa} o {sb}")


def test_canonical_broadcast_vs_brute_force():
    small = list(R.shapes_up_to_rank4())
    rng = np.random.default_rng(1)
    for sa in small:
        for sb in (small[i] for i in rng.choice(len(small), 12, replace=False)):
            check_broadcast(sa, sb)
        # a broadcastable partner of the same rank: each extent kept or set to 1
        for mask in itertools.product((0, 1), repeat=len(sa)):
            check_broadcast(sa, tuple(1 if m else e for e, m in zip(sa, mask)))
    for sa in sample_shapes(2):
        mask = np.random.default_rng(sum(sa)).integers(0, 2, len(sa))
        check_broadcast(sa, tuple(1 if m else e for e, m in zip(sa, mask))[int(mask[0]):])
    check_broadcast(*R.RANK6)


def check_reduce(shape, axis, keepdims):
    from neunet_hip import tensor_ops as T
    x = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    want = x.sum(axis=axis, keepdims=keepdims)
    try:
        c = T.canonical_reduce(shape, axis, keepdims)
    except ValueError as exc:
        assert "axis groups" in str(exc) and len(shape) > T.MAX_GROUPS
        return
    assert c["out_shape"] == want.shape and c["kept_shape"] == x.sum(axis=axis, keepdims=True).shape
    ext, st, red = c["extents"], c["strides"], c["red"]
    assert all(a != b for a, b in zip(red, red[1:])), "kept and reduced groups alternate"
    # gather: kept groups outermost in order, reduced groups behind them -> [n_out, n_red] index sets
    off = offsets(ext, st).reshape(ext)
    order = [i for i, r in enumerate(red) if not r] + [i for i, r in enumerate(red) if r]
    nout = int(np.prod([ext[i] for i, r in enumerate(red) if not r]))
    sets = off.transpose(order).reshape(nout, -1)
    assert sets.shape[1] == c["n"] or want.size == 0
    np.testing.assert_array_equal(sets.sum(1), want.ravel(), err_msg=f"{shape} axis {axis}")
    np.testing.assert_array_equal(np.sort(sets.ravel()), np.arange(x.size))


def test_canonical_reduce_vs_brute_force():
    for shape in R.shapes_up_to_rank4():
        axes_sets = [None] + [c for k in range(1, len(shape) + 1) for c in itertools.combinations(range(len(shape)), k)]
        for axis in axes_sets:
            for keep in (False, True):
                check_reduce(shape, axis, keep)
                if axis is not None and len(axis) == 1:
                    check_reduce(shape, axis[0] - len(shape), keep)             # a negative int
    for shape in sample_shapes(3):
        rng = np.random.default_rng(sum(shape) + len(shape))
        axis = tuple(int(a) - len(shape) * int(rng.integers(0, 2)) for a in np.flatnonzero(rng.integers(0, 2, len(shape))))
        check_reduce(shape, axis or None, bool(rng.integers(0, 2)))


def test_axis_errors():
    from neunet_hip import tensor_ops as T
    for bad in (3, -4, (0, 0), (1, -2)):
        with pytest.raises(ValueError):
            T.canonical_reduce((2, 3, 4), bad)
    with pytest.raises(ValueError, match="over the limit"):
        T.canonical_reduce((1,) * 9, None)
    with pytest.raises(ValueError, match="over the limit"):
        T.canonical_broadcast((1,) * 9, (2,))


# ===================================================================================================== route coverage
def test_case_tables_reach_every_tier():
    from neunet_hip import tensor_ops as T
    got = [R.route("binary", sa=a, sb=b) for a, b in R.BINARY_CASES]
    assert got == R.BINARY_TIERS
    assert set(got) == {"same", "scalar", "inner", "outer", "vec2d", "general"}
    assert got == [T.route_binary(a, b) for a, b in R.BINARY_CASES]                  # the package's own statement agrees
    for n in R.INNER_EXTENTS:                                                          # the 16-byte tiers take multiples of 4 only
        want = ("inner", "outer") if n % 4 == 0 else ("general", "general")
        if n == 1:
            want = ("scalar", "same")
        assert (R.route("binary", sa=(6, n), sb=(n,)), R.route("binary", sa=(6, n), sb=(6, 1))) == want, n
        assert R.route("binary", sa=(6, n), sb=(n,), aligned=False) in ("general", "scalar")
    got = [R.route("reduce", shape=s, axis=a) for s, a in R.REDUCE_CASES]
    assert got == R.REDUCE_TIERS
    assert {t for t, _ in got} == {"row-wave", "row-block", "col", "general"}
    assert {(t, S > 1) for t, S in got} >= {("row-block", True), ("row-block", False), ("col", True), ("col", False), ("general", True),
                                            ("general", False)}
    for (s, a), want in zip(R.REDUCE_CASES, got):
        c = T.canonical_reduce(s, a)
        assert T.route_reduce(c["extents"], c["red"]) == want
    # the boundaries themselves
    assert [R.route("reduce", shape=(3, r), axis=1)[0] for r in (R.WAVE_MAX_R, R.WAVE_MAX_R + 1)] == ["row-wave", "row-block"]
    assert [R.route("reduce", shape=(3, r), axis=1)[1] for r in (R.ROW_SPLIT_MIN_R - 1, R.ROW_SPLIT_MIN_R)] == [1, 2]
    assert [R.route("reduce", shape=(k, 8192), axis=1)[1] for k in (R.FILL_BLOCKS - 1, R.FILL_BLOCKS)] == [2, 1]
    assert [R.route("reduce", shape=(r, 65), axis=0)[1] for r in (R.COL_SPLIT_MIN_R - 1, R.COL_SPLIT_MIN_R)] == [1, 4]
    # copies
    for r, c in itertools.product(R.TRANSPOSE_2D, repeat=2):
        want = "tile" if r > 1 and c > 1 else ("vec2d" if (r * c) % 4 == 0 else "general")
        assert R.route("copy", shape=(c, r), strides=(1, c)) == want == T.route_copy((c, r), (1, c)), (r, c)
    (s, p), (_, q) = R.TRANSPOSE_4D
    st = T.contiguous_strides(s)
    assert T.route_copy([s[a] for a in p], [st[a] for a in p]) == "general"            # the innermost axis stays innermost
    assert T.route_copy([s[a] for a in q], [st[a] for a in q]) == "tile"


# ===================================================================================================== errors
def test_errors_on_cpu_tensors_and_shapes():
    import neunet_hip
    x, y = neunet_hip.tensor(np.ones((2, 3))), neunet_hip.tensor(np.ones((4,)))
    with pytest.raises(ValueError):
        x.add(y)                                                         # shapes that do not broadcast: ValueError on either device
    np.testing.assert_array_equal((x + x).data, 2 * np.ones((2, 3)))    # the same-shape CPU add stays
    for f in (lambda: x * 2.0, lambda: 2.0 - x, lambda: x / x, lambda: x ** 2, lambda: -x, lambda: x.sum(), lambda: x.mean(axis=0),
              lambda: x.var(axis=-1, keepdims=True), lambda: x.max(), lambda: x.T, lambda: x.swapaxes(0, 1), lambda: x @ x.T,
              lambda: neunet_hip.tanh(x), lambda: x.exp(), lambda: x.sqrt(), lambda: x.add(neunet_hip.tensor(np.ones(3))),
              lambda: neunet_hip.maximum(x, x), lambda: x.abs()):
        with pytest.raises(NotImplementedError):
            f()


def test_module_functions_exist():
    import neunet_hip
    for name in ("add", "sub", "mul", "div", "matmul", "sum", "mean", "var", "power", "sqrt", "log", "exp", "tanh", "sin", "cos", "maximum",
                 "minimum", "max", "min", "reshape", "abs", "transpose", "swapaxes"):
        assert callable(getattr(neunet_hip, name)), name
    for name in ("__sub__", "__rsub__", "__mul__", "__rmul__", "__truediv__", "__rtruediv__", "__pow__", "__rpow__", "__neg__", "__pos__",
                 "__matmul__", "__rmatmul__", "__radd__", "T"):
        assert hasattr(neunet_hip.Tensor, name), name


def test_version_is_223(lib):
    assert lib.load_hip_function("nnhipVersion")() >= 223


def test_abi_argument_errors_are_status_codes(lib):
    """Every check precedes the first device call: the pointers here are never dereferenced."""
    EINVAL, EALIGN = -1, -2
    D = 0x1000
    i64 = lambda *v: (ctypes.c_int64 * max(len(v), 1))(*v)  # noqa: E731
    i32 = lambda *v: (ctypes.c_int32 * max(len(v), 1))(*v)  # noqa: E731
    fwd, bwd = lib.load_hip_function("nnhipBroadcastBinaryForward"), lib.load_hip_function("nnhipBroadcastBinaryBackward")
    rf, rb, cp = lib.load_hip_function("nnhipReduceAxesForward"), lib.load_hip_function("nnhipReduceAxesBackward"), lib.load_hip_function("nnhipStridedCopy")
    sh, st = i64(2, 3), i64(3, 1)
    for kind in (-1, 7, 100):
        assert fwd(kind, D, D, D, 0.0, 2, sh, st, st, None) == EINVAL and "unknown kind" in lib.last_error()
        assert bwd(kind, D, D, D, D, D, 0.0, 2, sh, st, st, None) == EINVAL and "unknown kind" in lib.last_error()
    for kind in (-1, 5):
        assert rf(kind, D, None, D, 2, sh, st, i32(0, 1), None) == EINVAL and "unknown kind" in lib.last_error()
        assert rb(kind, D, D, D, D, 2, sh, i32(0, 1), None) == EINVAL and "unknown kind" in lib.last_error()
    nine = i64(*([2] * 9))
    assert fwd(0, D, D, D, 0.0, 9, nine, nine, nine, None) == EINVAL and "rank" in lib.last_error()
    assert rf(0, D, None, D, 9, nine, nine, i32(*([0] * 9)), None) == EINVAL and "rank" in lib.last_error()
    assert cp(D, D, 1.0, 9, nine, nine, None) == EINVAL and "rank" in lib.last_error()
    assert cp(D, D, 1.0, -1, nine, nine, None) == EINVAL
    assert fwd(0, D, D, D, 0.0, 2, i64(2, -3), st, st, None) == EINVAL and "negative extent" in lib.last_error()
    assert fwd(0, D, None, None, 0.0, 2, sh, st, st, None) == EINVAL and "null" in lib.last_error()
    assert fwd(0, None, D, D, 0.0, 2, sh, st, st, None) == EINVAL and "null" in lib.last_error()
    assert fwd(0, D + 2, D, D, 0.0, 2, sh, st, st, None) == EALIGN
    assert bwd(0, D, None, D, None, D, 0.0, 2, sh, st, st, None) == EINVAL and "no gradient" in lib.last_error()
    assert rf(0, D, None, None, 2, sh, st, i32(0, 1), None) == EINVAL and "null" in lib.last_error()
    assert rb(2, D, D, None, D, 2, sh, i32(0, 1), None) == EINVAL and "null" in lib.last_error()          # var needs x
    assert cp(None, D, 1.0, 2, sh, st, None) == EINVAL and "null" in lib.last_error()
    # eight alternating broadcast axes do not collapse below seven groups
    e8, sa8, sb8 = i64(*([2] * 8)), i64(*[s if i % 2 else 0 for i, s in enumerate((128, 64, 32, 16, 8, 4, 2, 1))]), i64(*[0 if i % 2 else 1 for i in range(8)])
    assert fwd(0, D, D, D, 0.0, 8, e8, sa8, sb8, None) == EINVAL and "axis groups" in lib.last_error()
    # zero size: a no-op whatever the pointers are
    z = i64(2, 0)
    assert fwd(0, None, D, D, 0.0, 2, z, st, st, None) == 0 and bwd(0, None, None, None, D, D, 0.0, 2, z, st, st, None) == 0
    assert rf(0, None, None, None, 2, i64(0, 3), st, i32(0, 1), None) == 0 and rb(0, None, None, None, None, 2, z, i32(0, 1), None) == 0
    assert cp(None, None, 1.0, 2, z, st, None) == 0
    for kind in (8, 9, 10, 11, 12):                                        # the new unary kinds are known; 7 stays unknown
        assert lib.load_hip_function("nnhipActivationForward")(kind, D, D, 0.0, 0, None) == 0
    assert lib.load_hip_function("nnhipActivationForward")(7, D, D, 0.0, 0, None) == EINVAL
