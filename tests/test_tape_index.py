"""CPU: the indexing half of the Tensor tape (ABI 224).  canonical_index / canonical_lattice / canonical_advanced of
neunet_hip/tensor_index.py against NumPy (a table of keys and a seeded fuzz); the restatements of tests/index_ref.py and the CPU-tensor
paths of every new method against the reference's fixtures (tests/golden/tape_index.npz) and against NumPy; the hash / NotImplemented
rules that keep Tensors usable in sets, lists and `is None` style host code; the constructors; the ABI's argument checks as status codes."""
import ctypes
import random

import numpy as np
import pytest

import index_ref as IR


@pytest.fixture(scope="module")
def lib():
    import neunet_hip
    from neunet_hip import _lib
    neunet_hip.load_library()
    return _lib


def cpu(a, **kw):
    from neunet_hip import Tensor
    a = np.asarray(a)
    kw.setdefault("requires_grad", False)
    return Tensor(a, dtype=a.dtype, device="cpu", **kw)


def test_version_is_224(lib):
    assert lib.load_hip_function("nnhipVersion")() >= 224


# ===================================================================================================== canonicalisation vs NumPy
def check_key(shape, key):
    """The descriptor applied to np.arange(n).reshape(shape) equals NumPy's x[key], and IndexError is raised exactly where NumPy raises."""
    from neunet_hip.tensor_index import canonical_index, canonical_lattice
    x = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    try:
        ref = x[key]
    except IndexError:
        with pytest.raises(IndexError):
            canonical_index(shape, key)
        return "error"
    offset, out_shape, strides = canonical_index(shape, key)
    assert out_shape == ref.shape, (shape, key, out_shape, ref.shape)
    assert all(s != 0 for s in strides), (shape, key, strides)
    np.testing.assert_array_equal(IR.apply_descriptor(shape, offset, out_shape, strides), ref, err_msg=f"{shape} {key}")
    # the lattice of the backward: scattering x[key] back lands every selected element where it came from
    start, step, count = canonical_lattice(shape, key)
    back = IR.lattice_scatter(shape, start, step, count, ref + 1)
    np.testing.assert_array_equal(back, IR.getitem_backward(shape, key, ref + 1), err_msg=f"lattice {shape} {key}")
    return "ok"


@pytest.mark.parametrize("shape", IR.BASIC_SHAPES, ids=str)
def test_canonical_index_table(shape):
    seen = {"ok": 0, "error": 0}
    for key in IR.BASIC_KEYS + [5, -7, (0, 0, 0, 0, 0), (Ellipsis, Ellipsis), (slice(None),) * 5, (None, None), ()]:
        seen[check_key(shape, key)] += 1
    assert seen["ok"] >= len(IR.BASIC_KEYS) - 4 and seen["error"] >= 2, seen


def test_canonical_index_fuzz():
    rng = random.Random(224)
    seen = {"ok": 0, "error": 0}
    for _ in range(1500):
        rank = rng.randint(1, 5)
        shape = tuple(rng.randint(1, 7) for _ in range(rank))
        seen[check_key(shape, IR.random_key(rng, rank))] += 1
    assert seen["ok"] >= 500 and seen["error"] >= 100, seen


ADVANCED_KEYS = [((7, 4), [1, 3, 1]), ((7, 4), np.array([[1, 3, 1], [0, 3, 6]])), ((3, 4, 5), (slice(None), [1, 3, 1])),
                 ((3, 4, 5), (Ellipsis, [0, 0, 3])), ((3, 4, 5), (np.arange(3), [3, 1, 3])), ((3, 4, 5), (slice(None), [[0], [3]], [[4, 1, 4]])),
                 ((3, 4, 5), (1, [0, 2])), ((3, 4, 5), (slice(None), 2, [0, 4, -1])), ((3, 4, 5), ([-1, 0],)), ((2, 3, 4, 5), ([0, 1], [2, 0], [3, 3])),
                 ((3, 4, 5), (slice(1, None), [0, 2])), ((3, 4, 5), ([], slice(None))), ((6,), ([5, 0, 5, 5],))]


@pytest.mark.parametrize("shape,key", ADVANCED_KEYS, ids=[f"{s}{IR.key_id(k)}" for s, k in ADVANCED_KEYS])
def test_canonical_advanced_matches_numpy(shape, key):
    """[outer, D1..Dk, inner] and the broadcast index arrays reproduce NumPy's x[key] (through NumPy's own take on the flat row index)."""
    from neunet_hip.tensor_index import canonical_advanced
    x = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    c = canonical_advanced(shape, key)
    src = x[c["slices"]] if not c["full"] else x
    if not c["full"]:
        c = canonical_advanced(src.shape, (slice(None),) * c["axis"] + tuple(c["arrays"]))
    arrays = [np.broadcast_to(a, c["bshape"]) for a in c["arrays"]]
    lin = np.zeros(c["bshape"], np.int64)
    for a, d in zip(arrays, c["dims"]):
        lin = lin * d + np.where(a < 0, a + d, a)
    got = src.reshape(c["outer"], int(np.prod(c["dims"])), c["inner"])[:, lin.reshape(-1), :].reshape(c["out_shape"])
    np.testing.assert_array_equal(got, x[key])


def test_advanced_key_refusals():
    from neunet_hip.tensor_index import canonical_advanced, classify_key
    with pytest.raises(NotImplementedError, match="separated"):
        canonical_advanced((3, 4, 5), ([0, 1], slice(None), [1, 2]))
    with pytest.raises(NotImplementedError, match="separated"):
        canonical_advanced((3, 4, 5), (0, slice(None), [1, 2]))
    with pytest.raises(NotImplementedError):
        canonical_advanced((3, 4, 5), ([0, 1], None))
    with pytest.raises(IndexError, match="out of bounds"):
        canonical_advanced((3, 4), ([0, 3],))
    with pytest.raises(IndexError, match="out of bounds"):
        canonical_advanced((3, 4), (slice(None), [-5]))
    with pytest.raises(IndexError, match="integer"):
        canonical_advanced((3, 4), ([0.5, 1.0],))
    with pytest.raises(IndexError, match="broadcast"):
        canonical_advanced((3, 4), ([0, 1], [0, 1, 2]))
    with pytest.raises(IndexError, match="too many"):
        canonical_advanced((3, 4), ([0], [0], [0]))
    assert classify_key(([True, False, True],)) == "mask" and classify_key((1, slice(None))) == "basic" and classify_key([1, 2]) == "advanced"
    with pytest.raises(NotImplementedError):
        classify_key((np.array([True, False]), 0))


# ===================================================================================================== fixtures: restatements and CPU tensors
def run_case_cpu(tag, g):
    import neunet_hip
    specs, fn = IR.tape_index_cases()[tag]
    ins = [g[f"{tag}/in{i}"] for i in range(len(specs))]
    ts = [cpu(a.copy(), requires_grad=s[1] == "f") for a, s in zip(ins, specs)]
    return ins, ts, fn(neunet_hip, "cpu", *ts)


def test_fixture_covers_the_cases(golden):
    g = golden(IR.FIX)
    tags = {k.split("/")[0] for k in g}
    assert tags == set(IR.tape_index_cases()), tags ^ set(IR.tape_index_cases())
    assert set(IR.COMPOSITIONS) <= tags
    m = g["masked_scores/in1"]
    assert (m.sum(axis=-1) == 0).any(), "the composition's mask has one fully masked row"
    dW = g["embedding/d0"]
    assert np.array_equal(dW, IR.getitem_backward(dW.shape, IR.IDS, g["embedding/dY"])) and (dW[[2, 4, 5]] == 0).all()
    assert np.array_equal(dW[1], g["embedding/dY"][0, 2]), "id 1 occurs twice: the last occurrence stays"


def test_cpu_tensors_reproduce_reference_fixtures(golden):
    """Every case of the fixture on CPU tensors (NumPy paths, gradients included).  Copies, selects and comparisons bit for bit; the
    compositions run the existing device-only arithmetic and are left to the GPU test."""
    g = golden(IR.FIX)
    ran = 0
    for tag in sorted(IR.tape_index_cases()):
        if tag in ("masked_scores", "positional", "last_step", "nll", "flip_squares", "where_function") or tag.startswith("where_"):
            continue        # arithmetic on a CPU tensor raises NotImplementedError (no CPU fallback): test_tape_ops.py
        ins, ts, y = run_case_cpu(tag, g)
        ref = g[f"{tag}/Y"]
        got = np.asarray(y.data)
        assert got.shape == ref.shape, tag
        if got.dtype == np.bool_:
            assert y.requires_grad is False and y.args is None, tag
            np.testing.assert_array_equal(got, ref != 0, err_msg=tag)
        else:
            np.testing.assert_array_equal(got, ref, err_msg=tag)
        if f"{tag}/dY" in g:
            y.backward(g[f"{tag}/dY"])
            for i, t in enumerate(ts):
                if f"{tag}/d{i}" in g:
                    np.testing.assert_array_equal(np.asarray(t.grad).reshape(ins[i].shape), g[f"{tag}/d{i}"], err_msg=f"{tag} d{i}")
        ran += 1
    assert ran >= 35, ran


def test_where_on_cpu_tensors_matches_fixtures(golden):
    g = golden(IR.FIX)
    for tag in ("where_row", "where_col_scalar", "where_function"):
        ins, ts, y = run_case_cpu(tag, g)
        np.testing.assert_array_equal(y.data, g[f"{tag}/Y"], err_msg=tag)
        assert y.dtype == np.float32
        y.backward(g[f"{tag}/dY"])
        for i, t in enumerate(ts):
            if f"{tag}/d{i}" in g:
                np.testing.assert_allclose(np.asarray(t.grad).reshape(ins[i].shape), g[f"{tag}/d{i}"], rtol=1e-6, atol=1e-6, err_msg=f"{tag} d{i}")


def test_restatements_reproduce_reference_fixtures(golden):
    g = golden(IR.FIX)
    x, dY = g["getitem_3/in0"], g["getitem_3/dY"]
    key = (slice(None, None, -2), slice(1, None, 3))
    np.testing.assert_array_equal(IR.getitem_backward(x.shape, key, dY), g["getitem_3/d0"])
    from neunet_hip.tensor_index import canonical_lattice
    np.testing.assert_array_equal(IR.lattice_scatter(x.shape, *canonical_lattice(x.shape, key), dY), g["getitem_3/d0"])
    a, h, b, dY = g["where_row/in0"], g["where_row/in1"], g["where_row/in2"], g["where_row/dY"]
    dA, dB, _, _ = IR.where_backward(h > 0, dY, a.shape, b.shape)
    np.testing.assert_array_equal(np.where(h > 0, a, b), g["where_row/Y"])
    np.testing.assert_allclose(dA, g["where_row/d0"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(dB, g["where_row/d2"], rtol=1e-6, atol=1e-6)
    for op in IR.COMPARE:
        np.testing.assert_array_equal(IR.NP_COMPARE[op](g[f"{op}_row/in0"], g[f"{op}_row/in1"]), g[f"{op}_row/Y"] != 0, err_msg=op)


# ===================================================================================================== CPU tensors vs NumPy
def test_cpu_comparisons_and_logical_against_numpy():
    a = np.array([[np.nan, 0.0, -0.0, 1.5], [2.0, -np.inf, np.inf, 1e-45]], np.float32)
    b = np.array([0.0, 0.0, 0.0, 1.5], np.float32)
    ta, tb = cpu(a), cpu(b)
    for op in IR.COMPARE:
        for got, ref in ((getattr(ta, op)(tb), IR.NP_COMPARE[op](a, b)), (getattr(ta, op)(1.5), IR.NP_COMPARE[op](a, np.float32(1.5)))):
            assert got.dtype == np.bool_ and got.requires_grad is False and got.args is None and got.op == op
            np.testing.assert_array_equal(got.data, ref, err_msg=op)
    np.testing.assert_array_equal((ta == tb).data, a == b)
    np.testing.assert_array_equal((ta != tb).data, a != b)
    np.testing.assert_array_equal(((ta > 0) & (tb >= 1)).data, (a > 0) & (b >= 1))
    np.testing.assert_array_equal(((ta > 0) | (tb >= 1)).data, (a > 0) | (b >= 1))
    np.testing.assert_array_equal((~(ta > 0)).data, ~(a > 0))
    np.testing.assert_array_equal(ta.logical_and(tb).data, np.logical_and(a, b))       # a NaN is true
    i = np.array([1, 0, -3, 2 ** 31 - 1], np.int32)
    np.testing.assert_array_equal((cpu(i) == 0).data, i == 0)
    np.testing.assert_array_equal((cpu(i) < 0.5).data, i < 0.5)
    np.testing.assert_array_equal((cpu(i) == [1, 0, 3, 0]).data, i == np.array([1, 0, 3, 0]))


def test_cpu_indexing_flip_setitem_against_numpy():
    import neunet_hip
    rng = np.random.default_rng(0)
    for shape, key in IR.basic_cases():
        x = rng.standard_normal(shape).astype(np.float32)
        t = cpu(x, requires_grad=True)
        y = t[key]
        np.testing.assert_array_equal(y.data, x[key])
        assert y.data.flags["C_CONTIGUOUS"] and y.op == "getitem"
        if y.data.size:
            dY = rng.standard_normal(y.shape).astype(np.float32)
            y.backward(dY)
            np.testing.assert_array_equal(t.grad, IR.getitem_backward(shape, key, dY))
    x = rng.standard_normal((2, 3, 4)).astype(np.float32)
    for axis in IR.FLIP_AXES:
        t = cpu(x, requires_grad=True)
        y = t.flip(axis)
        np.testing.assert_array_equal(y.data, np.flip(x, axis))
        y.backward(x)
        np.testing.assert_array_equal(t.grad, np.flip(x, axis))
        np.testing.assert_array_equal(neunet_hip.flip(cpu(x), axis).data, np.flip(x, axis))
    with pytest.raises(ValueError):
        cpu(x).flip((0, 0))
    t, ref = cpu(x), x.copy()
    t[:, ::2] = 1.5
    ref[:, ::2] = 1.5
    t[[0, 1, 0], 1] = cpu(np.arange(12, dtype=np.float32).reshape(3, 4))
    ref[[0, 1, 0], 1] = np.arange(12, dtype=np.float32).reshape(3, 4)
    t[cpu(ref[..., 0] > 0)] = -2.0
    ref[ref[..., 0] > 0] = -2.0
    np.testing.assert_array_equal(t.data, ref)
    ids = cpu(np.array([2, 0, 2], np.int64))
    w = cpu(x[0], requires_grad=True)
    out = w[ids]
    np.testing.assert_array_equal(out.data, x[0][[2, 0, 2]])
    out.backward(np.ones((3, 4), np.float32) * np.arange(1, 4, dtype=np.float32)[:, None])
    np.testing.assert_array_equal(w.grad, np.array([[2] * 4, [0] * 4, [3] * 4], np.float32))
    c = cpu(x)
    assert c.contiguous() is c


def test_argmin_on_cpu_tensors():
    import neunet_hip
    x = np.array([[3.0, 1.0, 1.0, 2.0], [np.nan, 0.0, np.nan, -1.0]], np.float32)
    for axis, keep in ((None, False), (1, False), (0, True), (-1, True), (None, True)):
        got = neunet_hip.argmin(cpu(x), axis=axis, keepdims=keep)
        assert got.dtype == np.int32 and got.requires_grad is False
        np.testing.assert_array_equal(got.data, np.argmin(x, axis=axis, keepdims=keep))


# ===================================================================================================== hash / NotImplemented rules
def test_tensors_stay_hashable_and_comparable_with_anything():
    t, u = cpu(np.ones(3)), cpu(np.ones(3))
    assert hash(t) == object.__hash__(t) and len({t, u, t}) == 2 and {t: 1}[t] == 1
    assert (t == None) is False and (t != None) is True          # noqa: E711  (the point of the test)
    assert (t == "abc") is False and (t == object()) is False
    assert t.equal(None) is NotImplemented and t.__lt__("x") is NotImplemented
    with pytest.raises(TypeError):
        t < None                                                 # noqa: B015
    assert t in [None, t] and None in [t, None] and [None, t].index(t) == 1
    assert not hasattr(type(t), "__bool__")
    from neunet_hip.nn.parameter import Parameter
    p = Parameter(cpu(np.ones((2, 2), np.float32)))
    assert hash(p) == object.__hash__(p) and p in [p] and len({p, Parameter(cpu(np.ones((2, 2), np.float32)))}) == 2


def test_setitem_refuses_a_tensor_that_requires_grad():
    t = cpu(np.zeros((2, 3), np.float32), requires_grad=True)
    with pytest.raises(RuntimeError, match="requires_grad=True"):
        t[0] = 1.0
    with pytest.raises(RuntimeError, match="requires_grad=True"):
        t[[0, 1]] = 1.0


# ===================================================================================================== constructors
def test_constructors_defaults_shapes_and_dtypes():
    """The reference's wrapper contract (its tests/test_init_api_wrappers.py), restated: float32, requires_grad=False and "cpu" by
    default; shapes as separate ints, one tuple or one list; *_like follow their argument's dtype and device; arange's one-argument form."""
    import neunet_hip as nh
    for fn, value in ((nh.ones, 1.0), (nh.zeros, 0.0)):
        for args in ((2, 3), ((2, 3),), ([2, 3],)):
            t = fn(*args)
            assert t.shape == (2, 3) and t.dtype == np.float32 and t.requires_grad is False and t.device == "cpu"
            assert (t.data == value).all()
        t = fn(4, dtype=np.int32, requires_grad=True)
        assert t.shape == (4,) and t.dtype == np.int32 and t.requires_grad is True
        assert fn().shape == ()
    np.random.seed(7)
    r = nh.rand(3, 2)
    np.random.seed(7)
    np.testing.assert_array_equal(r.data, np.random.rand(3, 2).astype(np.float32))
    assert r.dtype == np.float32 and r.requires_grad is False and (r.data >= 0).all() and (r.data < 1).all()
    np.random.seed(8)
    n = nh.randn((2, 5))
    np.random.seed(8)
    np.testing.assert_array_equal(n.data, np.random.randn(2, 5).astype(np.float32))
    assert nh.randn(2, 2, dtype=np.float64).dtype == np.float64
    np.testing.assert_array_equal(nh.arange(5).data, np.arange(5, dtype=np.float32))
    np.testing.assert_array_equal(nh.arange(2, 9, 3).data, np.arange(2, 9, 3, dtype=np.float32))
    a = nh.arange(0, 6, 2, dtype=np.int64)
    assert a.dtype == np.int64 and a.requires_grad is False and a.data.tolist() == [0, 2, 4]
    src = cpu(np.arange(6, dtype=np.int32).reshape(2, 3))
    for fn, value in ((nh.ones_like, 1), (nh.zeros_like, 0)):
        t = fn(src)
        assert t.shape == (2, 3) and t.dtype == np.int32 and t.device == "cpu" and t.requires_grad is False and (t.data == value).all()
        assert fn(src, dtype=np.float32, requires_grad=True).dtype == np.float32 and fn(src, requires_grad=True).requires_grad is True
    for fn in (nh.copy, nh.clone):
        leaf = cpu(np.arange(4, dtype=np.float32), requires_grad=True)
        c = fn(leaf)
        assert c is not leaf and c.data is not leaf.data and c.requires_grad is True and c.dtype == np.float32 and c.args is None
        c.data[0] = 9
        assert leaf.data[0] == 0
    t = nh.tensor([1, 2, 3])
    assert t.requires_grad is True and t.dtype == np.float32 and t.device == "cpu"      # neunet_hip.tensor keeps its defaults
    for name in ("ones", "zeros", "rand", "randn", "arange", "ones_like", "zeros_like", "argmin", "flip", "where", "equal", "not_equal",
                 "greater", "greater_equal", "less", "less_equal", "logical_and", "logical_or", "logical_not", "copy", "clone"):
        assert callable(getattr(nh, name)), name
    for name in ("equal", "not_equal", "greater", "greater_equal", "less", "less_equal", "logical_and", "logical_or", "logical_not",
                 "__eq__", "__ne__", "__gt__", "__ge__", "__lt__", "__le__", "__and__", "__or__", "__invert__", "where", "flip",
                 "__getitem__", "__setitem__", "contiguous"):
        assert hasattr(nh.Tensor, name), name


def test_every_reference_name_is_provided():
    """No public function of the reference's package module and no method of its Tensor is missing here (names only, read from the
    fixture of names below: the reference itself is not importable from a test)."""
    import neunet_hip as nh
    functions = ("save load tensor ones zeros rand randn arange ones_like zeros_like argmax argmin add sub mul div matmul sum mean var power "
                 "sqrt log exp tanh sin cos maximum minimum max min concatenate reshape abs transpose swapaxes flip where equal not_equal greater "
                 "greater_equal less less_equal logical_and logical_or logical_not copy clone").split()
    methods = ("to add sub mul div matmul sum mean var power sqrt log exp tanh sin cos maximum minimum max min reshape abs transpose swapaxes "
               "T flip where equal not_equal greater greater_equal less less_equal logical_and logical_or logical_not backward").split()
    assert not [f for f in functions if not callable(getattr(nh, f, None))]
    assert not [m for m in methods if not hasattr(nh.Tensor, m)]


# ===================================================================================================== ABI argument checks
def test_abi_argument_errors_are_status_codes(lib):
    """Every check precedes the first device call: the pointers here are never dereferenced."""
    EINVAL, EALIGN = -1, -2
    D = 0x1000
    i64 = lambda *v: (ctypes.c_int64 * max(len(v), 1))(*v)  # noqa: E731
    f = lib.load_hip_function
    sh, st = i64(2, 3), i64(3, 1)
    cmp_, logical, wf, wb = f("nnhipCompare"), f("nnhipLogical"), f("nnhipWhereForward"), f("nnhipWhereBackward")
    sf, sb, sa = f("nnhipSliceForward"), f("nnhipSliceBackward"), f("nnhipStridedAssign")
    ig, ia, ma, amin = f("nnhipIndexGather"), f("nnhipIndexAssign"), f("nnhipMaskedAssign"), f("nnhipArgminF32")
    for kind in (-1, 6):
        assert cmp_(kind, D, D, D, 0.0, 0, 0, 0, 2, sh, st, st, None) == EINVAL and "unknown kind" in lib.last_error()
    assert logical(3, D, D, D, 0, 0, 2, sh, st, st, None) == EINVAL and "unknown kind" in lib.last_error()
    assert cmp_(0, D, D, D, 0.0, 0, 0, 4, 2, sh, st, st, None) == EINVAL and "dtype" in lib.last_error()
    assert cmp_(0, D, None, None, 0.0, 0, 0, 0, 2, sh, st, st, None) == EINVAL and "null" in lib.last_error()
    assert cmp_(0, None, D, D, 0.0, 0, 0, 0, 2, sh, st, st, None) == EINVAL and "null" in lib.last_error()
    assert cmp_(0, D, D + 2, D, 0.0, 0, 0, 0, 2, sh, st, st, None) == EALIGN
    assert cmp_(0, D, D + 4, D, 0.0, 0, 0, 2, 2, sh, st, st, None) == EALIGN            # int64 operands: 8-byte alignment
    nine = i64(*([2] * 9))
    assert cmp_(0, D, D, D, 0.0, 0, 0, 0, 9, nine, nine, nine, None) == EINVAL and "rank" in lib.last_error()
    assert wf(D, D, 2, D, D, 0.0, 0.0, 2, sh, st, st, st, None) == EINVAL and "condition" in lib.last_error()     # an int64 condition
    assert wb(D, D, D, D, 2, 2, sh, st, st, st, None) == EINVAL and "condition" in lib.last_error()
    assert wf(None, D, 3, D, D, 0.0, 0.0, 2, sh, st, st, st, None) == EINVAL and "null" in lib.last_error()
    assert wb(D, None, None, D, 3, 2, sh, st, st, None, None) == EINVAL and "null" in lib.last_error()
    assert wb(None, None, None, None, 3, 2, sh, st, None, None, None) == 0                                        # nothing asked for
    assert sf(D, D, 0, 7, 2, sh, st, None) == EINVAL and "dtype" in lib.last_error()
    assert sf(D, None, 0, 0, 2, sh, st, None) == EINVAL and "null" in lib.last_error()
    assert sf(D, D, 0, 0, 9, nine, nine, None) == EINVAL and "rank" in lib.last_error()
    e8, s8 = i64(*([2] * 8)), i64(*[3 ** (8 - i) for i in range(8)])
    assert sf(D, D, 0, 0, 8, e8, s8, None) == EINVAL and "axis groups" in lib.last_error()
    assert sb(D, D, 2, sh, i64(0, 0), i64(1, 0), i64(2, 3), None) == EINVAL and "zero step" in lib.last_error()
    assert sb(D, D, 2, sh, i64(0, 1), i64(1, 1), i64(2, 3), None) == EINVAL and "leaves the tensor" in lib.last_error()
    assert sb(D, D, 2, sh, i64(0, 0), i64(-1, 1), i64(2, 3), None) == EINVAL and "leaves the tensor" in lib.last_error()
    assert sb(None, D, 2, sh, i64(0, 0), i64(1, 1), i64(2, 3), None) == EINVAL and "null" in lib.last_error()
    assert sb(D, D, 8, e8, i64(*([0] * 8)), i64(*([2] * 8)), i64(*([1] * 8)), None) == EINVAL and "axis groups" in lib.last_error()
    assert sa(D, 0, i64(3, 0), None, None, 1.0, 0, 0, 0, 2, sh, None) == EINVAL and "destination stride" in lib.last_error()
    assert sa(None, 0, st, None, None, 1.0, 0, 0, 0, 2, sh, None) == EINVAL and "null" in lib.last_error()
    ptrs = (ctypes.c_void_p * 4)(D, D, D, D)
    dims = i64(3, 4, 5, 6)
    assert ig(D, D, 0, ptrs, 1, 0, dims, 1, 4, 1, None) == EINVAL and "index arrays" in lib.last_error()
    assert ig(D, D, 0, ptrs, 1, 5, dims, 1, 4, 1, None) == EINVAL and "index arrays" in lib.last_error()
    assert ig(D, D, 0, ptrs, 0, 1, dims, 1, 4, 1, None) == EINVAL and "int32 or int64" in lib.last_error()
    assert ig(D, D, 0, ptrs, 1, 1, dims, 1, 1 << 31, 1, None) == EINVAL and "int32" in lib.last_error()
    assert ig(D, D, 0, (ctypes.c_void_p * 4)(D + 4, D, D, D), 2, 1, dims, 1, 4, 1, None) == EALIGN
    assert ia(D, D, 0.0, 0, 0, 9, 1, ptrs, 1, 1, dims, 1, 4, 1, None) == EINVAL and "dtype" in lib.last_error()
    assert ia(D, D, 0.0, 0, 0, 0, 1, ptrs, 1, 1, dims, -1, 4, 1, None) == EINVAL and "negative" in lib.last_error()
    assert ma(D, None, None, 0.0, 0, 0, 0, 4, 4, None) == EINVAL and "null" in lib.last_error()
    assert ma(D, D, None, 0.0, 0, 0, 0, -4, 4, None) == EINVAL
    assert amin(D, D, 2, 0, 3, None) == EINVAL and "argmin of an empty sequence" in lib.last_error()
    assert amin(None, D, 2, 5, 3, None) == EINVAL and "nnhipArgminF32" in lib.last_error()
    # zero size: 0 without a launch, whatever the pointers are
    z = i64(2, 0)
    assert cmp_(0, None, None, D, 0.0, 0, 0, 0, 2, z, st, st, None) == 0
    assert logical(0, None, None, None, 0, 0, 2, z, st, st, None) == 0
    assert wf(None, None, 3, None, None, 0.0, 0.0, 2, z, st, st, st, None) == 0
    assert wb(D, D, None, None, 3, 2, z, st, st, st, None) == 0
    assert sf(None, None, 0, 0, 2, z, st, None) == 0
    assert sb(None, None, 2, z, i64(0, 0), i64(1, 1), i64(2, 0), None) == 0
    assert sa(None, 0, st, None, None, 1.0, 0, 0, 0, 2, z, None) == 0
    assert ig(None, None, 0, ptrs, 1, 1, dims, 1, 0, 4, None) == 0
    assert ia(None, None, 0.0, 0, 0, 0, 1, ptrs, 1, 1, dims, 0, 4, 4, None) == 0
    assert ma(None, None, None, 0.0, 0, 0, 0, 0, 4, None) == 0
    assert amin(None, None, 0, 5, 3, None) == 0
