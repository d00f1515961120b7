"""CPU: nn.AvgPool2d, nn.ZeroPad2d, nn.Flatten (ABI 225).  The float64 restatement of tests/avgpool_ref.py reproduces what the
reference recorded (tests/golden/shape_layers.npz) inside the bounds the GPU tests hold the kernels to; route() reaches every tier over
the case table and agrees with the library's own rule (nnhipAvgPool2dTier, host only); the constructors' normalisation and refusals;
Flatten on CPU tensors against the fixtures bit for bit, gradients included; every layer name the reference exports is a name of
neunet_hip.nn; the two new entries resolve and refuse bad arguments with status codes before anything touches a device."""
import ctypes
import os

import numpy as np
import pytest

import avgpool_ref as AR
from conftest import GOLDEN

FLAT = [("default", ()), ("d0_1", (0, 1)), ("dm2", (-2,)), ("d0_m1", (0, -1))]


@pytest.fixture(scope="module")
def lib():
    import neunet_hip
    from neunet_hip import _lib
    neunet_hip.load_library()
    return _lib


@pytest.fixture(scope="module")
def fx(golden):
    return golden("shape_layers")


def make_desc(g, dh=1, dw=1):
    from neunet_hip._lib import Pool2dDesc
    return Pool2dDesc(*[g[k] for k in "B C H W kh kw sh sw pu pd pl pr".split()], dh, dw)


# ---- the restatement against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in AR.CASES if AR.equal_padding(c)], ids=AR.case_id)
def test_restatement_reproduces_the_reference(fx, case):
    """The reference's float32 forward and input gradient sit inside the bounds around the float64 restatement (the issue measured
    0.29 / 0.31 of them at worst over the table)."""
    g = AR.geometry(*case[:4])
    tag = "avg/" + AR.case_id(case)
    assert fx[f"{tag}/Y"].shape == (g["B"], g["C"], g["Ho"], g["Wo"])
    rf = AR.check_forward(fx[f"{tag}/Y"], fx[f"{tag}/X"], g, tag)
    rb = AR.check_backward(fx[f"{tag}/dX"], fx[f"{tag}/dY"], g, tag)
    print(f"{tag}: reference forward {rf:.2f}, backward {rb:.2f} of the bound")


def test_every_row_the_reference_cannot_run_is_left_to_the_restatement(fx):
    recorded = {k.split("/")[1] for k in fx if k.startswith("avg/")}
    assert recorded == {AR.case_id(c) for c in AR.CASES if AR.equal_padding(c)}
    assert len(recorded) == len(AR.CASES) - 2                       # the unequal and the 4-tuple padding rows


def test_restated_backward_is_the_adjoint_of_the_forward():
    """<forward(X), dY> == <X, backward(dY)> in float64 on every row: the 4-tuple crop included, which no fixture covers."""
    rng = np.random.default_rng(7)
    for case in AR.CASES:
        g = AR.geometry(*case[:4])
        X = rng.standard_normal(case[0])
        dY = rng.standard_normal((g["B"], g["C"], g["Ho"], g["Wo"]))
        y, _ = AR.forward64(X, g)
        dx, _, m = AR.backward64(dY, g)
        assert dx.shape == X.shape
        np.testing.assert_allclose((y * dY).sum(), (X * dx).sum(), rtol=1e-12, atol=1e-12, err_msg=AR.case_id(case))
        assert m.max() <= g["kh"] * g["kw"]


# ---- the tier rule ---------------------------------------------------------------------------------------------------------------
def test_route_reaches_every_tier_and_keeps_padding_and_overlap_off_tiles(lib):
    seen = {}
    tier = lib.load_hip_function("nnhipAvgPool2dTier")
    for case in AR.CASES:
        g = AR.geometry(*case[:4])
        r = AR.route(g)
        seen.setdefault(r, []).append(case)
        if r == "tiles":
            assert g["pu"] + g["pd"] + g["pl"] + g["pr"] == 0 and (g["kh"], g["kw"]) == (g["sh"], g["sw"]), case
            assert g["H"] == g["Ho"] * g["kh"] and g["W"] == g["Wo"] * g["kw"], case
        if r.startswith("global"):
            assert (g["Ho"], g["Wo"]) == (1, 1)
        assert r.split("_")[0] in case[4] or r == "general", case           # the table's own label
        assert tier(ctypes.byref(make_desc(g))) == AR.TIER_IDS[r], case      # the library's rule is the restated one
    assert set(seen) == {"general", "tiles", "global_wave", "global_block"}
    planes = sorted(c[0][2] * c[0][3] for c in seen["global_wave"]), sorted(c[0][2] * c[0][3] for c in seen["global_block"])
    assert planes[0][-1] == AR.GLOBAL_WAVE_MAX and planes[1][0] == AR.GLOBAL_WAVE_MAX + 1   # one case on each side of the threshold
    for case in AR.CASES:                                                    # rows with leftovers, overlap, gaps or padding
        if any(w in case[4] for w in ("leftover", "overlap", "gaps", "padding")):
            assert AR.route(AR.geometry(*case[:4])) == "general", case
    modes = {AR.tiles_mode(AR.geometry(*c[:4]), 0, 0) for c in seen["tiles"]}
    assert modes == {0, 1, 2}                                                # scalar, pairs of 2-wide windows, 4-wide windows
    for c in seen["tiles"]:
        assert AR.tiles_mode(AR.geometry(*c[:4]), 4, 4) == 0                 # a base pointer one float in: the scalar kernel


def test_forced_general_route(lib):
    setr, tier = lib.load_hip_function("nnhipSetAvgPool2dRoute"), lib.load_hip_function("nnhipAvgPool2dTier")
    g = AR.geometry((2, 3, 6, 6), 2, None, 0)
    assert setr(1) == 0
    try:
        assert tier(ctypes.byref(make_desc(g))) == 0
        assert setr(7) == 1                                                  # an unknown value changes nothing
        assert tier(ctypes.byref(make_desc(g))) == 0
    finally:
        assert setr(0) == 1
    assert tier(ctypes.byref(make_desc(g))) == 1


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_version_and_entries(lib):
    assert lib.load_hip_function("nnhipVersion")() >= 225
    for name in ("nnhipAvgPool2dForward", "nnhipAvgPool2dBackward"):
        lib.load_hip_function(name)


def test_refusals_are_status_codes_before_any_device_call(lib):
    """Every refusal the header lists, with pointers that are never dereferenced (no device on this machine)."""
    EINVAL, EALIGN = -1, -2
    P = 0x1000
    base = AR.geometry((2, 3, 7, 5), 3, 2, 1)
    bad = [dict(base, **{k: 0}) for k in "B C H W kh kw sh sw".split()] + [dict(base, **{k: -1}) for k in "pu pd pl pr".split()]
    bad += [dict(base, kh=10), dict(base, kw=8)]                                             # output extent < 1
    bad += [dict(base, B=1 << 16, C=1 << 15, H=1, W=1, kh=1, kw=1, sh=1, sw=1, pu=0, pd=0, pl=0, pr=0)]   # 2^31 elements in and out
    bad += [dict(base, B=1 << 15, C=1 << 15, H=2, W=1, kh=2, kw=1, sh=1, sw=1, pu=0, pd=0, pl=0, pr=0)]   # 2^31 elements in only
    bad += [dict(base, B=1 << 15, C=1 << 15, H=1, W=1, kh=1, kw=1, sh=1, sw=1, pu=1, pd=0, pl=0, pr=0)]   # 2^31 elements out only
    for name in ("nnhipAvgPool2dForward", "nnhipAvgPool2dBackward"):
        f = lib.load_hip_function(name)
        assert f(P, P, None, None) == EINVAL
        assert f(None, P, ctypes.byref(make_desc(base)), None) == EINVAL and f(P, None, ctypes.byref(make_desc(base)), None) == EINVAL
        for g in bad:
            assert f(P, P, ctypes.byref(make_desc(g)), None) == EINVAL, g
        for dh, dw in [(2, 1), (1, 2), (-1, 1)]:
            assert f(P, P, ctypes.byref(make_desc(base, dh, dw)), None) == EINVAL
        assert f(P + 2, P, ctypes.byref(make_desc(base)), None) == EALIGN and f(P, P + 1, ctypes.byref(make_desc(base)), None) == EALIGN
        assert isinstance(lib.last_error(), str) and name in lib.last_error()
    assert lib.load_hip_function("nnhipAvgPool2dTier")(ctypes.byref(make_desc(base, 0, 0))) == 0          # dilation 0 reads as 1


# ---- constructors ------------------------------------------------------------------------------------------------------------------
def test_avgpool_constructor():
    import neunet_hip.nn as nn
    m = nn.AvgPool2d(2)
    assert (m.kernel_size, m.stride, m.padding) == ((2, 2), (2, 2), (0, 0, 0, 0))
    m = nn.AvgPool2d((3, 2), (2, 1), (1, 2))
    assert (m.kernel_size, m.stride, m.padding) == ((3, 2), (2, 1), (1, 1, 2, 2))
    assert nn.AvgPool2d(3, 0, 1).stride == (3, 3) and nn.AvgPool2d(3, None, (1, 0, 2, 1)).padding == (1, 0, 2, 1)
    assert nn.AvgPool2d(3, 1).stride == (1, 1) and nn.AvgPool2d(2, padding=5).padding == (5, 5, 5, 5)       # padding >= kernel is accepted
    for bad in ("same", "valid", "real same"):
        with pytest.raises(ValueError):
            nn.AvgPool2d(2, padding=bad)
    for kw in (dict(kernel_size=0), dict(kernel_size=2, stride=(1, 0)), dict(kernel_size=2, padding=-1), dict(kernel_size=2, padding=(1, 2, 3)),
               dict(kernel_size=(1, 2, 3)), dict(kernel_size=2.5)):
        with pytest.raises(ValueError):
            nn.AvgPool2d(**kw)
    from neunet_hip import Tensor
    with pytest.raises(TypeError):
        m(np.zeros((1, 1, 4, 4), np.float32))
    with pytest.raises(NotImplementedError):                                  # no CPU fallback
        m(Tensor(np.zeros((1, 1, 4, 4), np.float32), device="cpu"))


def test_zeropad_constructor():
    import neunet_hip.nn as nn
    from neunet_hip import Tensor
    assert nn.ZeroPad2d(2).padding == (2, 2, 2, 2) and nn.ZeroPad2d((1, 2)).padding == (1, 1, 2, 2)
    assert nn.ZeroPad2d((1, 2, 3, 0)).padding == (1, 2, 3, 0)
    for bad in (-1, (1, -2), (1, 2, 3), "same", 1.5):
        with pytest.raises(ValueError):
            nn.ZeroPad2d(bad)
    for shape in ((4, 4), (1, 1, 1, 4, 4)):
        with pytest.raises(ValueError):
            nn.ZeroPad2d(1)(Tensor(np.zeros(shape, np.float32), device="cpu"))
    with pytest.raises(NotImplementedError):
        nn.ZeroPad2d(1)(Tensor(np.zeros((1, 4, 4), np.float32), device="cpu"))
    with pytest.raises(TypeError):
        nn.ZeroPad2d(1)(np.zeros((1, 4, 4), np.float32))


def test_zeropad_fixture_is_numpy_pad(fx):
    """What the reference recorded is np.pad with (up, down, left, right): the GPU test's reference."""
    for tag in ("int", "pair", "four", "three_d"):
        X, p = fx[f"pad/{tag}/X"], [int(v) for v in fx[f"pad/{tag}/padding"]]
        pu, pd, pl, pr = (p[0], p[0], p[1], p[1]) if len(p) == 2 else p
        np.testing.assert_array_equal(fx[f"pad/{tag}/Y"], np.pad(X, ((0, 0),) * (X.ndim - 2) + ((pu, pd), (pl, pr))))


# ---- Flatten on the CPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,dims", FLAT, ids=[t for t, _ in FLAT])
def test_flatten_cpu_is_bit_equal_to_the_reference(fx, tag, dims):
    import neunet_hip.nn as nn
    from neunet_hip import Tensor
    assert tuple(int(v) for v in fx[f"flat/{tag}/dims"]) == dims
    x = Tensor(fx[f"flat/{tag}/X"], device="cpu")
    y = nn.Flatten(*dims)(x)
    assert y.shape == fx[f"flat/{tag}/Y"].shape and y.op == "reshape"
    np.testing.assert_array_equal(y.data.view(np.uint32), fx[f"flat/{tag}/Y"].view(np.uint32))
    y.backward(fx[f"flat/{tag}/dY"])
    assert x.grad.shape == x.shape
    np.testing.assert_array_equal(np.asarray(x.grad, np.float32).view(np.uint32), fx[f"flat/{tag}/dX"].view(np.uint32))


def test_flatten_refusals():
    import neunet_hip.nn as nn
    from neunet_hip import Tensor
    x = Tensor(np.zeros((2, 3, 4), np.float32), device="cpu")
    assert (nn.Flatten().start_dim, nn.Flatten().end_dim) == (1, -1)
    assert nn.Flatten(1, 1)(x).shape == (2, 3, 4) and nn.Flatten(-3, -2)(x).shape == (6, 4)
    for dims in ((2, 1), (-1, 0), (3, 3), (0, 5), (-4, -1)):
        with pytest.raises(ValueError):
            nn.Flatten(*dims)(x)
    with pytest.raises(TypeError):
        nn.Flatten()(np.zeros((2, 3)))


# ---- name parity -----------------------------------------------------------------------------------------------------------------
def test_every_reference_layer_name_is_in_nn():
    import neunet_hip.nn as nn
    names = open(os.path.join(GOLDEN, "nn_layer_names.txt")).read().split()
    assert len(names) == 17 and {"AvgPool2d", "ZeroPad2d", "Flatten"} <= set(names)
    missing = [n for n in names if not hasattr(nn, n)]
    assert not missing, missing
    from neunet_hip.nn import experimental as E
    assert nn.AvgPool2d is E.HIPAvgPool2d and nn.ZeroPad2d is E.HIPZeroPad2d and nn.Flatten is E.HIPFlatten
