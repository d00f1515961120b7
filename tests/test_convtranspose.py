"""CPU-only tests of ConvTranspose2d: the float64 restatement (tests/convtranspose_ref.py) against the reference's recorded
outputs and against torch, the host-only plan and the C ABI's argument checks (no device call is made), the host module, and what
the tier table of convtranspose_ref.py reaches in csrc/conv_transpose.hip and csrc/conv_mfma.hip."""
import ctypes

import numpy as np
import pytest

import convtranspose_ref as R

torch = pytest.importorskip("torch")

BIG = (3, 70, 5, 7, 130, 4, 2, 1, 1, 0)
FIELDS = "B Cin H W Cout kh kw sh sw dh dw pu pd pl pr oph opw".split()
EINVAL = -1
ROUTE_PHASE, ROUTE_GATHER, ROUTE_CONV2D = 1, 2, 3


def _load():
    """The library, built first where a clean checkout has none (as tests/test_abi.py does)."""
    import os

    import neunet_hip
    from neunet_hip import _lib
    if not os.path.exists(_lib.lib_path()):
        import importlib.util
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("nnhip_build", os.path.join(root, "numpy-nn-model_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return neunet_hip.load_library()


def make_desc(g, **over):
    from neunet_hip._lib import ConvTranspose2dDesc
    v = dict(g)
    v.update(over)
    return ConvTranspose2dDesc(*[v[k] for k in FIELDS])


def plan(desc, capacity=None):
    from neunet_hip._lib import load_hip_function
    n = int(desc.sh * desc.sw) if capacity is None else capacity
    route = ctypes.c_int32(-7)
    taps, pixels = (ctypes.c_int32 * max(n, 1))(), (ctypes.c_int32 * max(n, 1))()
    rc = load_hip_function("nnhipConvTranspose2dPlan")(ctypes.byref(desc), ctypes.byref(route), taps, pixels, n)
    return rc, route.value, list(taps)[:n], list(pixels)[:n]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.GEOMETRIES))
def test_restatement_matches_reference_fixture(golden, name):
    """rtol = atol = 1e-5: the level the golden tests hold float32 reference output to."""
    f, g = golden(name), R.normalise(R.GEOMETRIES[name])
    assert tuple(f["padding4"]) == (g["pu"], g["pd"], g["pl"], g["pr"])
    assert tuple(f["kernel"]) == (g["kh"], g["kw"]) and tuple(f["stride"]) == (g["sh"], g["sw"])
    assert tuple(f["dilation"]) == (g["dh"], g["dw"]) and tuple(f["output_padding"]) == (g["oph"], g["opw"])
    assert f["O"].shape == (g["B"], g["Cout"], g["Ho"], g["Wo"])
    np.testing.assert_allclose(R.forward(f["X"], f["W"], f["b"], g), f["O"], rtol=1e-5, atol=1e-5)
    dX, dW, db = R.backward(f["X"], f["W"], f["dO"], g)
    np.testing.assert_allclose(dX, f["dX"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dW, f["dW"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(db, f["db"].reshape(-1), rtol=1e-5, atol=1e-5)


def geometry(name):
    return BIG if name == "big" else R.GEOMETRIES[name] if name in R.GEOMETRIES else R.TIER_CASES[name]


@pytest.mark.parametrize("name", sorted(R.GEOMETRIES) + ["big"] + sorted(R.TIER_CASES))
def test_restatement_matches_torch_float64(name):
    """= torch conv_transpose2d(X, W.flip(2, 3).transpose(0, 1), ...); a 4-tuple padding is the zero-padding result cropped."""
    import torch.nn.functional as F
    g, X, W, b, dO = R.make_case(geometry(name), 5)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)   # noqa: E731
    Xt, Wt, bt = t(X), t(W), t(b)
    # torch wants padding <= d (k-1) + ... and symmetric: run it unpadded, with the output padding the crop leaves room for
    full = F.conv_transpose2d(Xt, Wt.flip(2, 3).transpose(0, 1), bt, (g["sh"], g["sw"]), 0, 0, 1, (g["dh"], g["dw"]))
    extra_h = max(0, g["pu"] + g["Ho"] - full.shape[2])
    extra_w = max(0, g["pl"] + g["Wo"] - full.shape[3])
    full = F.pad(full - bt.reshape(1, -1, 1, 1), (0, extra_w, 0, extra_h)) + bt.reshape(1, -1, 1, 1)   # output padding: bias only
    Ot = full[:, :, g["pu"]:g["pu"] + g["Ho"], g["pl"]:g["pl"] + g["Wo"]]
    assert tuple(Ot.shape) == (g["B"], g["Cout"], g["Ho"], g["Wo"])
    Ot.backward(torch.tensor(dO, dtype=torch.float64))
    np.testing.assert_allclose(R.forward(X, W, b, g), Ot.detach().numpy(), rtol=1e-12, atol=1e-12)
    dX, dW, db = R.backward(X, W, dO, g)
    np.testing.assert_allclose(dX, Xt.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dW, Wt.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-12, atol=1e-12)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.GEOMETRIES) + ["big"])
def test_plan(name):
    _load()
    g = R.normalise(BIG if name == "big" else R.GEOMETRIES[name])
    rc, route, taps, pixels = plan(make_desc(g))
    assert rc == g["sh"] * g["sw"] == len(taps)
    # every (output pixel, tap) pair whose divisions are exact is in exactly one phase, and every output pixel too
    assert sum(t * p for t, p in zip(taps, pixels)) * g["B"] == R.tap_pixel_pairs(g) * g["B"]
    assert sum(pixels) == g["Ho"] * g["Wo"]
    # a phase (py, px) is empty iff no tap r has r dh = py (mod sh), or none has s dw = px (mod sw)
    reach_y = {(r * g["dh"]) % g["sh"] for r in range(g["kh"])}
    reach_x = {(s * g["dw"]) % g["sw"] for s in range(g["kw"])}
    empty = [py * g["sw"] + px for py in range(g["sh"]) for px in range(g["sw"]) if py not in reach_y or px not in reach_x]
    assert [i for i, t in enumerate(taps) if t == 0] == empty
    if name in R.EMPTY_PHASES:
        assert empty == R.EMPTY_PHASES[name]
    if g["sh"] == 1 and g["sw"] == 1:
        small = g["pu"] <= g["dh"] * (g["kh"] - 1) and g["pl"] <= g["dw"] * (g["kw"] - 1)
        assert route == (ROUTE_CONV2D if small else ROUTE_GATHER)
    else:
        assert route == (ROUTE_GATHER if empty else ROUTE_PHASE)


def test_plan_routes_of_the_fixture_table():
    _load()
    routes = {n: plan(make_desc(R.normalise(geom)))[1] for n, geom in R.GEOMETRIES.items()}
    assert routes["convt_unet_in"] == routes["convt_unet_out"] == ROUTE_CONV2D
    assert routes["convt_s1_bigpad"] == ROUTE_GATHER                      # padding beyond d (k-1) at stride 1
    assert routes["convt_k4s2p1"] == routes["convt_pad4"] == routes["convt_op_ge_s"] == ROUTE_PHASE
    assert routes["convt_dil_gcd"] == routes["convt_s3k2"] == routes["convt_mixed"] == routes["convt_uneven"] == ROUTE_GATHER


# ---- the tier table (convtranspose_ref.TIER_CASES) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.TIER_CASES))
def test_tier_plan_matches_brute_force(name):
    """nnhipConvTranspose2dPlan per phase = the brute-force counts = the restated phase_axis / phase_taps; `auto` = the restated
    resolve_route; the bias-only pixels the GPU tests look at are the pixels no tap divides into."""
    _load()
    g = R.normalise(R.TIER_CASES[name])
    rc, route, taps, pixels = plan(make_desc(g))
    assert rc == g["sh"] * g["sw"]
    bt, bp = R.phase_tap_pixel_counts(g)
    assert taps == bt and pixels == bp
    assert sum(t * p for t, p in zip(taps, pixels)) == R.tap_pixel_pairs(g)
    fp = R.forward_plan(g)
    assert [p["taps"] for p in fp["phases"]] == taps and [p["pixels"] for p in fp["phases"]] == pixels
    assert route == R.auto_route(g)
    none = np.array([[not any((y + g["pu"] - r * g["dh"]) % g["sh"] == 0 for r in range(g["kh"])) or
                      not any((x + g["pl"] - s * g["dw"]) % g["sw"] == 0 for s in range(g["kw"]))
                      for x in range(g["Wo"])] for y in range(g["Ho"])])
    np.testing.assert_array_equal(R.tapless_pixels(g), none)


def test_tier_table_reaches_every_condition():
    """What the GPU tests of the tier table run, from the selection rules restated in convtranspose_ref.py (forward_plan:
    launch_conv_phase and the head of conv_phase_kernel; backward_plan: launch_conv_tap and conv_mfma_wgrad; auto_route: make_plan and
    resolve_route).  One assertion per condition, so that a row taken out of the table names what it alone provided."""
    _load()
    fwd, bwd, routes = {}, {}, {}
    for name, geom in R.TIER_CASES.items():
        g = R.normalise(geom)
        routes[name] = plan(make_desc(g))[1]
        assert routes[name] == R.auto_route(g), name
        if g["sh"] * g["sw"] > 1:                                          # the rows on which the phase kernel and the stride > 1 backward run
            fwd[name], bwd[name] = dict(R.forward_plan(g), g=g), dict(R.backward_plan(g), g=g)
            assert R.forced_route(g, ROUTE_PHASE) == ROUTE_PHASE and R.forced_route(g, ROUTE_GATHER) == ROUTE_GATHER
        else:
            assert R.forced_route(g, ROUTE_PHASE) == routes[name] != ROUTE_PHASE

    def rows(pred, table=fwd):
        return sorted(n for n, p in table.items() if pred(p))

    def live(p):                                                           # the phases that launch a block that does not return at once
        return [q for q in p["phases"] if q["pixels"]]

    for wm in (1, 2):
        assert rows(lambda p: p["wm"] == wm), f"no row runs conv_phase_kernel<{wm}>"
        for what, pred in (("T = 0", lambda t: t == 0), ("T = 1", lambda t: t == 1), ("even T >= 2", lambda t: t >= 2 and t % 2 == 0),
                           ("odd T >= 3", lambda t: t >= 3 and t % 2 == 1)):
            assert rows(lambda p: p["wm"] == wm and any(pred(q["T"]) for q in live(p))), f"no phase with {what} at WM = {wm}"
        assert rows(lambda p: p["wm"] == wm and p["ctiles"] >= 2 and any(q["T"] == 0 for q in live(p))), \
            f"no empty phase next to phases of more than one channel tile at WM = {wm}"
        assert rows(lambda p: p["wm"] == wm and p["ctiles"] % 2 == 1 and p["ctiles"] >= 3 and any(q["taps"] >= 2 for q in live(p))), \
            f"no row at WM = {wm} whose fetch moves to the next tap in the middle of a pair of k-tiles (odd channel tiles, >= 2 taps)"
    for n in (1, 2):
        assert rows(lambda p: p["m_tiles"] == n), f"no row with {n} m-tile(s)"
    assert rows(lambda p: p["g"]["Cout"] == 64 and any(q["T"] == 0 for q in live(p))), "no empty phase at WM = 1 with a full 64-row tile"
    assert rows(lambda p: p["wm"] == 2 and p["m_tiles"] == 2 and any(q["T"] == 0 for q in live(p))), "no empty phase at WM = 2 with two m-tiles"
    for what, pred in (("1", lambda c: c == 1), ("2", lambda c: c == 2), (">= 3", lambda c: c >= 3)):
        assert rows(lambda p: pred(p["ctiles"])), f"no row with {what} channel tile(s)"
    for wm in (1, 2):
        assert rows(lambda p: p["wm"] == wm and any(q["pixels"] == 0 for q in p["phases"])), f"no phase with zero pixels at WM = {wm}"
    assert rows(lambda p: p["grid_n"] >= 2 and any(0 < q["tiles"] < p["grid_n"] for q in p["phases"])), \
        "no phase with fewer pixel tiles than the largest phase's >= 2 (the `n0 >= N` return)"
    assert rows(lambda p: any(q["tiles"] >= 2 and q["spans"] for q in p["phases"])), "no pixel tile that spans two images in a phase of >= 2 tiles"
    assert rows(lambda p: len({q["N"] for q in live(p)}) >= 3 and any(q["spans"] for q in live(p))), \
        "no row with pixel tiles that span images in phases of unequal sizes"
    for wm in (1, 2):
        assert rows(lambda p: p["wm"] == wm and any(q["tiles"] >= 8 and q["N"] % (256 // wm) for q in p["phases"])), \
            f"no row with many pixel tiles and a ragged last one at WM = {wm}"

    def strided_subset(p):
        return 1 < p["rstep"] < p["g"]["sh"] or 1 < p["sstep"] < p["g"]["sw"]

    assert rows(strided_subset), "no row with 1 < rstep < stride"
    assert rows(lambda p: p["wm"] == 2 and strided_subset(p)), "no row with 1 < rstep < stride at the 128-row tile"
    assert rows(lambda p: p["wm"] == 2 and p["g"]["dh"] != p["g"]["dw"] and p["g"]["sh"] != p["g"]["sw"]), \
        "no row with unequal dilations and strides at the 128-row tile"
    assert rows(lambda p: p["wm"] == 2 and (p["g"]["sh"] > p["g"]["kh"] or p["g"]["sw"] > p["g"]["kw"])), \
        "no row with stride > kernel at the 128-row tile"
    for route, word in ((ROUTE_PHASE, "phase"), (ROUTE_GATHER, "gather"), (ROUTE_CONV2D, "conv2d")):
        assert [n for n, r in routes.items() if r == route], f"`auto` resolves to {word} on no row"
    assert [n for n, r in routes.items() if r == ROUTE_GATHER and n not in fwd], "no stride-1 row that is not a Conv2d"

    # the backward
    for wm in (1, 2):
        assert rows(lambda p: p["dx_wm"] == wm, bwd), f"no row runs dX on conv_tap_kernel<false, {wm}>"
    for pair in ((1, 32), (1, 64), (1, 128), (1, 256), (2, 32), (2, 64), (2, 128)):
        assert rows(lambda p: p["wg"] == pair, bwd), f"no row runs conv_wgrad_mfma_kernel<WM, CB> = {pair}"
    for flag in ("flat", "avec"):
        for on in (True, False):
            assert rows(lambda p: p[flag] is on, bwd), f"no row with {flag.upper()} {'on' if on else 'off'}"


# ---- ABI edges (no device work: argument checks come first) -------------------------------------------------------------------
def test_abi_edges():
    _load()
    from neunet_hip._lib import last_error, load_hip_function
    fwd, bwd = load_hip_function("nnhipConvTranspose2dForward"), load_hip_function("nnhipConvTranspose2dBackward")
    g = R.normalise(R.GEOMETRIES["convt_k4s2p1"])
    ptr = ctypes.c_void_p(256)                                             # never dereferenced

    def rejected(rc, word):
        assert rc == EINVAL
        assert word in last_error(), last_error()

    rejected(fwd(ptr, ptr, ptr, ptr, None, None), "null descriptor")
    rejected(bwd(ptr, ptr, ptr, ptr, ptr, ptr, None, None), "null descriptor")
    for over, word in ((dict(oph=2), "output_padding"), (dict(opw=2), "output_padding"), (dict(sh=0), "bad descriptor"),
                       (dict(sw=-1), "bad descriptor"), (dict(pu=8, pd=8), "empty output"), (dict(B=1 << 20, H=64, W=64), "2 GiB")):
        d = make_desc(g, **over)
        rejected(fwd(ptr, ptr, ptr, ptr, ctypes.byref(d), None), word)
        rejected(bwd(ptr, ptr, ptr, ptr, ptr, ptr, ctypes.byref(d), None), word)
        rejected(plan(d, capacity=64)[0], word)
    d = make_desc(g)
    rejected(fwd(None, ptr, ptr, ptr, ctypes.byref(d), None), "null pointer")
    rejected(bwd(ptr, ptr, None, ptr, ptr, ptr, ctypes.byref(d), None), "null pointer")
    rejected(plan(d, capacity=3)[0], "capacity")
    # output padding up to max(stride, dilation) - 1: stride 2, dilation 3 takes 2
    assert plan(make_desc(R.normalise(R.GEOMETRIES["convt_op_ge_s"])))[0] == 4
    # an empty batch is fine and launches nothing (no pointer is looked at)
    d0 = make_desc(g, B=0)
    assert fwd(None, None, None, None, ctypes.byref(d0), None) == 0
    assert bwd(None, None, None, None, None, None, ctypes.byref(d0), None) == 0


def test_route_switch_round_trip():
    _load()
    from neunet_hip._lib import load_hip_function
    import neunet_hip
    setr, getr = load_hip_function("nnhipSetConvTransposeRoute"), load_hip_function("nnhipGetConvTransposeRoute")
    assert getr() == 0
    with neunet_hip.conv_transpose_route("gather"):
        assert getr() == 2
        with neunet_hip.conv_transpose_route("phase"):
            assert getr() == 1
        assert getr() == 2
    assert getr() == 0
    assert setr(7) == 0 and getr() == 0                                    # an unknown route changes nothing
    with pytest.raises(ValueError):
        neunet_hip.conv_transpose_route("fastest")


# ---- the host module ---------------------------------------------------------------------------------------------------------
def test_module_constructor_and_reference_state_dict(golden):
    import neunet_hip.nn as nn
    from neunet_hip.nn.experimental import HIPConvTranspose2d
    assert nn.ConvTranspose2d is HIPConvTranspose2d
    layer = HIPConvTranspose2d(3, 5, (4, 4), (2, 2), (1, 1), device="cpu")
    assert (layer.in_channels, layer.out_channels, layer.kernel_size, layer.stride) == (3, 5, (4, 4), (2, 2))
    assert (layer.padding, layer.dilation, layer.output_padding) == ((1, 1, 1, 1), (1, 1), (0, 0))
    assert layer.weight.shape == (5, 3, 4, 4) and layer.bias.shape == (5,)
    bound = 1.0 / np.sqrt(3 * 4 * 4)
    assert np.abs(layer.weight.data).max() <= bound and not layer.bias.data.any()
    assert [tuple(p.shape) for p in layer.parameters()] == [(5, 3, 4, 4), (5,)]
    # positional order of the reference's constructor: ..., dilation, output_padding, bias
    odd = HIPConvTranspose2d(2, 3, 3, 2, (1, 2, 0, 1), 3, 1, False, device="cpu")
    assert (odd.kernel_size, odd.stride, odd.padding, odd.dilation, odd.output_padding, odd.bias) == \
        ((3, 3), (2, 2), (1, 2, 0, 1), (3, 3), (1, 1), None)
    with pytest.raises(ValueError):
        HIPConvTranspose2d(2, 3, 3, padding="same", device="cpu")
    # a state_dict the reference wrote for the same layer
    f = golden("convt_state")
    assert list(f["keys"]) == list(layer.state_dict())
    layer.load_state_dict({k: f[k] for k in f["keys"]})
    np.testing.assert_array_equal(layer.weight.data, f["weight"])
    np.testing.assert_array_equal(layer.bias.data, f["bias"].reshape(-1))


def test_glue_on_host_tensors():
    """concatenate / add_channel_bias keep the tape on host tensors too (the device path is tested on the GPU)."""
    import neunet_hip
    rng = np.random.default_rng(0)
    a, b = neunet_hip.tensor(rng.standard_normal((2, 3, 4, 5))), neunet_hip.tensor(rng.standard_normal((2, 5, 4, 5)))
    c = neunet_hip.concatenate(a, b, axis=1)
    g = rng.standard_normal(c.shape).astype(np.float32)
    c.backward(g)
    np.testing.assert_array_equal(c.data, np.concatenate([a.data, b.data], 1))
    np.testing.assert_array_equal(a.grad, g[:, :3])
    np.testing.assert_array_equal(b.grad, g[:, 3:])
    h, t = neunet_hip.tensor(rng.standard_normal((2, 3, 4, 5))), neunet_hip.tensor(rng.standard_normal((2, 3)))
    o = neunet_hip.add_channel_bias(h, t)
    g = rng.standard_normal(o.shape).astype(np.float32)
    o.backward(g)
    np.testing.assert_array_equal(o.data, h.data + t.data[:, :, None, None])
    np.testing.assert_array_equal(h.grad, g)
    np.testing.assert_allclose(t.grad, g.sum((2, 3)), rtol=1e-6)
    with pytest.raises(ValueError):
        neunet_hip.add_channel_bias(h, neunet_hip.tensor(np.zeros((2, 4))))
    with pytest.raises(ValueError):
        h.add(t)                                                           # Tensor.add keeps refusing broadcasts
