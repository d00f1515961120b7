"""GPU: ConvTranspose2d through the C ABI (include/neunet_hip.h) on both stride > 1 routes -- the stride-phase kernel of
csrc/conv_transpose.hip and the Conv2d input-gradient gather -- and through nn.ConvTranspose2d, against the reference's recorded
outputs (tests/golden/convt_*.npz) and the float64 restatement of tests/convtranspose_ref.py; the U-Net glue; and one training
step of the reference's DDPM U-Net (tests/golden/ddpm_unet.npz) through examples/ddpm_unet.py.

Bounds.  O, dX, dW, db: the project's 1e-4 of max(|ref|, rms(ref)) per element against float64 (assert_close_scaled) and
rtol = atol = 1e-4 (test_hip_parity.TOL) against the float32 fixture.  At the tile-edge shapes O is also held to the dot-product
bound 32 * 2^-24 * sum|x||w| + 4 * 2^-24 * |ref| (assert_dot_close's, with the sum taken through the restatement on |X|, |W|),
and the two routes to twice that of each other.  Each test prints its largest error / bound ratio before it asserts (-s).

The tier table (convtranspose_ref.TIER_CASES; tests/test_convtranspose.py checks on the CPU which template instantiation, k-loop
length, phase size and weight-gradient configuration each row reaches): O as above on both routes; dX and dW additionally within the
same dot bound with the sums taken by the restated backward on |X|, |W|, |dO|; db within 4 * 2^-24 * sum|dO| + 2^-24 |ref|.  The
pixels of a stride phase without a tap hold the bias (or 0) bit for bit; repeated calls, calls with an output left out, `auto`
against the forced route and a captured graph's replays are bit-identical; operands and outputs that start one float into their
buffers leave the sentinels around the outputs alone.  None of the bounds is tuned: float32 numpy einsums stand at 0.11 (O), 0.07
(dX), 0.13 (dW) and 0.18 (db) of them on this table, the kernels at 0.12, 0.08, 0.11 and 0.21 (EXPERIMENTS.md 5.15b)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import convtranspose_ref as R
from test_hip_parity import TOL, assert_close_scaled, assert_within, grad_list_scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN = float("nan")
FIELDS = "B Cin H W Cout kh kw sh sw dh dw pu pd pl pr oph opw".split()
ROUTES = {"phase": 1, "gather": 2}
# ragged channel tiles on both sides, pixel tiles that span images, 18 k-tiles at BK = 16 / exactly one 128-row tile at the
# notebook's batch / a 2 x 2 output / one output channel
EDGES = {"ragged": (3, 70, 5, 7, 130, 4, 2, 1, 1, 0), "one_m_tile": (5, 128, 4, 4, 128, 4, 2, 1, 1, 0),
         "tiny": (1, 1, 1, 1, 1, 4, 2, 1, 1, 0), "one_cout": (2, 130, 3, 3, 1, 3, 2, 0, 1, 1)}


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
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()   # a copy: the shared references are read-only


def host(t):
    return t.detach().cpu().numpy()


def make_desc(g):
    from neunet_hip._lib import ConvTranspose2dDesc
    return ConvTranspose2dDesc(*[g[k] for k in FIELDS])


def forward(route, X, W, b, g, fill=NAN):
    """nnhipConvTranspose2dForward on `route` into a buffer pre-filled with NaN; the previous route comes back afterwards."""
    from neunet_hip._lib import load_hip_function
    O = torch.full((g["B"], g["Cout"], g["Ho"], g["Wo"]), fill, device="cuda")
    d = make_desc(g)
    prev = load_hip_function("nnhipSetConvTransposeRoute")(ROUTES[route])
    try:
        call("nnhipConvTranspose2dForward", X, W, b, O, ctypes.byref(d))
        torch.cuda.synchronize()
    finally:
        load_hip_function("nnhipSetConvTransposeRoute")(prev)
    return O


def backward(X, W, dO, g, want=(True, True, True), fill=NAN):
    outs = [torch.full(s, fill, device="cuda") if w else None
            for s, w in zip((X.shape, W.shape, (g["Cout"],)), want)]
    d = make_desc(g)
    call("nnhipConvTranspose2dBackward", X, W, dO, outs[0], outs[1], outs[2], ctypes.byref(d))
    torch.cuda.synchronize()
    return outs


def report(tag, got, ref):
    ref = np.asarray(ref, np.float64)
    scale = np.maximum(np.abs(ref), np.sqrt(np.mean(ref ** 2))) + 1e-30
    print(f"{tag}: max |err| / (1e-4 scale) = {np.nanmax(np.abs(got - ref) / (1e-4 * scale)):.3f}")


# ---- the fixtures from the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", sorted(R.GEOMETRIES))
def test_fixture_c_abi(hip, golden, name, route):
    f, g = golden(name), R.normalise(R.GEOMETRIES[name])
    X, W, b, dO = dev(f["X"]), dev(f["W"]), dev(f["b"]), dev(f["dO"])
    O = host(forward(route, X, W, b, g))
    assert not np.isnan(O).any(), "output pixels left unwritten (the bias-only pixels of an empty phase?)"
    ref = R.forward(f["X"], f["W"], f["b"], g)
    report(f"{name} {route} O", O, ref)
    assert_close_scaled(O, ref, tol=1e-4, err_msg="O vs float64")
    np.testing.assert_allclose(O, f["O"], **TOL)
    dX, dW, db = (host(t) for t in backward(X, W, dO, g))
    rdX, rdW, rdb = R.backward(f["X"], f["W"], f["dO"], g)
    for tag, got, r64, r32 in (("dX", dX, rdX, f["dX"]), ("dW", dW, rdW, f["dW"]), ("db", db, rdb, f["db"].reshape(-1))):
        assert not np.isnan(got).any(), f"{tag} not fully written"
        report(f"{name} {tag}", got, r64)
        assert_close_scaled(got, r64, tol=1e-4, err_msg=f"{tag} vs float64")
        np.testing.assert_allclose(got, r32, **TOL)


@pytest.mark.parametrize("name", sorted(R.GEOMETRIES))
def test_fixture_module(hip, golden, name):
    from neunet_hip.nn.experimental import HIPConvTranspose2d
    f, g = golden(name), R.normalise(R.GEOMETRIES[name])
    layer = HIPConvTranspose2d(g["Cin"], g["Cout"], (g["kh"], g["kw"]), (g["sh"], g["sw"]), (g["pu"], g["pd"], g["pl"], g["pr"]),
                               (g["dh"], g["dw"]), (g["oph"], g["opw"]))
    layer.weight.data.copy_(dev(f["W"]))
    layer.bias.data.copy_(dev(f["b"]))
    w_before = host(layer.weight.data).copy()
    x = hip.Tensor(f["X"], device="cuda")
    y = layer(x)
    assert y.shape == f["O"].shape
    y.backward(dev(f["dO"]))
    rO = R.forward(f["X"], f["W"], f["b"], g)
    rdX, rdW, rdb = R.backward(f["X"], f["W"], f["dO"], g)
    for tag, got, r64, r32 in (("O", host(y.data), rO, f["O"]), ("dX", host(x.grad), rdX, f["dX"]),
                               ("dW", host(layer.weight.grad), rdW, f["dW"]),
                               ("db", host(layer.bias.grad).reshape(-1), rdb, f["db"].reshape(-1))):
        assert_close_scaled(got, r64, tol=1e-4, err_msg=f"{tag} vs float64")
        np.testing.assert_allclose(got, r32, **TOL)
    np.testing.assert_array_equal(host(layer.weight.data), w_before)      # never mutated (the reference dilates it in place)


# ---- tile edges ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_cases():
    """name -> (g, X, W, b, dO, float64 O, its dot bound, float64 (dX, dW, db)): computed once, shared, never changed."""
    out = {}
    for name, geom in EDGES.items():
        g, X, W, b, dO = R.make_case(geom, 7)
        ref = R.forward(X, W, b, g)
        out[name] = (g, X, W, b, dO, ref, R.dot_bound(X, W, ref, g), R.backward(X, W, dO, g))
    return out


@pytest.mark.parametrize("name", sorted(EDGES))
def test_tile_edges_both_routes(hip, edge_cases, name):
    g, X, W, b, dO, ref, bound, (rdX, rdW, rdb) = edge_cases[name]
    Xd, Wd, bd = dev(X), dev(W), dev(b)
    outs = {}
    for route in sorted(ROUTES):
        O = host(forward(route, Xd, Wd, bd, g))
        assert not np.isnan(O).any()
        print(f"{name} {route}: max |err| / dot bound = {np.max(np.abs(O - ref) / bound):.3f}")
        assert_within(O, ref, bound, f"{route} O vs float64 (dot bound)")
        assert_close_scaled(O, ref, tol=1e-4, err_msg=f"{route} O vs float64")
        again = host(forward(route, Xd, Wd, bd, g))
        np.testing.assert_array_equal(O, again, err_msg=f"{route}: two runs differ")
        outs[route] = O
    assert_within(outs["phase"], outs["gather"], 2 * bound, "phase vs gather")
    # without a bias the bias-only pixels are zeros
    O0 = host(forward("phase", Xd, Wd, None, g))
    assert_within(O0, ref - b.reshape(1, -1, 1, 1).astype(np.float64), bound, "phase, no bias")
    dX, dW, db = (host(t) for t in backward(Xd, Wd, dev(dO), g))
    for tag, got, r in (("dX", dX, rdX), ("dW", dW, rdW), ("db", db, rdb)):
        assert not np.isnan(got).any(), f"{tag} not fully written"
        report(f"{name} {tag}", got, r)
        assert_close_scaled(got, r, tol=1e-4, err_msg=f"{tag} vs float64")


@pytest.mark.parametrize("name", ["convt_k4s2p1", "convt_s3k2", "convt_unet_out"])
def test_skipped_outputs_leave_the_others_unchanged(hip, golden, name):
    """dX / dW / db NULL: the remaining outputs are bit for bit those of the full call (stride > 1, empty phases, and the
    stride-1 layer that runs as a Conv2d)."""
    f, g = golden(name), R.normalise(R.GEOMETRIES[name])
    X, W, dO = dev(f["X"]), dev(f["W"]), dev(f["dO"])
    full = [host(t) for t in backward(X, W, dO, g)]
    for skip in range(3):
        want = tuple(i != skip for i in range(3))
        part = backward(X, W, dO, g, want=want)
        assert part[skip] is None
        for i in range(3):
            if i != skip:
                np.testing.assert_array_equal(host(part[i]), full[i], err_msg=f"output {i} with output {skip} skipped")
    only_db = backward(X, W, dO, g, want=(False, False, True))
    np.testing.assert_array_equal(host(only_db[2]), full[2])


# ---- every tier on irregular geometry (convtranspose_ref.TIER_CASES; tests/test_convtranspose.py says what the table reaches) --------
SETTINGS = dict(ROUTES, auto=0)
SENTINEL = -7.0
NULL_ROWS = ("k2s3_w2", "gcd_w2", "bw_w2_cb64")
GUARD_ROWS = ("k3s2_w2", "uneq_tiles_w2", "nopix_w2", "uneven_w1", "k1s2_w1")


def tier_routes(name):
    """the routes a row is run on: both at stride > 1, else the one resolve_route dictates whatever is asked for"""
    g = R.normalise(R.TIER_CASES[name])
    return ["gather", "phase"] if g["sh"] * g["sw"] > 1 else [{R.ROUTE_GATHER: "gather", R.ROUTE_CONV2D: "conv2d"}[R.auto_route(g)]]


@pytest.fixture(scope="module")
def tier_cases():
    """name -> the seeded float32 inputs, the float64 O / (dX, dW, db) and their bounds: computed once, shared, read-only."""
    out = {}
    for name, geom in R.TIER_CASES.items():
        g, X, W, b, dO = R.make_case(geom, 11)
        ref = R.forward(X, W, b, g)
        grads = R.backward(X, W, dO, g)
        ref0 = R.forward(X, W, None, g)
        asum = 32 * 2.0 ** -24 * R.abs_sum(X, W, g)                        # R.dot_bound's first term: the same with and without a bias
        c = dict(g=g, X=X, W=W, b=b, dO=dO, O=ref, bound=asum + 4 * 2.0 ** -24 * np.abs(ref), O0=ref0, bound0=asum + 4 * 2.0 ** -24 * np.abs(ref0),
                 grads=grads, gbounds=R.backward_bounds(X, W, dO, grads, g))
        for v in (X, W, b, dO, ref, c["bound"], ref0, c["bound0"]) + tuple(grads) + tuple(c["gbounds"]):
            v.setflags(write=False)
        out[name] = c
    return out


def forward_into(setting, X, W, b, O, g):
    """nnhipConvTranspose2dForward into O with the route switch at `setting`; the previous setting comes back afterwards."""
    from neunet_hip._lib import load_hip_function
    d = make_desc(g)
    prev = load_hip_function("nnhipSetConvTransposeRoute")(SETTINGS[setting])
    try:
        call("nnhipConvTranspose2dForward", X, W, b, O, ctypes.byref(d))
    finally:
        load_hip_function("nnhipSetConvTransposeRoute")(prev)
    return O


def tier_forward(route, X, W, b, g):
    """into NaN; a stride-1 row ("conv2d", or "gather" where the layer is no Conv2d) is asked for the phase route and must not follow"""
    O = torch.full((g["B"], g["Cout"], g["Ho"], g["Wo"]), NAN, device="cuda")
    forward_into("phase" if g["sh"] * g["sw"] == 1 else route, X, W, b, O, g)
    torch.cuda.synchronize()
    return host(O)


def ratio(got, ref, bound):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / np.maximum(bound, 1e-300))) if np.size(ref) else 0.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_forward(tag, O, c, bias=True):
    ref, bound = (c["O"], c["bound"]) if bias else (c["O0"], c["bound0"])   # O0: the float64 sum without the bias (= O - b)
    scale = 1e-4 * np.maximum(np.abs(ref), np.sqrt(np.mean(ref ** 2))) + 1e-30
    print(f"{tag}: max |err| / dot bound = {ratio(O, ref, bound):.3f}, / (1e-4 scale) = {ratio(O, ref, scale):.3f}")
    assert not np.isnan(O).any(), f"{tag}: output pixels left unwritten"
    assert_within(O, ref, bound, f"{tag} vs float64 (dot bound)")
    assert_close_scaled(O, ref, tol=1e-4, err_msg=f"{tag} vs float64")
    # the pixels of the phases without a tap hold the bias (or zero) itself, not a sum that rounds to it
    mask = R.tapless_pixels(c["g"])
    want = np.broadcast_to((c["b"] if bias else np.zeros_like(c["b"])).reshape(1, -1, 1), O[:, :, mask].shape)
    np.testing.assert_array_equal(bits(O[:, :, mask] + 0.0), bits(want), err_msg=f"{tag}: bias-only pixels")


def check_backward(tag, got, c):
    worst = {}
    for k, o, r, bd in zip(("dX", "dW", "db"), got, c["grads"], c["gbounds"]):
        if o is None:
            continue
        scale = 1e-4 * np.maximum(np.abs(r), np.sqrt(np.mean(r ** 2))) + 1e-30
        worst[k] = ratio(o, r, bd)
        print(f"{tag} {k}: max |err| / {'sum' if k == 'db' else 'dot'} bound = {worst[k]:.3f}, / (1e-4 scale) = {ratio(o, r, scale):.3f}")
    for k, o, r, bd in zip(("dX", "dW", "db"), got, c["grads"], c["gbounds"]):
        if o is None:
            continue
        assert not np.isnan(o).any(), f"{tag} {k} not fully written"
        assert_close_scaled(o, r, tol=1e-4, err_msg=f"{tag} {k} vs float64")
        assert_within(o, r, bd, f"{tag} {k} vs float64 ({'sum' if k == 'db' else 'dot'} bound)")
    return worst


@pytest.mark.parametrize("name,route", [(n, r) for n in R.TIER_CASES for r in tier_routes(n)])
def test_tier_forward(hip, tier_cases, name, route):
    c = tier_cases[name]
    g = c["g"]
    Xd, Wd, bd = dev(c["X"]), dev(c["W"]), dev(c["b"])
    O = tier_forward(route, Xd, Wd, bd, g)
    check_forward(f"{name} {route} O", O, c)
    np.testing.assert_array_equal(bits(O), bits(tier_forward(route, Xd, Wd, bd, g)), err_msg=f"{route}: two runs differ")
    check_forward(f"{name} {route} O, no bias", tier_forward(route, Xd, Wd, None, g), c, bias=False)
    if g["sh"] * g["sw"] > 1:
        other = tier_forward("gather" if route == "phase" else "phase", Xd, Wd, bd, g)
        print(f"{name} {route} vs the other route: max |diff| / (2 dot bound) = {ratio(O, other.astype(np.float64), 2 * c['bound']):.3f}")
        assert_within(O, other, 2 * c["bound"], "phase vs gather")


@pytest.mark.parametrize("name", list(R.TIER_CASES))
def test_tier_backward(hip, tier_cases, name):
    c = tier_cases[name]
    g = c["g"]
    Xd, Wd, dOd = dev(c["X"]), dev(c["W"]), dev(c["dO"])
    full = [host(t) for t in backward(Xd, Wd, dOd, g)]
    check_backward(name, full, c)
    for k, a, b_ in zip(("dX", "dW", "db"), full, backward(Xd, Wd, dOd, g)):
        np.testing.assert_array_equal(bits(a), bits(host(b_)), err_msg=f"{k}: two runs differ")
    if name in NULL_ROWS:
        for skip in range(3):
            part = backward(Xd, Wd, dOd, g, want=tuple(i != skip for i in range(3)))
            assert part[skip] is None
            for i in range(3):
                if i != skip:
                    np.testing.assert_array_equal(bits(host(part[i])), bits(full[i]), err_msg=f"output {i} with output {skip} skipped")


class Fenced:
    """A tensor that starts one float into a larger buffer -- 4-byte but not 16-byte aligned -- with 65 floats of SENTINEL before it and
    64 after it (torch's allocations are 512-byte aligned); with `data`: an operand, one float in, nothing behind it."""

    def __init__(self, shape, fill=NAN, data=None):
        n = int(np.prod(shape))
        self.lo = 1 if data is not None else 65
        self.buf = torch.full((self.lo + n + (0 if data is not None else 64),), SENTINEL, device="cuda")
        self.view = self.buf[self.lo:self.lo + n].view(*shape)
        assert self.view.data_ptr() % 16 == 4 and self.buf.data_ptr() % 16 == 0
        if data is not None:
            self.view.copy_(dev(data))
        else:
            self.view.fill_(fill)

    def intact(self):
        b = host(self.buf)
        n = self.view.numel()
        return bool((bits(b[:self.lo]) == bits(np.float32(SENTINEL))).all() and (bits(b[self.lo + n:]) == bits(np.float32(SENTINEL))).all())


@pytest.mark.parametrize("name", GUARD_ROWS)
def test_guard_bands_and_unaligned_operands(hip, tier_cases, name):
    """Every operand and output one float into its buffer (no float4 store in conv_tap_kernel, no 16-byte dO load in the weight
    gradient), the outputs between sentinels that must keep their bits: a store the kernel should have skipped, or one past a
    tensor's end, lands on them."""
    c = tier_cases[name]
    g = c["g"]
    X, W, b, dO = (Fenced(c[k].shape, data=c[k]) for k in ("X", "W", "b", "dO"))
    for route in tier_routes(name):
        O = Fenced((g["B"], g["Cout"], g["Ho"], g["Wo"]))
        forward_into(route, X.view, W.view, b.view, O.view, g)
        torch.cuda.synchronize()
        check_forward(f"{name} {route} O, one float in", host(O.view), c)
        assert O.intact(), f"{route}: wrote outside O"
    outs = [Fenced(s) for s in (c["X"].shape, c["W"].shape, c["b"].shape)]
    call("nnhipConvTranspose2dBackward", X.view, W.view, dO.view, outs[0].view, outs[1].view, outs[2].view, ctypes.byref(make_desc(g)))
    torch.cuda.synchronize()
    check_backward(f"{name}, one float in,", [host(o.view) for o in outs], c)
    for k, o in zip(("dX", "dW", "db"), outs):
        assert o.intact(), f"wrote outside {k}"
    assert all(t.intact() for t in (X, W, b, dO))


@pytest.mark.parametrize("name", ["k3s2_w2", "k2s3_w2", "s1_bigpad_w2", "s1_conv_w2"])
def test_route_auto_matches_the_forced_route(hip, tier_cases, name):
    """`auto` = the route the restated resolve_route names, bit for bit: phase, gather (empty phases), gather (stride 1), conv2d."""
    from neunet_hip._lib import load_hip_function
    c = tier_cases[name]
    g = c["g"]
    Xd, Wd, bd = dev(c["X"]), dev(c["W"]), dev(c["b"])
    resolved = {R.ROUTE_PHASE: "phase", R.ROUTE_GATHER: "gather", R.ROUTE_CONV2D: "conv2d"}[R.auto_route(g)]
    outs = {}
    before = load_hip_function("nnhipGetConvTransposeRoute")()
    try:
        for setting in ("auto", "phase", "gather"):
            O = torch.full((g["B"], g["Cout"], g["Ho"], g["Wo"]), NAN, device="cuda")
            outs[setting] = host(forward_into(setting, Xd, Wd, bd, O, g))
    finally:
        load_hip_function("nnhipSetConvTransposeRoute")(before)
    assert load_hip_function("nnhipGetConvTransposeRoute")() == before
    print(f"{name}: auto -> {resolved}")
    if resolved == "conv2d":
        O = torch.full((g["B"], g["Cout"], g["Ho"], g["Wo"]), NAN, device="cuda")
        eh, ew = g["dh"] * (g["kh"] - 1), g["dw"] * (g["kw"] - 1)
        from neunet_hip._lib import Conv2dDesc
        cd = Conv2dDesc(g["B"], g["Cin"], g["H"], g["W"], g["Cout"], g["kh"], g["kw"], 1, 1, g["dh"], g["dw"],
                        eh - g["pu"], eh - g["pd"] + g["oph"], ew - g["pl"], ew - g["pr"] + g["opw"])
        call("nnhipConv2dForward", Xd, Wd, bd, O, ctypes.byref(cd))
        outs["conv2d"] = host(O)
    np.testing.assert_array_equal(bits(outs["auto"]), bits(outs[resolved]))
    if g["sh"] * g["sw"] == 1:                                            # nothing to force at stride 1
        np.testing.assert_array_equal(bits(outs["phase"]), bits(outs["auto"]))
        np.testing.assert_array_equal(bits(outs["gather"]), bits(outs["auto"]))
    check_forward(f"{name} auto O", outs["auto"], c)


@pytest.mark.parametrize("name", ["k3s2_w1", "k3s2_c3_w2"])
def test_phase_forward_in_a_captured_graph(hip, tier_cases, name):
    """One forward on the phase route (weight repack + conv_phase_kernel) captured on one stream after an eager call has sized the
    workspace and set the kernel's shared-memory attribute; two replays into NaN equal the eager bits."""
    from neunet_hip._lib import load_hip_function
    c = tier_cases[name]
    g = c["g"]
    assert R.forward_plan(g)["wm"] == (2 if name.endswith("w2") else 1)
    Xd, Wd, bd = dev(c["X"]), dev(c["W"]), dev(c["b"])
    eager = tier_forward("phase", Xd, Wd, bd, g)
    check_forward(f"{name} phase O, eager", eager, c)
    O = torch.full((g["B"], g["Cout"], g["Ho"], g["Wo"]), NAN, device="cuda")
    d = make_desc(g)
    torch.cuda.synchronize()
    prev = load_hip_function("nnhipSetConvTransposeRoute")(ROUTES["phase"])
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            call("nnhipConvTranspose2dForward", Xd, Wd, bd, O, ctypes.byref(d))
    finally:
        load_hip_function("nnhipSetConvTransposeRoute")(prev)
    torch.cuda.synchronize()
    assert bool(torch.isnan(O).all()), "capturing runs nothing"
    for replay in range(2):
        O.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(host(O)), bits(eager), err_msg=f"replay {replay}")
    del graph


def test_tier_batch_zero_touches_nothing(hip, tier_cases):
    c = tier_cases["k3s2_w2"]
    g = dict(c["g"], B=0)
    Xd, Wd, bd, dOd = dev(c["X"]), dev(c["W"]), dev(c["b"]), dev(c["dO"])
    outs = [Fenced(s) for s in (c["O"].shape, c["X"].shape, c["W"].shape, c["b"].shape)]
    for route in ("phase", "gather"):
        forward_into(route, Xd, Wd, bd, outs[0].view, g)
    call("nnhipConvTranspose2dBackward", Xd, Wd, dOd, outs[1].view, outs[2].view, outs[3].view, ctypes.byref(make_desc(g)))
    torch.cuda.synchronize()
    for o in outs:
        assert o.intact() and bool(torch.isnan(o.view).all())


# ---- U-Net glue ---------------------------------------------------------------------------------------------------------------
def test_concatenate_and_add_channel_bias(hip):
    rng = np.random.default_rng(3)
    A, B_ = rng.standard_normal((2, 3, 4, 5)).astype(np.float32), rng.standard_normal((2, 5, 4, 5)).astype(np.float32)
    a, b = hip.Tensor(A, device="cuda"), hip.Tensor(B_, device="cuda")
    c = hip.concatenate(a, b, axis=1)
    G = rng.standard_normal(c.shape).astype(np.float32)
    c.backward(dev(G))
    np.testing.assert_array_equal(host(c.data), np.concatenate([A, B_], 1))
    np.testing.assert_array_equal(host(a.grad), G[:, :3])
    np.testing.assert_array_equal(host(b.grad), G[:, 3:])
    assert a.grad.is_contiguous() and b.grad.is_contiguous()
    H, T = rng.standard_normal((2, 3, 4, 5)).astype(np.float32), rng.standard_normal((2, 3)).astype(np.float32)
    h, t = hip.Tensor(H, device="cuda"), hip.Tensor(T, device="cuda")
    o = hip.add_channel_bias(h, t)
    G = rng.integers(-8, 9, o.shape).astype(np.float32)                   # small integers: the sum over H, W is exact in any order
    o.backward(dev(G))
    np.testing.assert_array_equal(host(o.data), H + T[:, :, None, None])
    np.testing.assert_array_equal(host(h.grad), G)
    np.testing.assert_array_equal(host(t.grad), G.sum((2, 3)))


# ---- the DDPM U-Net -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_ddpm_unet_step_vs_reference(hip, golden, tag):
    """One training step of the notebook's SimpleUNet as the reference ran it (a: 16 x 16, Conv2d in / ConvTranspose2d out;
    b: 12 x 12, ConvTranspose2d 5x5 in / Conv2d 5x5 out), through examples/ddpm_unet.py.  The bounds are those
    test_hip_parity.test_conv_classifier_golden applies to its fixture: |loss - ref| < 1e-6, the model output at rtol 1e-4 /
    atol 1e-5, every gradient within assert_close_scaled's 1e-4 of max(|ref|, rms(ref), grad_list_scale(all gradients)) (conv
    biases in front of a BatchNorm have a mathematically zero gradient).

    Parameters after the Adam step.  The first Adam step from zero moments is p - lr g / (|g| + eps) (optim.py:17-32 of the
    reference: m_hat = g, v_hat = g^2, eps = 1e-8), so its sensitivity to a gradient error dg is lr eps dg / (|g| + eps)^2.
    With e = the gradient bound above (1e-4 max(|g|, rms(g), gscale)) an element is CLEAR when |g_ref| > 2 e -- our gradient
    then has the reference's sign -- and is held to
        1e-4 lr  +  2 * 2^-24 |p_ref|  +  lr eps e / (|g_ref| - e)^2
    (the update to 1e-4 of its size, the float32 rounding of the stored parameter on either side, the sensitivity term: at most
    2.5 % of lr at the threshold, ~1e-4 lr for ordinary gradients).  An element left un-stepped, or stepped by another size or
    sign, is lr away and fails.  The remaining elements (gradient within rounding noise of zero: the update's SIGN is noise, the
    floor test_conv_classifier_golden states for its own trajectory) get 2 lr + the rounding term, and must be fewer than 5 %
    of the model (the fixture has 1.7 % / 2.3 %).  The reference's own float32 step is 0.32 / 0.29 of the clear bound away from
    the float64 formula (computed on the CPU from the fixture; EXPERIMENTS 5.15)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import ddpm_unet
    f = golden("ddpm_unet")
    cfg = [int(v) for v in f[f"{tag}_cfg"]]
    model = ddpm_unet.SimpleUNet(image_channels=cfg[0], image_size=cfg[1], down_channels=tuple(cfg[2:]))
    params = model.parameters()
    n = int(f[f"{tag}_n_params"])
    assert len(params) == n
    for i, p in enumerate(params):
        assert p.size == f[f"{tag}_p{i}"].size, f"parameter {i}: {p.shape} vs {f[f'{tag}_p{i}'].shape}"
        p.data.copy_(dev(f[f"{tag}_p{i}"]).reshape(p.shape))
    lr = 2e-4
    diffusion = ddpm_unet.Diffusion(model, timesteps=int(f["timesteps"]), lr=lr)
    x0, t, noise = f[f"{tag}_x0"], f[f"{tag}_t"], f[f"{tag}_noise"]
    np.testing.assert_array_equal(diffusion.noised(x0, t, noise), f[f"{tag}_x_t"])
    diffusion.optimizer.zero_grad()
    loss, pred = diffusion.loss(x0, t, noise)
    loss.backward()
    print(f"{tag}: loss {loss.item():.7f} vs {float(f[f'{tag}_loss']):.7f}")
    assert abs(loss.item() - float(f[f"{tag}_loss"])) < 1e-6
    np.testing.assert_allclose(host(pred.data), f[f"{tag}_pred"], rtol=1e-4, atol=1e-5)
    grads = [f[f"{tag}_g{i}"] for i in range(n)]
    gscale = grad_list_scale(grads)
    worst = 0.0
    for i, p in enumerate(params):
        ref = grads[i].reshape(p.shape).astype(np.float64)
        got = host(p.grad).reshape(p.shape)
        worst = max(worst, float(np.max(np.abs(got - ref) / (1e-4 * np.maximum(np.maximum(np.abs(ref), np.sqrt(np.mean(ref ** 2))), gscale)))))
    print(f"{tag}: worst gradient error / bound = {worst:.3f}")
    for i, p in enumerate(params):
        assert_close_scaled(host(p.grad).reshape(p.shape), grads[i].reshape(p.shape), err_msg=f"grad {i} {p.shape}", scale=gscale)
    diffusion.optimizer.step()
    eps, n_clear, n_all, worst_clear = 1e-8, 0, 0, 0.0
    checks = []
    for i, p in enumerate(params):
        g = grads[i].reshape(p.shape).astype(np.float64)
        ref = f[f"{tag}_p_after{i}"].reshape(p.shape).astype(np.float64)
        e = 1e-4 * np.maximum(np.maximum(np.abs(g), np.sqrt(np.mean(g ** 2))), gscale)
        clear = np.abs(g) > 2 * e
        rounding = 2 * 2.0 ** -24 * np.abs(ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            tight = 1e-4 * lr + rounding + lr * eps * e / (np.abs(g) - e) ** 2
        bound = np.where(clear, tight, 2 * lr + rounding)
        got = host(p.data).astype(np.float64)
        n_clear, n_all = n_clear + int(clear.sum()), n_all + clear.size
        if clear.any():
            worst_clear = max(worst_clear, float(np.max((np.abs(got - ref) / bound)[clear])))
        checks.append((i, got, ref, bound))
    print(f"{tag}: parameters after the step: {n_clear} of {n_all} elements clear, worst clear error / bound = {worst_clear:.3f}")
    assert n_all - n_clear < 0.05 * n_all
    for i, got, ref, bound in checks:
        assert_within(got, ref, bound, f"parameter {i} after the step")
