"""GPU: ConvTranspose2d through the C ABI (include/neunet_hip.h) on both stride > 1 routes -- the stride-phase kernel of
csrc/conv_transpose.hip and the Conv2d input-gradient gather -- and through nn.ConvTranspose2d, against the reference's recorded
outputs (tests/golden/convt_*.npz) and the float64 restatement of tests/convtranspose_ref.py; the U-Net glue; and one training
step of the reference's DDPM U-Net (tests/golden/ddpm_unet.npz) through examples/ddpm_unet.py.

Bounds.  O, dX, dW, db: the project's 1e-4 of max(|ref|, rms(ref)) per element against float64 (assert_close_scaled) and
rtol = atol = 1e-4 (test_hip_parity.TOL) against the float32 fixture.  At the tile-edge shapes O is also held to the dot-product
bound 32 * 2^-24 * sum|x||w| + 4 * 2^-24 * |ref| (assert_dot_close's, with the sum taken through the restatement on |X|, |W|),
and the two routes to twice that of each other.  Each test prints its largest error / bound ratio before it asserts (-s)."""
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
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).cuda()


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
