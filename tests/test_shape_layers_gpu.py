"""GPU: nn.AvgPool2d, nn.ZeroPad2d, nn.Flatten and the LeNet-5 example (ABI 225).

AvgPool2d: every row of tests/avgpool_ref.py's case table through the C ABI (csrc/avgpool.hip: the general, tiles and global tiers,
and every row again with the general tier forced) and through the module, forward and backward, inside
    |y - y64| <= (n + 2) u sum|taps| / n,      |dx - dx64| <= (m + 2) u sum|dY_j| / n,      uncovered elements exactly +0.0
(u = 2^-24, n = kh kw, m = covering windows; derived in avgpool_ref's docstring, not fitted).  Reruns are bit-identical, a NaN poisons
exactly the windows that hold it, base pointers one float into their buffers stay inside the bounds and inside their fences, every
refusal leaves a sentinel-filled output untouched.  Each test prints its largest error / bound ratio before it asserts (-s).
ZeroPad2d is bit-equal to np.pad and its backward to the crop, -0.0 and NaN included.  Flatten is bit-equal to the reference's
fixtures, keeps a pending BatchNorm2d output pending, and leaves the conv classifier's step bit-identical when it replaces the
model's reshape.  LeNet-5: the reference's recorded training step (tests/golden/lenet5_*.npz) through examples/lenet5.py at the bounds
of test_convtranspose_gpu.test_ddpm_unet_step_vs_reference, and hipGraph replays equal to eager steps bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

import avgpool_ref as AR
from test_hip_parity import assert_close_scaled, assert_within, grad_list_scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN = float("nan")
SENTINEL = -77.25
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
FLAT = [("default", ()), ("d0_1", (0, 1)), ("dm2", (-2,)), ("d0_m1", (0, -1))]


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


@pytest.fixture(scope="module")
def fx(golden):
    return golden("shape_layers")


@pytest.fixture(scope="module")
def table():
    """Inputs of every row, drawn once and left unchanged: X and dY."""
    rng = np.random.default_rng(2250)
    out = {}
    for case in AR.CASES:
        g = AR.geometry(*case[:4])
        out[AR.case_id(case)] = (g, rng.standard_normal(case[0]).astype(np.float32),
                                 rng.standard_normal((g["B"], g["C"], g["Ho"], g["Wo"])).astype(np.float32))
    return out


def call(name, *args):
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    return call_hip_function(name, *args, get_current_stream_ptr())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def make_desc(g, dh=1, dw=1):
    from neunet_hip._lib import Pool2dDesc
    return Pool2dDesc(*[g[k] for k in "B C H W kh kw sh sw pu pd pl pr".split()], dh, dw)


def out_shape(g):
    return (g["B"], g["C"], g["Ho"], g["Wo"])


def in_shape(g):
    return (g["B"], g["C"], g["H"], g["W"])


def abi_forward(X, g):
    out = torch.full(out_shape(g), NAN, device="cuda")
    call("nnhipAvgPool2dForward", out, X, ctypes.byref(make_desc(g)))
    return out


def abi_backward(dY, g):
    dx = torch.full(in_shape(g), NAN, device="cuda")
    call("nnhipAvgPool2dBackward", dx, dY, ctypes.byref(make_desc(g)))
    return dx


class general_route:
    def __enter__(self):
        from neunet_hip._lib import load_hip_function
        self.prev = load_hip_function("nnhipSetAvgPool2dRoute")(1)

    def __exit__(self, *exc):
        from neunet_hip._lib import load_hip_function
        load_hip_function("nnhipSetAvgPool2dRoute")(self.prev)


# ===================================================================================================== AvgPool2d
@pytest.mark.parametrize("case", AR.CASES, ids=AR.case_id)
def test_avgpool_abi_every_row(hip, table, case):
    """Both directions on the tier the descriptor selects and on the forced general tier, into NaN-filled outputs; a second run
    gives the same bits."""
    from neunet_hip._lib import load_hip_function
    g, X, dY = table[AR.case_id(case)]
    assert load_hip_function("nnhipAvgPool2dTier")(ctypes.byref(make_desc(g))) == AR.TIER_IDS[AR.route(g)]
    Xd, dYd = dev(X), dev(dY)
    y, dx = host(abi_forward(Xd, g)), host(abi_backward(dYd, g))
    rf, rb = AR.check_forward(y, X, g, "auto"), AR.check_backward(dx, dY, g, "auto")
    np.testing.assert_array_equal(bits(host(abi_forward(Xd, g))), bits(y))
    np.testing.assert_array_equal(bits(host(abi_backward(dYd, g))), bits(dx))
    with general_route():
        assert load_hip_function("nnhipAvgPool2dTier")(ctypes.byref(make_desc(g))) == 0
        yg, dxg = host(abi_forward(Xd, g)), host(abi_backward(dYd, g))
    gf, gb = AR.check_forward(yg, X, g, "general"), AR.check_backward(dxg, dY, g, "general")
    print(f"\n[{AR.case_id(case)} {AR.route(g)}] error / bound: forward {rf:.3f}, backward {rb:.3f}; general tier {gf:.3f}, {gb:.3f}")


@pytest.mark.parametrize("case", AR.CASES, ids=AR.case_id)
def test_avgpool_module_every_row(hip, table, case):
    import neunet_hip.nn as nn
    g, X, dY = table[AR.case_id(case)]
    x = hip.Tensor(X, device="cuda")
    y = nn.AvgPool2d(*case[1:4])(x)
    assert y.op == "avgpool2d" and y.shape == out_shape(g) and y.requires_grad
    y.backward(dev(dY))
    rf, rb = AR.check_forward(host(y.data), X, g, "module"), AR.check_backward(host(x.grad), dY, g, "module")
    print(f"\n[{AR.case_id(case)} module] error / bound: forward {rf:.3f}, backward {rb:.3f}")
    frozen = nn.AvgPool2d(*case[1:4])(hip.Tensor(X, device="cuda", requires_grad=False))
    assert frozen.args is None and not frozen.requires_grad                    # no gradient work for an input that wants none
    np.testing.assert_array_equal(bits(host(frozen.data)), bits(host(y.data)))


@pytest.mark.parametrize("case", [c for c in AR.CASES if AR.equal_padding(c)], ids=AR.case_id)
def test_avgpool_against_the_reference_fixture(hip, fx, case):
    """The reference's own inputs: our result and the reference's both sit inside the bound around float64, so they are within two
    bounds of each other."""
    g = AR.geometry(*case[:4])
    tag = "avg/" + AR.case_id(case)
    y, dx = host(abi_forward(dev(fx[f"{tag}/X"]), g)), host(abi_backward(dev(fx[f"{tag}/dY"]), g))
    AR.check_forward(y, fx[f"{tag}/X"], g, tag)
    AR.check_backward(dx, fx[f"{tag}/dY"], g, tag)
    _, a = AR.forward64(fx[f"{tag}/X"], g)
    assert_within(y, fx[f"{tag}/Y"], 2 * AR.forward_bound(a, g), tag + " vs reference Y")
    _, a, m = AR.backward64(fx[f"{tag}/dY"], g)
    assert_within(dx, fx[f"{tag}/dX"], 2 * AR.backward_bound(a, m, g), tag + " vs reference dX")


@pytest.mark.parametrize("case", AR.CASES, ids=AR.case_id)
def test_avgpool_nan_poisons_exactly_its_windows(hip, table, case):
    """One NaN and one +inf in X, one NaN in dY: the NaN (and inf) pattern of the output is the float64 restatement's -- every window
    that holds it, nothing else; uncovered input elements stay +0."""
    g, X, dY = table[AR.case_id(case)]
    rng = np.random.default_rng(len(AR.case_id(case)))
    Xn, dYn = X.copy(), dY.copy()
    at = rng.choice(Xn.size, 2, replace=False)
    Xn.flat[at[0]], Xn.flat[at[1]] = NAN, np.inf
    dYn.flat[rng.integers(dYn.size)] = NAN
    with np.errstate(invalid="ignore"):
        y64, _ = AR.forward64(Xn, g)
        dx64, _, m = AR.backward64(dYn, g)
    y, dx = host(abi_forward(dev(Xn), g)), host(abi_backward(dev(dYn), g))
    np.testing.assert_array_equal(np.isnan(y), np.isnan(y64))
    np.testing.assert_array_equal(np.isposinf(y), np.isposinf(y64))
    np.testing.assert_array_equal(np.isnan(dx), np.isnan(dx64))
    assert not bits(dx)[m == 0].any()                                          # +0.0 bit for bit
    assert np.isnan(y).any() or AR.route(g) == "general"                       # (a NaN in a leftover row or a gap reaches no window)


@pytest.mark.parametrize("case", [c for c in AR.CASES if AR.route(AR.geometry(*c[:4])) == "tiles"], ids=AR.case_id)
def test_avgpool_tiles_with_pointers_one_float_in(hip, table, case):
    """Every tensor starts 4 bytes into its buffer: 4-byte aligned, never 16.  The vector kernels must not be chosen (results inside
    the bounds), and the floats around the outputs keep their values."""
    g, X, dY = table[AR.case_id(case)]

    def off(a=None, n=None, fill=SENTINEL):
        n = a.size if a is not None else n
        buf = torch.full((n + 2,), fill, device="cuda")
        if a is not None:
            buf[1:n + 1] = dev(a).reshape(-1)
        return buf, buf[1:n + 1]

    (_, Xv), (_, dYv) = off(X), off(dY)
    (ybuf, yv), (dxbuf, dxv) = off(n=int(np.prod(out_shape(g)))), off(n=X.size)
    assert Xv.data_ptr() % 16 == 4 and AR.tiles_mode(g, Xv.data_ptr(), yv.data_ptr()) == 0
    d = make_desc(g)
    call("nnhipAvgPool2dForward", yv, Xv, ctypes.byref(d))
    call("nnhipAvgPool2dBackward", dxv, dYv, ctypes.byref(d))
    rf = AR.check_forward(host(yv).reshape(out_shape(g)), X, g, "offset")
    rb = AR.check_backward(host(dxv).reshape(X.shape), dY, g, "offset")
    for buf in (ybuf, dxbuf):
        assert float(buf[0]) == SENTINEL and float(buf[-1]) == SENTINEL
    # aligned and offset runs take different kernels with the same summation order: the same bits
    np.testing.assert_array_equal(bits(host(yv).reshape(out_shape(g))), bits(host(abi_forward(dev(X), g))))
    np.testing.assert_array_equal(bits(host(dxv).reshape(X.shape)), bits(host(abi_backward(dev(dY), g))))
    print(f"\n[{AR.case_id(case)} offset] error / bound: forward {rf:.3f}, backward {rb:.3f}")


def test_avgpool_refusals_touch_nothing(hip):
    from neunet_hip._lib import get_current_stream_ptr, load_hip_function
    EINVAL, EALIGN = -1, -2
    base = AR.geometry((2, 3, 7, 5), 3, 2, 1)
    big = torch.full((2 * 3 * 7 * 5 + 1,), SENTINEL, device="cuda")
    src = torch.zeros(2 * 3 * 7 * 5 + 1, device="cuda")
    bad = [dict(base, **{k: 0}) for k in "B C H W kh kw sh sw".split()] + [dict(base, **{k: -1}) for k in "pu pd pl pr".split()]
    bad += [dict(base, kh=10), dict(base, kw=8)]
    bad += [dict(base, B=1 << 16, C=1 << 15, H=1, W=1, kh=1, kw=1, sh=1, sw=1, pu=0, pd=0, pl=0, pr=0)]
    st = get_current_stream_ptr()
    for name in ("nnhipAvgPool2dForward", "nnhipAvgPool2dBackward"):
        f = load_hip_function(name)
        p, q = big.data_ptr(), src.data_ptr()
        assert f(p, q, None, st) == EINVAL
        assert f(None, q, ctypes.byref(make_desc(base)), st) == EINVAL and f(p, None, ctypes.byref(make_desc(base)), st) == EINVAL
        for g in bad:
            assert f(p, q, ctypes.byref(make_desc(g)), st) == EINVAL, g
        assert f(p, q, ctypes.byref(make_desc(base, 2, 1)), st) == EINVAL and f(p, q, ctypes.byref(make_desc(base, 1, 3)), st) == EINVAL
        assert f(p + 2, q, ctypes.byref(make_desc(base)), st) == EALIGN and f(p, q + 1, ctypes.byref(make_desc(base)), st) == EALIGN
    torch.cuda.synchronize()
    assert bool((big == SENTINEL).all())


def test_avgpool_module_refuses_other_inputs(hip):
    import neunet_hip.nn as nn
    with pytest.raises(ValueError):
        nn.AvgPool2d(2)(hip.Tensor(np.zeros((3, 4, 4), np.float32), device="cuda"))
    with pytest.raises(ValueError):
        nn.AvgPool2d(5)(hip.Tensor(np.zeros((1, 1, 4, 4), np.float32), device="cuda"))
    with pytest.raises(NotImplementedError):
        nn.AvgPool2d(2)(hip.Tensor(np.zeros((1, 1, 4, 4)), dtype=np.int32, device="cuda"))


# ===================================================================================================== ZeroPad2d
PADS = [((2, 3, 4, 4), 1, False), ((1, 2, 3, 5), (1, 2, 3, 0), False), ((3, 4, 4), (1, 2), False), ((2, 2, 3, 3), 0, False),
        ((1, 1, 1, 1), (5, 4, 3, 2), False), ((2, 3, 5, 4), (2, 1), True)]


@pytest.mark.parametrize("shape,padding,transposed", PADS, ids=[f"{s}-{p}-{'t' if t else 'c'}".replace(" ", "") for s, p, t in PADS])
def test_zeropad_is_numpy_pad_and_its_backward_the_crop(hip, shape, padding, transposed):
    import neunet_hip.nn as nn
    rng = np.random.default_rng(sum(shape))
    X = rng.standard_normal(shape).astype(np.float32)
    X.flat[0], X.flat[-1] = -0.0, NAN
    if X.size > 3:
        X.flat[1] = np.inf
    m = nn.ZeroPad2d(padding)
    pu, pd, pl, pr = m.padding
    if transposed:                                   # a non-contiguous device array: the last two axes swapped in place
        xd = dev(X).transpose(-1, -2)
        assert not xd.is_contiguous()
        x = hip.Tensor._wrap(xd, None, None, "cuda", requires_grad=True)
        X = np.ascontiguousarray(np.swapaxes(X, -1, -2))
    else:
        x = hip.Tensor(X, device="cuda")
    want = np.pad(X, ((0, 0),) * (X.ndim - 2) + ((pu, pd), (pl, pr)))
    y = m(x)
    assert y.op == "zeropad2d" and y.shape == want.shape and y.data.is_contiguous()
    np.testing.assert_array_equal(bits(host(y.data)), bits(want))                 # the pad itself is +0.0, -0.0 and NaN travel
    G = rng.standard_normal(want.shape).astype(np.float32)
    G.flat[0] = NAN                                                               # in the padding (or the only element): cropped away
    G[..., pu, pl], G[..., pu, pl + X.shape[-1] - 1] = -0.0, NAN
    y.backward(dev(G))
    crop = G[..., pu:pu + X.shape[-2], pl:pl + X.shape[-1]]
    assert tuple(x.grad.shape) == X.shape
    np.testing.assert_array_equal(bits(host(x.grad)), bits(crop))
    frozen = m(hip.Tensor(X, device="cuda", requires_grad=False))
    assert frozen.args is None and not frozen.requires_grad                        # no tape node
    np.testing.assert_array_equal(bits(host(frozen.data)), bits(want))


def test_zeropad_reference_fixture(hip, fx):
    import neunet_hip.nn as nn
    for tag in ("int", "pair", "four", "three_d"):
        p = tuple(int(v) for v in fx[f"pad/{tag}/padding"])
        y = nn.ZeroPad2d(p)(hip.Tensor(fx[f"pad/{tag}/X"], device="cuda"))
        np.testing.assert_array_equal(bits(host(y.data)), bits(fx[f"pad/{tag}/Y"]), err_msg=tag)


def test_zeropad_refuses_other_inputs(hip):
    import neunet_hip.nn as nn
    for shape in ((4, 4), (1, 1, 1, 4, 4)):
        with pytest.raises(ValueError):
            nn.ZeroPad2d(1)(hip.Tensor(np.zeros(shape, np.float32), device="cuda"))
    with pytest.raises(NotImplementedError):
        nn.ZeroPad2d(1)(hip.Tensor(np.zeros((1, 4, 4)), dtype=np.int32, device="cuda"))


# ===================================================================================================== Flatten
@pytest.mark.parametrize("tag,dims", FLAT, ids=[t for t, _ in FLAT])
def test_flatten_device_is_bit_equal_to_the_reference(hip, fx, tag, dims):
    import neunet_hip.nn as nn
    x = hip.Tensor(fx[f"flat/{tag}/X"], device="cuda")
    y = nn.Flatten(*dims)(x)
    assert y.shape == fx[f"flat/{tag}/Y"].shape and y.op == "reshape"
    np.testing.assert_array_equal(bits(host(y.data)), bits(fx[f"flat/{tag}/Y"]))
    y.backward(dev(fx[f"flat/{tag}/dY"]))
    assert tuple(x.grad.shape) == x.shape
    np.testing.assert_array_equal(bits(host(x.grad)), bits(fx[f"flat/{tag}/dX"]))


@pytest.mark.parametrize("tail_one_launch", [False, True])
def test_flatten_in_the_conv_classifier(hip, monkeypatch, tail_one_launch):
    """examples/conv_classifier.py's model with nn.Flatten() in place of x.reshape(x.shape[0], -1): the same loss and gradients bit
    for bit.  With the one-launch tail on, the BatchNorm2d output is pending, Flatten's result is still pending, and so is the model
    output -- the tail survives the module."""
    sys.path.insert(0, EXAMPLES)
    import conv_classifier
    import neunet_hip.nn as nn
    import neunet_hip.nn.experimental.vision as V
    monkeypatch.setattr(V, "_FUSE_TAIL", tail_one_launch)
    seen = {}

    class WithFlatten(conv_classifier.Conv2dClassifier):
        def __init__(self):
            super().__init__()
            self.flatten = nn.Flatten()

        def forward(self, x):
            x = self.maxpool1(self.leaky_relu(self.conv1(x)))
            x = self.maxpool2(self.leaky_relu(self.conv2(x)))
            x = self.bnorm(x)
            seen["bn"] = getattr(x, "pending", lambda: False)()
            x = self.flatten(x)
            seen["flat"] = getattr(x, "pending", lambda: False)()
            return self.sigmoid(self.fc1(x))

    rng = np.random.default_rng(1005)
    X = rng.uniform(-1, 1, (256, 1, 28, 28)).astype(np.float32)
    Tt = np.eye(10, dtype=np.float32)[rng.integers(0, 10, 256)]
    results = []
    for cls in (conv_classifier.Conv2dClassifier, WithFlatten):
        np.random.seed(1005)
        model = cls()
        out = model(hip.Tensor(X, device="cuda"))
        assert getattr(out, "pending", lambda: False)() == tail_one_launch
        loss = nn.MSELoss()(out, hip.Tensor(Tt, device="cuda", requires_grad=False))
        loss.backward()
        results.append([host(loss.data)] + [host(p.grad) for p in model.parameters()] + [host(out.data)])
    assert seen == {"bn": tail_one_launch, "flat": tail_one_launch}
    assert len(results[0]) == len(results[1])
    for a, b in zip(*results):
        np.testing.assert_array_equal(bits(a), bits(b))


# ===================================================================================================== LeNet-5
def test_lenet5_step_vs_reference(hip, golden):
    """One training step of LeNet-5 as the reference ran it (batch 8), through examples/lenet5.py -- ZeroPad2d, AvgPool2d and Flatten
    in the path, the pad's backward included (the reference could not run it; the input needs no gradient here either).  Bounds as in
    test_ddpm_unet_step_vs_reference, which are those of test_conv_classifier_golden: |loss - ref| < 1e-6, logits at rtol 1e-4 /
    atol 1e-5, every gradient within 1e-4 of max(|ref|, rms(ref), grad_list_scale).  After the Adam step an element is CLEAR when
    |g_ref| > 2 e (e = that gradient bound) and is held to 1e-4 lr + 2 * 2^-24 |p_ref| + lr eps e / (|g_ref| - e)^2; the others get
    2 lr + the rounding term and must be fewer than 5 % of the model (the fixture records its own share: 0.4 %)."""
    sys.path.insert(0, EXAMPLES)
    import lenet5
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    f = golden("lenet5_0")
    assert float(f["unclear_share"]) < 0.01
    model = lenet5.LeNet5()
    params = model.parameters()
    n = int(f["n_params"])
    assert len(params) == n == 10 and sum(p.size for p in params) == 61706
    for i, p in enumerate(params):
        assert p.size == f[f"p{i}"].size, f"parameter {i}: {p.shape} vs {f[f'p{i}'].shape}"
        p.data.copy_(dev(f[f"p{i}"]).reshape(p.shape))
    lr = float(f["lr"])
    opt = Adam(params, lr=lr)
    opt.zero_grad()
    x = hip.Tensor(f["X"], device="cuda", requires_grad=False)
    np.testing.assert_array_equal(bits(host(model.pad(x).data)), bits(f["Xpad"]))
    logits = model(x)
    loss = nn.CrossEntropyLoss()(logits, hip.Tensor(f["Y"], dtype=np.int32, device="cuda", requires_grad=False))
    loss.backward()
    print(f"\nloss {loss.item():.7f} vs {float(f['loss']):.7f}")
    assert abs(loss.item() - float(f["loss"])) < 1e-6
    np.testing.assert_allclose(host(logits.data), f["logits"], rtol=1e-4, atol=1e-5)
    grads = [f[f"g{i}"] for i in range(n)]
    gscale = grad_list_scale(grads)
    worst = 0.0
    for i, p in enumerate(params):
        ref = grads[i].reshape(p.shape).astype(np.float64)
        got = host(p.grad).reshape(p.shape)
        worst = max(worst, float(np.max(np.abs(got - ref) / (1e-4 * np.maximum(np.maximum(np.abs(ref), np.sqrt(np.mean(ref ** 2))), gscale)))))
    print(f"worst gradient error / bound = {worst:.3f}")
    for i, p in enumerate(params):
        assert_close_scaled(host(p.grad).reshape(p.shape), grads[i].reshape(p.shape), err_msg=f"grad {i} {p.shape}", scale=gscale)
    opt.step()
    eps, n_clear, n_all, worst_clear = 1e-8, 0, 0, 0.0
    checks = []
    for i, p in enumerate(params):
        g = grads[i].reshape(p.shape).astype(np.float64)
        ref = f[f"p_after{i}"].reshape(p.shape).astype(np.float64)
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
    print(f"parameters after the step: {n_clear} of {n_all} elements clear, worst clear error / bound = {worst_clear:.3f}")
    assert n_all - n_clear < 0.05 * n_all
    assert abs((n_all - n_clear) / n_all - float(f["unclear_share"])) < 1e-12
    for i, got, ref, bound in checks:
        assert_within(got, ref, bound, f"parameter {i} after the step")


def test_graphed_lenet5_equals_eager(hip):
    """Two warm-up steps and three replays of the captured LeNet-5 step (the slice pair of ZeroPad2d and both AvgPool2d directions
    inside the hipGraph) leave exactly the parameters of five eager steps."""
    sys.path.insert(0, EXAMPLES)
    import lenet5
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    B = 32
    rng = np.random.default_rng(225)
    data = [(rng.uniform(-1, 1, (B, 1, 28, 28)).astype(np.float32), rng.integers(0, 10, B).astype(np.int32)) for _ in range(5)]

    def make():
        np.random.seed(44)
        model = lenet5.LeNet5()
        xs = hip.Tensor(data[0][0], device="cuda", requires_grad=False)
        ys = hip.Tensor(data[0][1], dtype=np.int32, device="cuda", requires_grad=False)
        loss_fn = nn.CrossEntropyLoss()

        def fb():
            loss = loss_fn(model(xs), ys)
            loss.backward()
            return loss

        return model, xs, ys, fb, Adam(model.parameters(), lr=1e-3)

    def feed(xs, ys, item):
        xs.data.copy_(dev(item[0]))
        ys.data.copy_(dev(item[1], np.int32))

    m0, xs0, ys0, fb0, opt0 = make()
    for item in data:
        feed(xs0, ys0, item)
        opt0.zero_grad()
        fb0()
        opt0.step()
    want = [host(p.data) for p in m0.parameters()]
    m, xs, ys, fb, opt = make()
    warm = iter(data[:2])

    def fb_warm():
        item = next(warm, None)
        if item is not None:
            feed(xs, ys, item)
        return fb()

    g = GraphedTrainStep(fb_warm, opt, GradBucket(m.parameters()), warmup=2)
    for item in data[2:]:
        feed(xs, ys, item)
        g()
    got = [host(p.data) for p in m.parameters()]
    g.release()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(bits(a), bits(b))
