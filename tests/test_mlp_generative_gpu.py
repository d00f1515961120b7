"""GPU: the small kernels behind the MLP generative examples (Tanh, BCELoss in both gradient forms, the Gaussian reparameterisation
and KL term) through the C ABI against the float64 restatements of tests/bn1d_ref.py; the modules (nn.BatchNorm1d, nn.Tanh,
nn.BCELoss, neunet_hip.reparameterize / gaussian_kld) against the reference's fixtures; and one whole training step of
examples/gan.py and examples/vae.py against the step the reference ran (tests/golden/gan_tiny.npz, vae_tiny.npz).

Bounds.  Tanh forward: 4 x 2^-24 relative (tanhf at 2 ulp, one to spare either side) plus one float32 underflow; backward: its three
operations (bn1d_ref.tanh_backward_bound).  BCE / KLD losses: the derived sum bounds (bn1d_ref.bce_loss_bound, kld_bound); gradients:
the project's 1e-4 of max(|ref|, rms(ref)).  Whole steps: the bounds of test_convtranspose_gpu.test_ddpm_unet_step_vs_reference.
Each test prints its largest error / bound ratio before it asserts (run with -s)."""
import os
import sys

import numpy as np
import pytest

from bn1d_ref import (bce, bce_loss_bound, bce_term_bound, kld, kld_bound, reparam, reparam_bound, tanh_backward, tanh_backward_bound,
                      tanh_forward)
from test_hip_parity import assert_close_scaled, assert_within, grad_list_scale, rms_of
from vision_ref import FLT_MIN, U24

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
NAN = float("nan")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


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


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda", dtype=torch.float32)


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(np.max(err / np.maximum(np.broadcast_to(bound, err.shape), 1e-300))) if err.size else 0.0


def scaled_bound(ref, tol=1e-4, scale=0.0):
    ref = np.asarray(ref, np.float64)
    return tol * np.maximum(np.maximum(np.abs(ref), rms_of(ref)), scale) + 1e-30


# ===================================================================================================== Tanh
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_tanh_sizes(hip, golden, n, misaligned):
    """float4 body, scalar tail and the all-scalar path (operands one float into their buffers); the fixture's special values (+-0,
    +-1e-30, +-9.5 where float32 tanh is 1 - 2^-24 ... 1, +-20 where it is exactly 1) lead the input.  Nothing past the end is written."""
    rng = np.random.default_rng(n)
    X = np.concatenate([golden("tanh")["X"].reshape(-1)[-8:], rng.standard_normal(max(n - 8, 0)) * 3]).astype(np.float32)[:n]
    dY = rng.standard_normal(n).astype(np.float32)
    o = 1 if misaligned else 0
    xb, yb, gb, db = nans(n + 2), nans(n + 2), nans(n + 2), nans(n + 2)
    x, y, g, dx = (t[o:o + n] for t in (xb, yb, gb, db))
    x.copy_(dev(X))
    g.copy_(dev(dY))
    assert x.data_ptr() % 16 == (4 if misaligned else 0)
    call("nnhipTanhForward", y, x, n)
    call("nnhipTanhBackward", dx, g, y, n)
    for t in (yb, db):
        assert bool(torch.isnan(t[o + n])) and (not misaligned or bool(torch.isnan(t[0]))), "wrote outside the output"
    Yr = tanh_forward(X)
    f = host(y)
    dXr = tanh_backward(f, dY)                                  # at the kernel's own saved output, as the backward reads it
    rf, rb = ratio(f, Yr, 4 * U24 * np.abs(Yr) + FLT_MIN), ratio(host(dx), dXr, tanh_backward_bound(f, dY))
    print(f"\n[tanh n = {n}] forward {rf:.3f} of 4 x 2^-24, backward {rb:.3f} of its three roundings")
    assert_within(f, Yr, 4 * U24 * np.abs(Yr) + FLT_MIN, "tanh forward")
    assert_within(host(dx), dXr, tanh_backward_bound(f, dY), "tanh backward")
    assert np.all(np.abs(f) <= 1.0)


def test_tanh_module_matches_reference_fixture(hip, golden):
    from neunet_hip import Tensor
    g = golden("tanh")
    x = Tensor(g["X"], device="cuda")
    y = hip.nn.Tanh()(x)
    y.backward(dev(g["dY"]))
    np.testing.assert_allclose(host(y.data), g["Y"], rtol=1e-6, atol=1e-37)
    # dX = dY (1 - f^2) cancels where |f| -> 1 (the fixture has such entries): against float64 at the kernel's own f within the
    # three roundings; against the reference's float32 dX within both sides' roundings plus what the two f's may differ by
    # (tanhf at 2 ulp on either side: |d(1 - f^2)| = 2 |f| |df| <= 8 x 2^-24 f^2)
    f, dY = host(y.data), g["dY"]
    assert_within(host(x.grad), tanh_backward(f, dY), tanh_backward_bound(f, dY), "dX at the kernel's own output")
    assert_within(host(x.grad), g["dX"], 2 * tanh_backward_bound(f, dY) + 8 * U24 * np.abs(dY) * f.astype(np.float64) ** 2, "dX vs the reference")


# ===================================================================================================== BCELoss
def run_bce(P, Y, W, reduction, fold, scalar_w=1.0):
    n = P.size
    loss = nans(n + 1) if reduction == "none" else nans(2)
    dp = nans(n + 1)
    call("nnhipBCELossForwardBackward", dev(P), dev(Y), None if W is None else dev(W), float(scalar_w), loss, dp, n,
         {"mean": b"m", "sum": b"s", "none": b"n"}[reduction], int(fold))
    lh, gh = host(loss), host(dp)
    assert np.isnan(gh[n]) and np.isnan(lh[n if reduction == "none" else 1])           # nothing past the end
    return (lh[:n].reshape(P.shape) if reduction == "none" else float(lh[0])), gh[:n].reshape(P.shape)


@pytest.mark.parametrize("fold", [False, True], ids=["dp", "dz"])
@pytest.mark.parametrize("tag,reduction", [("mean", "mean"), ("sum", "sum"), ("none", "none"), ("weighted", "mean")])
def test_bce_fixtures(hip, golden, tag, reduction, fold):
    """The four reference fixtures, both gradient forms: d loss / d pred, and d loss / d z with pred = sigmoid(z) folded in."""
    g = golden(f"bce_{tag}")
    P, Y, W = g["P"], g["Y"], (g["W"] if tag == "weighted" else None)
    loss, grad = run_bce(P, Y, W, reduction, fold)
    ref_loss, dp, dz = bce(P, Y, W, reduction)
    ref_g = dz if fold else dp
    if reduction == "none":
        bound = bce_term_bound(P, Y, W)
        print(f"\n[bce {tag}] terms {ratio(loss, ref_loss, bound):.3f} of the term bound, gradient {ratio(grad, ref_g, scaled_bound(ref_g)):.3f}")
        assert_within(loss, ref_loss, bound, "terms")
    else:
        bound = bce_loss_bound(P, Y, W, reduction)
        print(f"\n[bce {tag}] |loss - float64| / bound = {abs(loss - ref_loss) / bound:.3f}, gradient {ratio(grad, ref_g, scaled_bound(ref_g)):.3f}")
        assert abs(loss - ref_loss) <= bound, (loss, ref_loss, bound)
        np.testing.assert_allclose(loss, float(g["loss"]), rtol=1e-5)                     # and the reference's own float32 value
    assert_close_scaled(grad, ref_g, err_msg="gradient")
    if not fold:
        np.testing.assert_allclose(grad, g["dP"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("n,reduction", [(16384, "mean"), (16385, "sum"), (78400, "sum"), (20000, "none")])
def test_bce_sizes(hip, n, reduction):
    """Either side of the one-block limit, the notebook VAE's 100 x 784 through the two-launch path, and a scalar weight."""
    rng = np.random.default_rng(n)
    P, Y = rng.uniform(1e-4, 1 - 1e-4, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    loss, grad = run_bce(P, Y, None, reduction, False, scalar_w=1.5)
    ref_loss, dp, _ = bce(P, Y, np.float64(1.5), reduction)
    if reduction == "none":
        assert_within(loss, ref_loss, bce_term_bound(P, Y, 1.5), "terms")
    else:
        bound = bce_loss_bound(P, Y, 1.5, reduction)
        print(f"\n[bce n = {n}] |loss - float64| / bound = {abs(loss - ref_loss) / bound:.3f}")
        assert abs(loss - ref_loss) <= bound, (loss, ref_loss, bound)
    assert_close_scaled(grad, dp, err_msg="gradient")


def test_bce_folded_gradient_at_a_saturated_prediction(hip):
    """p = 1.0 exactly with y = 0 (a saturated Sigmoid): the literal loss is +inf and the unfolded gradient (1 - y) / (1 - p) divides by
    zero, but the folded gradient is (p - y) w scale = w scale -- finite, exactly.  p = 0 with y = 1 likewise gives -w scale."""
    P = np.array([1.0, 0.0, 0.5, 0.25], np.float32)
    Y = np.array([0.0, 1.0, 0.5, 1.0], np.float32)
    for reduction, scale in (("mean", 0.25), ("sum", 1.0), ("none", 1.0)):
        loss, grad = run_bce(P, Y, None, reduction, True, scalar_w=2.0)
        assert np.all(np.isfinite(grad))
        np.testing.assert_array_equal(grad, np.array([1.0, -1.0, 0.0, -0.75], np.float32) * np.float32(2.0 * scale))
        assert np.isinf(loss) if reduction != "none" else (np.isinf(loss[0]) and np.isinf(loss[1]) and np.isfinite(loss[2:]).all())
        _, plain = run_bce(P, Y, None, reduction, False, scalar_w=2.0)
        assert not np.isfinite(plain[0])                       # what the fold avoids


def test_bce_module_and_sigmoid_fold(hip, golden):
    """nn.BCELoss on a Sigmoid's output: the folded gradient lands in the Sigmoid's input and equals the unfolded chain; the weighted
    fixture through the module; the reduced loss is a 0-d tensor whose backward() needs no seed."""
    from neunet_hip import Tensor
    g = golden("bce_weighted")
    p = Tensor(g["P"], device="cuda")
    loss = hip.nn.BCELoss(weight=g["W"], reduction="mean")(p, Tensor(g["Y"], device="cuda", requires_grad=False))
    assert loss.shape == () and getattr(loss, "_implicit_seed", False)
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(g["loss"]), rtol=1e-5)
    np.testing.assert_allclose(host(p.grad), g["dP"], rtol=1e-4, atol=1e-6)
    rng = np.random.default_rng(4)
    Z, Y = rng.standard_normal((6, 11)).astype(np.float32) * 2, rng.uniform(0, 1, (6, 11)).astype(np.float32)
    z = Tensor(Z, device="cuda")
    s = hip.nn.Sigmoid()(z)
    loss = hip.nn.BCELoss(reduction="sum")(s, Tensor(Y, device="cuda", requires_grad=False))
    loss.backward()
    pz = 1 / (1 + np.exp(-Z.astype(np.float64)))
    ref_loss, _, dz = bce(pz, Y, None, "sum")
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-5)
    assert_close_scaled(host(z.grad), dz, err_msg="folded gradient at the Sigmoid's input")
    none = hip.nn.BCELoss(reduction="none")(Tensor(g["P"], device="cuda"), Tensor(g["Y"], device="cuda", requires_grad=False))
    assert none.shape == g["P"].shape


# ===================================================================================================== reparameterise, KLD
@pytest.mark.parametrize("n", [24, 20000])
def test_reparam_and_kld_vs_float64(hip, n):
    rng = np.random.default_rng(n)
    mu, lv, eps, g = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    z, sd, dmu, dlv = nans(n + 1), nans(n + 1), nans(n + 1), nans(n + 1)
    call("nnhipGaussianReparamForward", dev(mu), dev(lv), dev(eps), z[:n], sd[:n], n)
    call("nnhipGaussianReparamBackward", dev(g), dev(eps), sd[:n], dmu[:n], dlv[:n], n)
    zr, dmur, dlvr = reparam(mu, lv, eps, g)
    for t in (z, sd, dmu, dlv):
        assert bool(torch.isnan(t[n]))
    print(f"\n[reparam n = {n}] z {ratio(host(z)[:n], zr, reparam_bound(mu, lv, eps)):.3f} of its bound")
    assert_within(host(z)[:n], zr, reparam_bound(mu, lv, eps), "z")
    np.testing.assert_array_equal(host(dmu)[:n], g)                                         # dmu = g, a copy
    assert_within(host(dlv)[:n], dlvr, 6 * U24 * np.abs(dlvr) + FLT_MIN, "dlogvar")         # expf at 2 ulp, 0.5 x exact, three products, one to spare
    loss, kmu, klv = nans(2), nans(n + 1), nans(n + 1)
    call("nnhipGaussianKLDForwardBackward", dev(mu), dev(lv), loss, kmu[:n], klv[:n], n)
    kr, kmur, klvr = kld(mu, lv)
    print(f"[kld n = {n}] |KLD - float64| / bound = {abs(float(host(loss)[0]) - kr) / kld_bound(mu, lv):.3f}")
    assert abs(float(host(loss)[0]) - kr) <= kld_bound(mu, lv) and np.isnan(host(loss)[1])
    np.testing.assert_array_equal(host(kmu)[:n], mu)
    e = np.exp(lv.astype(np.float64))
    assert_within(host(klv)[:n], klvr, U24 * (2 * e + np.abs(e - 1)) + FLT_MIN, "dKLD/dlogvar")   # expf at 2 ulp, the subtraction; 0.5 x exact
    call("nnhipGaussianKLDForwardBackward", dev(mu), dev(lv), loss, None, None, n)           # value only
    assert abs(float(host(loss)[0]) - kr) <= kld_bound(mu, lv)


def test_latent_ops_on_the_tape(hip, golden):
    """neunet_hip.reparameterize / gaussian_kld as tape nodes: KLD + a consumer of z, gradients accumulate in mu and logvar."""
    from neunet_hip import Tensor
    f = golden("vae_tiny")
    mu, lv = Tensor(f["mu"], device="cuda"), Tensor(f["logvar"], device="cuda")
    z = hip.reparameterize(mu, lv, Tensor(f["eps"], device="cuda", requires_grad=False))
    np.testing.assert_allclose(host(z.data), f["z"], rtol=1e-5, atol=1e-6)
    k = hip.gaussian_kld(mu, lv)
    assert k.shape == ()
    G = np.random.default_rng(6).standard_normal(f["mu"].shape).astype(np.float32)
    z.backward(dev(G))
    k.backward()
    _, dmu, dlv = reparam(f["mu"], f["logvar"], f["eps"], G)
    kr, kmu, klv = kld(f["mu"], f["logvar"])
    np.testing.assert_allclose(k.item(), kr, rtol=1e-5)
    assert_close_scaled(host(mu.grad), dmu + kmu, err_msg="dmu")
    assert_close_scaled(host(lv.grad), dlv + klv, err_msg="dlogvar")


# ===================================================================================================== nn.BatchNorm1d
@pytest.mark.parametrize("tag", ["affine", "plain"])
def test_batchnorm1d_module_matches_reference_fixture(hip, golden, tag):
    """The reference layer's two training steps, eval and the backward after each, through nn.BatchNorm1d; the second backward runs
    without a zero_grad, so weight.grad / bias.grad ACCUMULATE (the GAN's discriminator-side pattern)."""
    from neunet_hip import Tensor
    g = golden(f"bn1d_{tag}")
    F = g["X1"].shape[1]
    m = hip.nn.BatchNorm1d(F, eps=float(g["eps"]), momentum=float(g["momentum"]), affine=tag == "affine")
    if tag == "affine":
        m.weight.data.copy_(dev(g["w"]))
        m.bias.data.copy_(dev(g["b"]))
    x1 = Tensor(g["X1"], device="cuda")
    y1 = m(x1)
    np.testing.assert_allclose(host(y1.data), g["Y1"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(m.running_mean.data), g["running_mean1"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(m.running_var.data), g["running_var1"], rtol=1e-5, atol=1e-6)
    y1.backward(dev(g["dY"]))
    assert_close_scaled(host(x1.grad), g["dX1"], err_msg="dX1")
    if tag == "affine":
        assert tuple(m.weight.grad.shape) == (1, F)
        assert_close_scaled(host(m.weight.grad), g["dW1"], err_msg="dW1")
        assert_close_scaled(host(m.bias.grad), g["db1"], err_msg="db1")
    y2 = m(Tensor(g["X2"], device="cuda"))
    np.testing.assert_allclose(host(y2.data), g["Y2"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(m.running_mean.data), g["running_mean2"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(host(m.running_var.data), g["running_var2"], rtol=1e-5, atol=1e-6)
    m.eval()
    xe = Tensor(g["X1"], device="cuda")
    ye = m(xe)
    np.testing.assert_allclose(host(ye.data), g["Y_eval"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(m.running_mean.data), g["running_mean2"], rtol=1e-5, atol=1e-6)     # eval leaves them alone
    ye.backward(dev(g["dY"]))
    assert_close_scaled(host(xe.grad), g["dX_eval"], err_msg="dX_eval")
    if tag == "affine":                                                                     # no zero_grad in between: the two add up
        assert_close_scaled(host(m.weight.grad), g["dW1"].astype(np.float64) + g["dW_eval"], err_msg="dW accumulated")
        assert_close_scaled(host(m.bias.grad), g["db1"].astype(np.float64) + g["db_eval"], err_msg="db accumulated")
        assert list(m.state_dict()) == ["running_mean", "running_var", "weight", "bias"]
    with pytest.raises(ValueError, match="2-D"):
        m(Tensor(np.zeros((4, F, 3), np.float32), device="cuda"))


# ===================================================================================================== whole steps
LR_EPS = 1e-8


def check_grads(tag, params, refs, gscale):
    worst = 0.0
    for p, r in zip(params, refs):
        ref = r.reshape(p.shape).astype(np.float64)
        worst = max(worst, ratio(host(p.grad).reshape(p.shape), ref, scaled_bound(ref, scale=gscale)))
    print(f"{tag}: worst gradient error / bound = {worst:.3f}")
    for i, (p, r) in enumerate(zip(params, refs)):
        assert_close_scaled(host(p.grad).reshape(p.shape), r.reshape(p.shape), err_msg=f"{tag} grad {i} {p.shape}", scale=gscale)


def check_first_adam_step(tag, params, grads, after, lr, gscale):
    """The parameter bounds of test_ddpm_unet_step_vs_reference (first Adam step from zero moments: p - lr g / (|g| + eps)):
    1e-4 lr + 2 x 2^-24 |p| + lr eps e / (|g| - e)^2 where the gradient's sign is clear (|g| > 2 e, e the gradient bound), 2 lr + rounding
    elsewhere, and fewer than 5 % of the elements unclear."""
    n_clear, n_all, worst, checks = 0, 0, 0.0, []
    for i, p in enumerate(params):
        g = grads[i].reshape(p.shape).astype(np.float64)
        ref = after[i].reshape(p.shape).astype(np.float64)
        e = 1e-4 * np.maximum(np.maximum(np.abs(g), np.sqrt(np.mean(g ** 2))), gscale)
        clear = np.abs(g) > 2 * e
        rounding = 2 * 2.0 ** -24 * np.abs(ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            tight = 1e-4 * lr + rounding + lr * LR_EPS * e / (np.abs(g) - e) ** 2
        bound = np.where(clear, tight, 2 * lr + rounding)
        got = host(p.data).astype(np.float64)
        n_clear, n_all = n_clear + int(clear.sum()), n_all + clear.size
        if clear.any():
            worst = max(worst, float(np.max((np.abs(got - ref) / bound)[clear])))
        checks.append((i, got, ref, bound))
    print(f"{tag}: parameters after the step: {n_clear} of {n_all} elements clear, worst clear error / bound = {worst:.3f}")
    assert n_all - n_clear < 0.05 * n_all
    for i, got, ref, bound in checks:
        assert_within(got, ref, bound, f"{tag} parameter {i} after the step")


def load_params(params, f, prefix):
    for i, p in enumerate(params):
        assert p.size == f[f"{prefix}{i}"].size, f"parameter {i}: {p.shape} vs {f[f'{prefix}{i}'].shape}"
        p.data.copy_(dev(f[f"{prefix}{i}"]).reshape(p.shape))


def test_vae_step_vs_reference(hip, golden):
    """One training step of the notebook's VAE class as the reference ran it (64 pixels, hidden 48 / 32, latent 2, batch 12, the drawn
    eps injected), through examples/vae.py.  Bounds of test_ddpm_unet_step_vs_reference, with one difference that the loss forces: that
    test holds an O(1) MEAN loss to 1e-6 absolute; this loss is a SUM over 768 pixels (plus the KL term) near 500, where one float32
    spacing is 3e-5 -- it is held to the same 1e-6 RELATIVE to its size."""
    import vae as vae_example
    from neunet_hip import Tensor
    from neunet_hip.optim import Adam
    f = golden("vae_tiny")
    cfg = [int(v) for v in f["cfg"]]
    model = vae_example.VAE(cfg[0], cfg[3], (cfg[1], cfg[2])).to("cuda")
    params = model.parameters()
    n = int(f["n_params"])
    assert len(params) == n
    load_params(params, f, "p")
    lr = 0.0005
    opt = Adam(params, lr=lr)
    model.train()
    x = Tensor(f["x"], device="cuda", requires_grad=False)
    eps = Tensor(f["eps"], device="cuda", requires_grad=False)
    x_recon, mu, logvar = model.forward(x, eps)
    loss = model.loss_function(x, x_recon, mu, logvar)
    opt.zero_grad()
    loss.backward()
    ref_loss = float(f["loss"])
    print(f"\nvae: loss {loss.item():.5f} vs {ref_loss:.5f}: |difference| / (1e-6 |loss|) = {abs(loss.item() - ref_loss) / (1e-6 * abs(ref_loss)):.3f}")
    assert loss.shape == ()
    assert abs(loss.item() - ref_loss) < 1e-6 * abs(ref_loss)
    np.testing.assert_allclose(host(x_recon.data), f["x_recon"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(mu.data), f["mu"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(logvar.data), f["logvar"], rtol=1e-4, atol=1e-5)
    grads = [f[f"g{i}"] for i in range(n)]
    gscale = grad_list_scale(grads)
    check_grads("vae", params, grads, gscale)
    opt.step()
    check_first_adam_step("vae", params, grads, [f[f"p_after{i}"] for i in range(n)], lr, gscale)


def adam_two_steps(g1, g2, lr, b1=0.5, b2=0.999, eps=LR_EPS):
    """(update of step 1, update of step 2) of Adam from zero moments in float64 (the reference's optim.py: bias-corrected moments,
    lr m_hat / (sqrt(v_hat) + eps))."""
    m1, v1 = (1 - b1) * g1, (1 - b2) * g1 ** 2
    u1 = lr * (m1 / (1 - b1)) / (np.sqrt(v1 / (1 - b2)) + eps)
    m2, v2 = b1 * m1 + (1 - b1) * g2, b2 * v1 + (1 - b2) * g2 ** 2
    u2 = lr * (m2 / (1 - b1 ** 2)) / (np.sqrt(v2 / (1 - b2 ** 2)) + eps)
    return u1, u2


def test_gan_step_vs_reference(hip, golden):
    """One three-phase step of the notebook's GAN as the reference ran it (noise 16, hidden 32 / 48, 64 pixels, batch 12; the drawn noise
    and both dropout masks injected), through examples/gan.py: phase 1 (real -> d.step), phase 2 (fake -> d.step with the
    discriminator's gradients ACCUMULATED over phases 1 and 2 -- checked explicitly against the fixture's accumulated gradients -- and
    the gradient flowing on into the generator), phase 3 (g.zero_grad, fake -> g.step).  Bounds of test_ddpm_unet_step_vs_reference:
    losses to 1e-6, predictions at rtol 1e-4 / atol 1e-5, gradients at 1e-4 scaled, parameters after a FIRST Adam step by that test's
    rule.  The discriminator's SECOND step starts from non-zero moments, where that rule's closed form does not apply: its update is
    held to 1e-4 lr + rounding + twice the largest change of the float64 update over the four corners (g1 +- e1, g2 +- e2) of the two
    gradient bounds (first-order sensitivity, doubled), on top of the first step's own bound."""
    import gan as gan_example
    from neunet_hip import Tensor
    from neunet_hip.optim import Adam
    f = golden("gan_tiny")
    noise, g1h, g2h, pixels, d1h, d2h, B = [int(v) for v in f["cfg"]]
    cfg = dict(noise=noise, g_hidden=(g1h, g2h), pixels=pixels, d_hidden=(d1h, d2h), batch=B)
    generator, discriminator = gan_example.make_generator(**cfg), gan_example.make_discriminator(**cfg)
    gp, dp = generator.parameters(), discriminator.parameters()
    ng, nd = int(f["n_g"]), int(f["n_d"])
    assert (len(gp), len(dp)) == (ng, nd)
    load_params(gp, f, "g_p")
    load_params(dp, f, "d_p")
    lr = 0.001
    g_opt, d_opt = Adam(gp, lr=lr, betas=(0.5, 0.999)), Adam(dp, lr=lr, betas=(0.5, 0.999))
    loss_fn = hip.nn.MSELoss()
    generator.train()
    discriminator.train()
    T = lambda a: Tensor(a, device="cuda", requires_grad=False)      # noqa: E731
    ones, zeros = T(np.ones((B, 1), np.float32)), T(np.zeros((B, 1), np.float32))
    # ---- phase 1
    d_opt.zero_grad()
    real_pred = discriminator(T(f["real"]))
    real_loss = loss_fn(real_pred, ones)
    real_loss.backward()
    print(f"\ngan: real loss {real_loss.item():.7f} vs {float(f['real_loss']):.7f}")
    assert abs(real_loss.item() - float(f["real_loss"])) < 1e-6
    np.testing.assert_allclose(host(real_pred.data), f["real_pred"], rtol=1e-4, atol=1e-5)
    d_g1 = [f[f"d_g_real{i}"] for i in range(nd)]
    ds1 = grad_list_scale(d_g1)
    check_grads("gan phase 1 (D)", dp, d_g1, ds1)
    d_opt.step()
    check_first_adam_step("gan phase 1 (D)", dp, d_g1, [f[f"d_p_real{i}"] for i in range(nd)], lr, ds1)
    # ---- phase 2: no zero_grad
    fake_pred = discriminator(gan_example.run_generator(generator, T(f["noise_d"]), dev(f["mask_d"])))
    fake_loss = loss_fn(fake_pred, zeros)
    fake_loss.backward()
    assert abs(fake_loss.item() - float(f["fake_loss"])) < 1e-6
    np.testing.assert_allclose(host(fake_pred.data), f["fake_pred"], rtol=1e-4, atol=1e-5)
    d_g2 = [f[f"d_g_acc{i}"] for i in range(nd)]
    ds2 = grad_list_scale(d_g2)
    check_grads("gan phase 2 (D, accumulated over phases 1 and 2)", dp, d_g2, ds2)
    assert all(p.grad is not None for p in gp)                  # the gradient flowed on into the generator
    d_opt.step()
    worst = 0.0
    for i, p in enumerate(dp):
        a, b = d_g1[i].reshape(p.shape).astype(np.float64), d_g2[i].reshape(p.shape).astype(np.float64)
        e1 = 1e-4 * np.maximum(np.maximum(np.abs(a), rms_of(a)), ds1)
        e2 = 1e-4 * np.maximum(np.maximum(np.abs(b), rms_of(b)), ds2)
        u2 = adam_two_steps(a, b, lr)[1]
        sens = np.max([np.abs(adam_two_steps(a + s1 * e1, b + s2 * e2, lr)[1] - u2) for s1 in (-1, 1) for s2 in (-1, 1)], axis=0)
        ref1 = f[f"d_p_real{i}"].reshape(p.shape).astype(np.float64)
        ref = f[f"d_p_after{i}"].reshape(p.shape).astype(np.float64)
        clear = np.abs(a) > 2 * e1
        with np.errstate(divide="ignore", invalid="ignore"):
            first = np.where(clear, 1e-4 * lr + lr * LR_EPS * e1 / (np.abs(a) - e1) ** 2, 2 * lr)
        bound = first + 1e-4 * lr + 2 * sens + 4 * 2.0 ** -24 * np.abs(ref)
        np.testing.assert_allclose(ref1 - u2, ref, rtol=0, atol=1e-6)          # the float64 formula is the reference's second step
        worst = max(worst, ratio(host(p.data), ref, bound))
        assert_within(host(p.data), ref, bound, f"D parameter {i} after its second step")
    print(f"gan phase 2 (D): parameters after the second step: worst error / bound = {worst:.3f}")
    # ---- phase 3
    g_opt.zero_grad()
    fake_g = gan_example.run_generator(generator, T(f["noise_g"]), dev(f["mask_g"]))
    fake_pred_g = discriminator(fake_g)
    g_loss = loss_fn(fake_pred_g, ones)
    g_loss.backward()
    assert abs(g_loss.item() - float(f["g_loss"])) < 1e-6
    np.testing.assert_allclose(host(fake_g.data), f["fake_g"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(fake_pred_g.data), f["fake_pred_g"], rtol=1e-4, atol=1e-5)
    g_g = [f[f"g_g{i}"] for i in range(ng)]
    gs = grad_list_scale(g_g)
    check_grads("gan phase 3 (G)", gp, g_g, gs)
    g_opt.step()
    check_first_adam_step("gan phase 3 (G)", gp, g_g, [f[f"g_p_after{i}"] for i in range(ng)], lr, gs)
    bns = [m for m in generator.modules if isinstance(m, hip.nn.BatchNorm1d)]
    for k, m in enumerate(bns):                                 # two training forwards each (phases 2 and 3)
        np.testing.assert_allclose(host(m.running_mean.data), f[f"g_bn{k}_running_mean"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(host(m.running_var.data), f[f"g_bn{k}_running_var"], rtol=1e-4, atol=1e-5)
    pg, pd = gan_example.printed_losses(real_pred, fake_pred_g)
    np.testing.assert_allclose([pg, pd], [float(f["print_g_loss"]), float(f["print_d_loss"])], rtol=1e-4)


def test_gan_train_step_runs(hip):
    """examples/gan.py's own train_step (masks drawn on the device) at the tiny size: finite losses, every parameter moved."""
    import gan as gan_example
    from neunet_hip import Tensor
    from neunet_hip.optim import Adam
    cfg = gan_example.CONFIGS["tiny"]
    np.random.seed(0)
    rng = np.random.default_rng(0)
    generator, discriminator = gan_example.make_generator(**cfg), gan_example.make_discriminator(**cfg)
    before = [host(p.data).copy() for p in generator.parameters() + discriminator.parameters()]
    g_opt = Adam(generator.parameters(), lr=0.001, betas=(0.5, 0.999))
    d_opt = Adam(discriminator.parameters(), lr=0.001, betas=(0.5, 0.999))
    T = lambda a: Tensor(a.astype(np.float32), device="cuda", requires_grad=False)      # noqa: E731
    out = gan_example.train_step(generator, discriminator, g_opt, d_opt, hip.nn.MSELoss(),
                                 T(gan_example.synthetic_images(rng, cfg["batch"], cfg["pixels"])),
                                 T(rng.standard_normal((cfg["batch"], cfg["noise"]))), T(rng.standard_normal((cfg["batch"], cfg["noise"]))))
    assert all(np.isfinite(t.item()) for t in out[:3]) and all(np.isfinite(v) for v in gan_example.printed_losses(out[3], out[4]))
    after = [host(p.data) for p in generator.parameters() + discriminator.parameters()]
    assert all(not np.array_equal(a, b) for a, b in zip(before, after))
