"""GPU: the remaining activations and losses of neunet.nn (ABI 222).  The activation functors of csrc/elementwise.hip, the LogSoftmax
kernels and the LogSoftmax + NLLLoss fold of csrc/rowops.hip and the NLL / L1 / KLDiv kernels of csrc/losses_latent.hip through the C
ABI against the float64 restatements of tests/act_ref.py, at every size where the code takes another path; the modules against the
reference's fixtures; one captured training step; and three steps of examples/word2vec.py against the steps the reference ran.

Bounds.  Fixtures and maps: rtol = atol = 1e-5 (the bound test_swiglu_vs_oracle holds SwiGLU to; the reference's own float32 error
against the closed forms is at most 4.9e-6).  LogSoftmax: the Softmax tier tests' bounds (Y at rtol 1e-5 / atol 1e-6, dX at 1e-4 of
max(|ref|, rms)).  Losses: rtol 1e-5 on a sum of same-signed terms (n terms of relative error <= 2^-23 each and a fixed-order tree sum:
n <= 70001 gives < 2e-6 for blocks of 256 / 1024).  Each test prints its largest error / bound ratio before it asserts (run with -s)."""
import os
import sys

import numpy as np
import pytest

import act_ref as R
from test_hip_parity import assert_close_scaled, assert_within, grad_list_scale
from test_rowops_ref import MAP_SIZES, SOFTMAX_CASES, SOFTMAX_ROWS, SOFTMAX_STRIDED, SPECIALS, case_id, map_inputs, softmax_inputs
from test_rowops_tiers_gpu import Buf, call, close_bound, dev, hip, host, ratio, scaled_bound  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

FIX = dict(rtol=1e-5, atol=1e-5)
KIND = {k: i for i, k in enumerate(R.KINDS)}
ACT_FIXTURES = [("softplus", "softplus", 0.1), ("softsign", "softsign", 0.1), ("mish", "mish", 0.1), ("tanhexp", "tanhexp", 0.1),
                ("elu_a0.1", "elu", 0.1), ("elu_a1.0", "elu", 1.0), ("selu", "selu", 0.1)]
LB = {np.int16: 2, np.int32: 4, np.int64: 8}


def T(a, **kw):
    from neunet_hip import Tensor
    return Tensor(a, device="cuda", **kw)


def act_module(kind, alpha):
    import neunet_hip.nn as nn
    return {"softplus": nn.Softplus, "softsign": nn.Softsign, "mish": nn.Mish, "tanhexp": nn.TanhExp, "selu": nn.SELU}[kind]() \
        if kind != "elu" else nn.ELU(alpha)


def count_calls(monkeypatch):
    """{entry: calls} of everything neunet_hip.nn.experimental.losses launches from here on."""
    import neunet_hip.nn.experimental.losses as Lm
    counts, real = {}, Lm.call_hip_function

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(Lm, "call_hip_function", counting)
    return counts


# ===================================================================================================== fixtures through the modules
@pytest.mark.parametrize("tag,kind,alpha", ACT_FIXTURES, ids=[t for t, _, _ in ACT_FIXTURES])
def test_activation_module_vs_fixture(hip, golden, tag, kind, alpha):
    g = golden(f"act_{tag}")
    x = T(g["X"])
    y = act_module(kind, alpha)(x)
    y.backward(dev(g["dY"]))
    print(f"\n[{tag}] error / bound: Y {ratio(host(y.data), g['Y'], close_bound(g['Y'], 1e-5, 1e-5)):.3f}, "
          f"dX {ratio(host(x.grad), g['dX'], close_bound(g['dX'], 1e-5, 1e-5)):.3f}")
    np.testing.assert_allclose(host(y.data), g["Y"], **FIX)
    np.testing.assert_allclose(host(x.grad), g["dX"], **FIX)
    # the ABI entry on the same data (the module is nothing but this call)
    X, dY = dev(g["X"]), dev(g["dY"])
    Y, dX = torch.empty_like(X), torch.empty_like(X)
    call("nnhipActivationForward", KIND[kind], Y, X, alpha, X.numel())
    call("nnhipActivationBackward", KIND[kind], dX, dY, X, alpha, X.numel())
    assert torch.equal(Y, y.data) and torch.equal(dX, x.grad)


def test_log_tape_vs_fixture(hip, golden):
    g = golden("log_tape")
    x = T(g["X"])
    y = x.log()
    assert y.op == "log"
    y.backward(dev(g["dY"]))
    np.testing.assert_allclose(host(y.data), g["Y"], **FIX)
    np.testing.assert_allclose(host(x.grad), g["dX"], **FIX)


@pytest.mark.parametrize("tag", ["last", "axis1_2d", "axis1_4d"])
def test_logsoftmax_module_vs_fixture(hip, golden, tag):
    import neunet_hip.nn as nn
    g = golden(f"logsoftmax_{tag}")
    x = T(g["X"])
    y = nn.LogSoftmax(axis=int(g["axis"]))(x)
    y.backward(dev(g["dY"]))
    np.testing.assert_allclose(host(y.data), g["Y"], **FIX)
    np.testing.assert_allclose(host(x.grad), g["dX"], **FIX)


@pytest.mark.parametrize("dims", ["2d", "4d"])
@pytest.mark.parametrize("red", ["mean", "sum", "none"])
def test_nll_module_vs_fixture(hip, golden, red, dims):
    """NLLLoss on stored log-probabilities (the dense route: gradient with respect to logp), then LogSoftmax -> NLLLoss from the stored X
    (the fold for the reduced 2-D cases, dense otherwise): the gradient with respect to X."""
    import neunet_hip.nn as nn
    g = golden(f"nll_{red}_{dims}")
    labels = T(g["labels"], dtype=np.int32, requires_grad=False)
    make = lambda: nn.NLLLoss(weight=g["W"], ignore_index=int(g["ignore_index"]), reduction=red)  # noqa: E731
    lp = T(g["logp"])
    loss = make()(lp, labels)
    assert loss.op == "nll" and loss.shape == g["loss"].shape
    loss.backward()
    np.testing.assert_allclose(host(loss.data), g["loss"], **FIX)
    np.testing.assert_allclose(host(lp.grad), g["dlogp"], **FIX)
    x = T(g["X"])
    loss2 = make()(nn.LogSoftmax(axis=1)(x), labels)
    assert loss2.op == ("nll_log_softmax" if dims == "2d" and red != "none" else "nll")
    loss2.backward()
    np.testing.assert_allclose(host(loss2.data), g["loss"], **FIX)
    np.testing.assert_allclose(host(x.grad), g["dX"], **FIX)


@pytest.mark.parametrize("red", ["mean", "sum", "none"])
def test_l1_module_vs_fixture(hip, golden, red):
    import neunet_hip.nn as nn
    g = golden(f"l1_{red}")
    p, t = T(g["P"]), T(g["Y"])
    loss = nn.L1Loss(reduction=red)(p, t)
    loss.backward()
    assert loss.shape == g["loss"].shape and t.grad is None
    np.testing.assert_allclose(host(loss.data), g["loss"], **FIX)
    np.testing.assert_allclose(host(p.grad), g["dP"], **FIX)


@pytest.mark.parametrize("tag", ["lin", "log"])
@pytest.mark.parametrize("red", ["mean", "batchmean", "sum", "none"])
def test_kldiv_module_vs_fixture(hip, golden, red, tag):
    import neunet_hip.nn as nn
    g = golden(f"kldiv_{red}_{tag}")
    p, t = T(g["P"]), T(g["Y"])
    loss = nn.KLDivLoss(reduction=red, log_target=tag == "log")(p, t)
    loss.backward()
    assert loss.shape == g["loss"].shape and t.grad is None
    np.testing.assert_allclose(host(loss.data), g["loss"], **FIX)
    np.testing.assert_allclose(host(p.grad), g["dP"], **FIX)


# ===================================================================================================== the activation maps
def run_act(kind, X, dY, alpha, off):
    n = X.size
    x, dy, y, dx = Buf(X, off), Buf(dY, off), Buf((n,), off), Buf((n,), off)
    call("nnhipActivationForward", KIND[kind], y.t, x.t, alpha, n)
    call("nnhipActivationBackward", KIND[kind], dx.t, dy.t, x.t, alpha, n)
    assert y.intact() and dx.intact() and np.array_equal(x.host(), X, equal_nan=True)
    return y.host(), dx.host()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("n", MAP_SIZES)
def test_activation_map_sizes(hip, n, off):
    """All seven kinds at sizes around the float4 body / scalar tail and the one-block span, aligned and four bytes off (all scalar)."""
    X, dY, _ = map_inputs(n)
    worst = {}
    for kind in R.KINDS:
        Xk = (np.abs(X) + np.float32(0.05)) if kind == "log" else X
        for alpha in ((0.1, 1.0) if kind == "elu" else (0.1,)):
            y, dx = run_act(kind, Xk, dY, alpha, off)
            Yr, dXr = R.act_forward(kind, Xk, alpha), R.act_backward(kind, Xk, dY, alpha)
            worst[kind] = max(worst.get(kind, 0), ratio(y, Yr, close_bound(Yr, 1e-5, 1e-5)), ratio(dx, dXr, close_bound(dXr, 1e-5, 1e-5)))
            np.testing.assert_allclose(y, Yr, err_msg=f"{kind} forward", **FIX)
            np.testing.assert_allclose(dx, dXr, err_msg=f"{kind} backward", **FIX)
    print(f"\n[maps n = {n} off = {off}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
def test_activation_specials(hip, off):
    """SPECIALS plus +-88.8 (exp overflows float32 above 88.72), +-100, -20, -80: every output that is finite in float64 is finite here
    (and within the map bound), a NaN input gives NaN forward and backward, ELU'(0) = alpha and SELU'(0) = lambda alpha for 0 and -0."""
    X = np.concatenate([SPECIALS, np.array([88.8, -88.8, 100.0, -100.0, -20.0, -80.0], np.float32)])
    dY = np.ones_like(X)
    nan = np.isnan(X)
    for kind in R.KINDS[:-1]:
        for alpha in ((0.1, 1.0, 2.5) if kind == "elu" else (0.1,)):
            y, dx = run_act(kind, X, dY, alpha, off)
            for got, ref, what in ((y, R.act_forward(kind, X, alpha), "forward"), (dx, R.act_backward(kind, X, dY, alpha), "backward")):
                fin = np.isfinite(ref)
                assert np.all(np.isfinite(got[fin])), (kind, what, X[fin][~np.isfinite(got[fin])])
                np.testing.assert_allclose(got[fin], ref[fin], err_msg=f"{kind} {what}", **FIX)
                assert np.all(np.isnan(got[nan])), (kind, what)
            if kind == "elu":
                assert dx[0] == np.float32(alpha) and dx[1] == np.float32(alpha)
            if kind == "selu":
                want = np.float32(np.float32(R.SELU_LAMBDA) * np.float32(R.SELU_ALPHA))
                assert abs(dx[0] - want) <= 2.0 ** -23 * want and dx[0] == dx[1]
    Xl = np.array([0.0, -0.0, 1.0, np.inf, np.nan, -1.0, 2.0 ** -126, 3.5, -np.inf], np.float32)
    y, dx = run_act("log", Xl, np.ones_like(Xl), 0.0, off)
    assert y[0] == -np.inf and y[1] == -np.inf and y[2] == 0 and y[3] == np.inf and np.isnan(y[4]) and np.isnan(y[5]) and np.isnan(y[8])
    np.testing.assert_allclose(y[6:8], np.log(Xl[6:8].astype(np.float64)), rtol=1e-6)
    assert dx[0] == np.inf and dx[1] == -np.inf and dx[2] == 1 and dx[3] == 0 and np.isnan(dx[4]) and dx[5] == -1


def test_softplus_keeps_relative_accuracy_far_below_zero(hip):
    """x in [-80, -20]: softplus is exp(x) to first order, a few ulp from one exp; held to rtol 1e-5 (~80 ulp) with NO absolute term.
    (The reference's float32 log(1 + exp(x)) returns exactly 0 below -17.)"""
    X = np.linspace(-80, -20, 4099).astype(np.float32)
    y, _ = run_act("softplus", X, np.ones_like(X), 0.0, 0)
    ref = R.act_forward("softplus", X)
    print(f"\n[softplus -80..-20] worst relative error {np.max(np.abs(y - ref) / ref):.3e}")
    assert np.all(y > 0)
    np.testing.assert_allclose(y, ref, rtol=1e-5, atol=0)


# ===================================================================================================== LogSoftmax
def check_logsoftmax(tag, y, Yr, dx, dXr, axis=-1):
    r_y, r_dx = ratio(y, Yr, close_bound(Yr, 1e-5, 1e-6)), ratio(dx, dXr, scaled_bound(dXr))
    sums = np.exp(y.astype(np.float64)).sum(axis)
    print(f"\n[{tag}] error / bound: Y {r_y:.3f}, dX {r_dx:.3f}; |sum exp(Y) - 1| {np.max(np.abs(sums - 1)):.2e}")
    np.testing.assert_allclose(y, Yr, rtol=1e-5, atol=1e-6, err_msg=tag + " Y")
    assert_close_scaled(dx, dXr, err_msg=tag + " dX")
    # exp(Y) sums to 1 per slice within those tolerances: an error e_i <= 1e-5 |Y_i| + 1e-6 on Y_i moves the sum by p_i e_i, in all by at
    # most 1e-6 + 1e-5 sum_i p_i |Y_i| (the slice's entropy)
    with np.errstate(invalid="ignore"):
        entropy = -np.nansum(np.exp(Yr) * Yr, axis)
    assert np.all(np.abs(sums - 1) <= 1e-6 + 1e-5 * entropy + 2.0 ** -22), tag + " sum exp(Y)"


LOGSOFTMAX_CASES = SOFTMAX_CASES + [(16388, 0), (20001, 0)]


@pytest.mark.parametrize("cols,off", LOGSOFTMAX_CASES, ids=[case_id(c, o) for c, o in LOGSOFTMAX_CASES])
def test_logsoftmax_tiers(hip, cols, off):
    """Every register tier, float4 and scalar by width and by alignment, and the looped kernel: forward, then backward from the kernel's
    own output, both against float64 end to end; two runs are bit-identical."""
    rows = SOFTMAX_ROWS
    X, dY = softmax_inputs(rows, cols, cols + off)
    x, dy, y, dx = Buf(X, off), Buf(dY, off), Buf((rows, cols), off), Buf((rows, cols), off)
    call("nnhipLogSoftmaxForward", y.t, x.t, rows, cols, 1)
    call("nnhipLogSoftmaxBackward", dx.t, dy.t, y.t, rows, cols, 1)
    assert y.intact() and dx.intact() and np.array_equal(x.host(), X) and np.array_equal(dy.host(), dY)
    y1, dx1 = y.host().copy(), dx.host().copy()
    Yr = R.logsoftmax_forward(X)
    check_logsoftmax(f"logsoftmax {case_id(cols, off)}", y1, Yr, dx1, R.logsoftmax_backward(Yr, dY))
    call("nnhipLogSoftmaxForward", y.t, x.t, rows, cols, 1)
    call("nnhipLogSoftmaxBackward", dx.t, dy.t, y.t, rows, cols, 1)
    assert np.array_equal(y.host(), y1) and np.array_equal(dx.host(), dx1)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("outer,n,stride", SOFTMAX_STRIDED, ids=[f"strided-slice{n}-stride{s}" for _, n, s in SOFTMAX_STRIDED])
def test_logsoftmax_strided(hip, outer, n, stride, off):
    X, dY = softmax_inputs(outer * n, stride, n + off)
    X, dY = X.reshape(outer, n, stride), dY.reshape(outer, n, stride)
    x, dy, y, dx = Buf(X, off), Buf(dY, off), Buf(X.shape, off), Buf(X.shape, off)
    call("nnhipLogSoftmaxForward", y.t, x.t, outer * stride, n, stride)
    call("nnhipLogSoftmaxBackward", dx.t, dy.t, y.t, outer * stride, n, stride)
    assert y.intact() and dx.intact()
    check_logsoftmax(f"logsoftmax strided n = {n}", y.host(), R.logsoftmax_forward(X, 1), dx.host(), R.logsoftmax_backward(R.logsoftmax_forward(X, 1), dY, 1), 1)
    if n == 1:
        assert np.all(y.host() == 0) and np.all(dx.host() == 0)


@pytest.mark.parametrize("cols", [6, 260, 4100, 16384, 20001])
def test_logsoftmax_minus_inf_and_shift(hip, cols):
    """A -inf among finite values gives -inf there and finite values elsewhere; rows shifted by +-1e4 give the same Y bit for bit (the
    inputs sit on a 1/64 grid below 8 in size, so x +- 1e4 is exact in float32 and so is x - max)."""
    rng = np.random.default_rng(cols)
    rows = 5
    X = (rng.integers(-500, 500, (rows, cols)) / 64.0).astype(np.float32)
    Xi = X.copy()
    Xi[1, cols // 2] = -np.inf
    Xi[3, 0] = -np.inf
    x, y = dev(Xi), torch.empty((rows, cols), device="cuda")
    call("nnhipLogSoftmaxForward", y, x, rows, cols, 1)
    got = host(y)
    assert got[1, cols // 2] == -np.inf and got[3, 0] == -np.inf
    mask = np.isfinite(Xi)
    assert np.all(np.isfinite(got[mask]))
    np.testing.assert_allclose(got[mask], R.logsoftmax_forward(Xi)[mask], rtol=1e-5, atol=1e-6)
    base = torch.empty((rows, cols), device="cuda")
    call("nnhipLogSoftmaxForward", base, dev(X), rows, cols, 1)
    for shift in (1e4, -1e4):
        Xs = (X + np.float32(shift)).astype(np.float32)
        assert np.array_equal(Xs.astype(np.float64), X.astype(np.float64) + shift)
        call("nnhipLogSoftmaxForward", y, dev(Xs), rows, cols, 1)
        assert torch.equal(y, base), shift


# ===================================================================================================== NLLLoss
def nll_inputs(outer, C, inner, seed, dtype):
    rng = np.random.default_rng(seed)
    logp = -rng.uniform(0.05, 6.0, (outer, C, inner)).astype(np.float32)
    labels = rng.integers(0, C, (outer, inner)).astype(dtype)
    W = rng.uniform(0.5, 2.0, C).astype(np.float32)
    return logp, labels, W


def run_nll(logp, labels, W, ignore, red, dense=True):
    outer, C, inner = logp.shape
    P = outer * inner
    lp, lb = dev(logp), dev(labels, labels.dtype.type)
    w = None if W is None else dev(W)
    outs = []
    for _ in range(2):
        loss = torch.full((P,) if red == "none" else (1,), float("nan"), device="cuda")
        dlogp = torch.full(logp.shape, float("nan"), device="cuda") if dense else None
        pg = torch.full((P,), float("nan"), device="cuda")
        call("nnhipNLLLossForwardBackward", lp, lb, LB[labels.dtype.type], w, ignore, outer, C, inner, red[0].encode(), loss, dlogp, pg)
        outs.append((host(loss), host(dlogp) if dense else None, host(pg)))
    for a, b in zip(*outs):                                               # two runs: bit-identical
        assert a is None or np.array_equal(a, b)
    return outs[0]


def check_nll(tag, logp, labels, W, ignore, red):
    loss, dlogp, pg = run_nll(logp, labels, W, ignore, red)
    rl, rd, rp = R.nll(logp, labels, W, ignore, red)
    outer, C, inner = logp.shape
    if red == "none":
        np.testing.assert_allclose(loss.reshape(outer, inner), rl, rtol=1e-6, atol=0, err_msg=tag)
    else:
        np.testing.assert_allclose(loss[0], rl, rtol=1e-5, atol=0, err_msg=tag)
    np.testing.assert_allclose(pg.reshape(outer, inner), rp, rtol=1e-5, atol=0, err_msg=tag)
    # the dense gradient: exactly zero off the label positions, and pos_grad's bits on them
    lab = labels.astype(np.int64)
    counts = (lab != ignore) & (lab >= 0) & (lab < C)
    n_idx, i_idx = np.indices((outer, inner))
    want = np.zeros_like(dlogp)
    want[n_idx[counts], lab[counts], i_idx[counts]] = pg.reshape(outer, inner)[counts]
    assert np.array_equal(dlogp, want), tag
    assert np.all(pg.reshape(outer, inner)[~counts] == 0), tag
    return loss, pg


NLL_SHAPES = [(1, 1, 1), (5, 7, 1), (260, 256, 1), (3, 20001, 1), (2, 5, 12), (17000, 3, 1), (3, 4, 6000)]


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64], ids=["int16", "int32", "int64"])
@pytest.mark.parametrize("outer,C,inner", NLL_SHAPES, ids=[f"{o}x{c}x{i}" for o, c, i in NLL_SHAPES])
def test_nll_shapes(hip, outer, C, inner, dtype):
    """Every reduction, with and without class weights, one block (<= 16384 positions) and the partial-sum route beyond; some labels
    ignored."""
    logp, labels, W = nll_inputs(outer, C, inner, outer + C + inner, dtype)
    ignore = 0 if C > 1 else -100
    for red in ("mean", "sum", "none"):
        for w in (None, W):
            check_nll(f"nll {outer}x{C}x{inner} {red} {'weighted' if w is not None else 'plain'}", logp, labels, w, ignore, red)


@pytest.mark.parametrize("outer,inner", [(6, 1), (2, 9), (17000, 1)])
def test_nll_label_rules(hip, outer, inner):
    """ignore_index = -100 with 50 classes (the reference raises IndexError there): the ignored positions are never dereferenced; a label
    outside [0, C) that is not ignore_index counts as nothing; all labels ignored gives loss 0 and a zero gradient."""
    C = 50
    logp, labels, W = nll_inputs(outer, C, inner, 7 + outer, np.int64)
    flat = labels.reshape(-1)
    flat[[0, flat.size - 1]] = -100
    flat[1] = C                      # out of range above
    flat[2] = -3                     # and below
    for red in ("mean", "sum", "none"):
        for w in (None, W):
            check_nll(f"nll rules {red}", logp, labels, w, -100, red)
    labels[...] = -100
    for red in ("mean", "sum", "none"):
        loss, dlogp, pg = run_nll(logp, labels, W, -100, red)
        assert np.all(loss == 0) and np.all(dlogp == 0) and np.all(pg == 0) and not np.signbit(pg).any()


# ===================================================================================================== the fold
@pytest.mark.parametrize("rows,cols", [(260, 256), (9, 1001), (3, 16388)], ids=["260x256", "9x1001", "3x16388"])
def test_logsoftmax_nll_fold(hip, monkeypatch, rows, cols):
    """LogSoftmax -> NLLLoss takes the fold (counted: one nnhipLogSoftmaxNLLBackward, no nnhipLogSoftmaxBackward), gives the loss bits of
    the unfolded route and the float64 gradient at the fixture tolerance; with a non-unit scalar upstream; against CrossEntropyLoss."""
    import neunet_hip.nn as nn
    import neunet_hip.nn.experimental.activations as Am
    rng = np.random.default_rng(rows + cols)
    X = (rng.standard_normal((rows, cols)) * 2).astype(np.float32)
    labels = rng.integers(0, cols, rows).astype(np.int32)
    labels[1] = 3                                       # ignored below
    W = rng.uniform(0.5, 2.0, cols).astype(np.float32)
    y_true = T(labels, dtype=np.int32, requires_grad=False)
    counts = count_calls(monkeypatch)
    dense_bwd = []
    real_bwd = Am.hip_logsoftmax_backward
    monkeypatch.setattr(Am, "hip_logsoftmax_backward", lambda *a: (dense_bwd.append(1), real_bwd(*a))[1])
    for red in ("mean", "sum"):
        for k in (None, 0.375):
            Yr = R.logsoftmax_forward(X, 1)
            rl, rd, rp = R.nll(Yr[:, :, None], labels, W, 3, red)
            dXr = R.logsoftmax_nll_backward(Yr, labels, rp, 1.0 if k is None else k)
            counts.clear()
            dense_bwd.clear()
            x = T(X)
            loss = nn.NLLLoss(weight=W, ignore_index=3, reduction=red)(nn.LogSoftmax(axis=1)(x), y_true)
            assert loss.op == "nll_log_softmax" and loss.shape == ()
            loss.backward() if k is None else loss.backward(np.float32(k))
            assert counts == {"nnhipNLLLossForwardBackward": 1, "nnhipLogSoftmaxNLLBackward": 1} and not dense_bwd
            # the unfolded route: the same log-probabilities as a plain tensor's child
            x2 = T(X)
            lp = nn.LogSoftmax(axis=1)(x2)
            plain = lp.reshape(rows, cols)              # a reshape node in between: NLLLoss sees no LogSoftmax tensor
            loss2 = nn.NLLLoss(weight=W, ignore_index=3, reduction=red)(plain, y_true)
            assert loss2.op == "nll"
            loss2.backward() if k is None else loss2.backward(np.float32(k))
            assert len(dense_bwd) == 1
            assert host(loss.data).tobytes() == host(loss2.data).tobytes()
            np.testing.assert_allclose(host(loss.data), rl, rtol=1e-5)
            print(f"\n[fold {rows}x{cols} {red} k = {k}] dX error / bound: folded {ratio(host(x.grad), dXr, close_bound(dXr, 1e-5, 1e-5)):.3f}, "
                  f"unfolded {ratio(host(x2.grad), dXr, close_bound(dXr, 1e-5, 1e-5)):.3f}")
            np.testing.assert_allclose(host(x.grad), dXr, **FIX)
            np.testing.assert_allclose(host(x2.grad), dXr, **FIX)
            assert np.all(host(x.grad)[1] == 0)         # the ignored row: zeros
    # the reference's own CrossEntropyLoss is this composition (losses.py:66-77): same loss and gradient as the fused entry, at the
    # CrossEntropy fixtures' tolerance (test_cross_entropy_golden: loss rtol 1e-5, gradient rtol 1e-5 / atol 1e-6)
    x, xc = T(X), T(X)
    loss = nn.NLLLoss()(nn.LogSoftmax()(x), y_true)
    ce = nn.CrossEntropyLoss()(xc, y_true)
    loss.backward()
    ce.backward()
    np.testing.assert_allclose(loss.item(), ce.item(), rtol=1e-5)
    np.testing.assert_allclose(host(x.grad), host(xc.grad), rtol=1e-5, atol=1e-6)


def test_fold_is_not_taken_for_4d_or_none(hip, monkeypatch):
    import neunet_hip.nn as nn
    counts = count_calls(monkeypatch)
    rng = np.random.default_rng(5)
    X4 = rng.standard_normal((2, 5, 3, 4)).astype(np.float32)
    L4 = rng.integers(0, 5, (2, 3, 4)).astype(np.int64)
    x = T(X4)
    loss = nn.NLLLoss()(nn.LogSoftmax(axis=1)(x), T(L4, dtype=np.int64, requires_grad=False))
    loss.backward()
    assert loss.op == "nll" and "nnhipLogSoftmaxNLLBackward" not in counts
    Yr = R.logsoftmax_forward(X4, 1)
    rl, rd, _ = R.nll(Yr.reshape(2, 5, 12), L4, None, -100, "mean")
    np.testing.assert_allclose(loss.item(), rl, rtol=1e-5)
    np.testing.assert_allclose(host(x.grad), R.logsoftmax_backward(Yr, rd.reshape(X4.shape), 1), **FIX)
    X2 = rng.standard_normal((6, 9)).astype(np.float32)
    L2 = rng.integers(0, 9, 6).astype(np.int16)
    x = T(X2)
    loss = nn.NLLLoss(reduction="none")(nn.LogSoftmax(axis=1)(x), T(L2, dtype=np.int16, requires_grad=False))
    assert loss.op == "nll" and loss.shape == (6, 1)
    up = rng.standard_normal((6, 1)).astype(np.float32)
    loss.backward(up)
    assert "nnhipLogSoftmaxNLLBackward" not in counts
    Yr = R.logsoftmax_forward(X2, 1)
    _, rd, _ = R.nll(Yr[:, :, None], L2, None, -100, "none")
    np.testing.assert_allclose(host(x.grad), R.logsoftmax_backward(Yr, rd[:, :, 0] * up, 1), **FIX)
    # LogSoftmax over axis 0 of a 2-D input: not the composition the fold covers
    loss = nn.NLLLoss()(nn.LogSoftmax(axis=0)(T(X2)), T(L2, dtype=np.int16, requires_grad=False))
    assert loss.op == "nll"


# ===================================================================================================== L1Loss, KLDivLoss
@pytest.mark.parametrize("n", [1, 5, 16384, 16385, 70001])
def test_l1_kldiv_sizes(hip, n):
    """Both sides of the one-block limit (16384) and a size with several partials; every reduction against float64.  L1 at p == t: the
    gradient is 0."""
    rng = np.random.default_rng(n)
    P = rng.uniform(-1, 1, n).astype(np.float32)
    Y = rng.uniform(0.1, 1.0, n).astype(np.float32)
    P[::5] = Y[::5]                                     # exact ties
    batch = 5 if n % 5 == 0 else 1
    p, y = dev(P), dev(Y)
    for red in ("mean", "sum", "none"):
        loss, dp = torch.full((n,) if red == "none" else (1,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        call("nnhipL1LossForwardBackward", p, y, loss, dp, n, red[0].encode())
        rl, rg = R.l1(P, Y, red)
        np.testing.assert_allclose(host(loss) if red == "none" else host(loss)[0], rl, rtol=1e-5, atol=0, err_msg=f"l1 {red}")
        np.testing.assert_allclose(host(dp), rg, rtol=1e-6, atol=0, err_msg=f"l1 {red} gradient")
        assert np.all(host(dp)[::5] == 0)
    for red in ("mean", "batchmean", "sum", "none"):
        for log_target in (0, 1):
            loss, dp = torch.full((n,) if red == "none" else (1,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
            call("nnhipKLDivLossForwardBackward", p, y, loss, dp, n, batch, log_target, red[0].encode())
            rl, rg = R.kldiv(P.reshape(batch, -1), Y.reshape(batch, -1), red, bool(log_target))
            # the terms have either sign: the sum is held to 1e-5 of the sum of their sizes
            terms = np.abs(R.kldiv(P, Y, "none", bool(log_target))[0])
            scale = {"mean": 1.0 / n, "batchmean": 1.0 / batch, "sum": 1.0, "none": 1.0}[red]
            if red == "none":
                np.testing.assert_allclose(host(loss), rl.reshape(-1), rtol=1e-5, atol=1e-6, err_msg=f"kldiv {red}")
            else:
                assert abs(host(loss)[0] - rl) <= 1e-5 * terms.sum() * scale, f"kldiv {red} {log_target}"
            np.testing.assert_allclose(host(dp), rg.reshape(-1), rtol=1e-5, atol=0, err_msg=f"kldiv {red} gradient")


# ===================================================================================================== one captured step
def test_graphed_step_matches_eager(hip):
    """Linear -> ELU -> Linear -> LogSoftmax -> NLLLoss with Adam: one warm-up step and three replays of the captured step equal four
    eager steps bit for bit (losses, parameters)."""
    import neunet_hip.nn as nn
    from neunet_hip import optim
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    rng = np.random.default_rng(3)
    Xs = rng.uniform(-1, 1, (4, 16, 24)).astype(np.float32)
    Ys = rng.integers(0, 10, (4, 16)).astype(np.int32)

    def run(graphed):
        np.random.seed(5)

        class Net(nn.Module):
            def __init__(self):
                super().__init__()
                self.l1, self.act, self.l2, self.head = nn.Linear(24, 32), nn.ELU(), nn.Linear(32, 10), nn.LogSoftmax(axis=1)

            def forward(self, x):
                return self.head(self.l2(self.act(self.l1(x))))

        model = Net()
        ps = model.parameters()
        opt = optim.Adam(ps, lr=1e-3)
        x, y = T(Xs[0], requires_grad=False), T(Ys[0], dtype=np.int32, requires_grad=False)
        loss_fn = nn.NLLLoss()

        def fb():
            loss = loss_fn(model(x), y)
            assert loss.op == "nll_log_softmax"
            loss.backward()
            return loss

        losses = []
        step = GraphedTrainStep(fb, opt, GradBucket(ps), warmup=1) if graphed else None
        for s in range(0 if not graphed else 1, 4):
            x.data.copy_(dev(Xs[s]))
            y.data.copy_(dev(Ys[s], np.int32))
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
        assert np.array_equal(a, b)


# ===================================================================================================== word2vec
def w2v_model(w2v, kind, g, head):
    V, dim, cs, hidden, _ = (int(v) for v in g["cfg"])
    np.random.seed(0)
    model = (w2v.CBOWModeler if kind == "cbow" else w2v.SkipGramModeler)(V, dim, cs, hidden=hidden, head=head).to("cuda")
    named = [("E", model.embeddings.weight), ("W1", model.linear1.weight), ("b1", model.linear1.bias), ("W2", model.linear2.weight),
             ("b2", model.linear2.bias)]
    for n, p in named:
        assert p.size == g[f"{n}_init"].size, (n, p.shape, g[f"{n}_init"].shape)
        p.data.copy_(dev(g[f"{n}_init"]).reshape(p.shape))
    return model, named


@pytest.mark.parametrize("kind", ["cbow", "skipgram"])
def test_word2vec_steps_vs_reference(hip, golden, kind):
    """Three steps of the notebook's loop through examples/word2vec.py's classes, as the reference ran them (tests/golden/word2vec_*.npz):
    log-probabilities at rtol 1e-4 / atol 1e-5, losses to 1e-6 relative, gradients at 1e-4 scaled (the bounds of
    test_vae_step_vs_reference).  Parameters after each Adam step (act_ref.adam_param_bounds): after the first by that test's
    first-step rule -- 1e-4 lr + rounding + lr eps e / (|g| - e)^2 where the gradient's sign is clear, 2 lr elsewhere, fewer than 5 % of
    the elements unclear -- after the second and third by the sensitivity rule of test_gan_step_vs_reference (1e-4 lr + twice the
    largest change of the float64 Adam update when every gradient so far moves by its bound), the steps' bounds added up; an element
    whose reference gradient has been exactly 0 so far (embedding rows no pair has used, units the ReLU keeps off) must keep its
    initial bits.  On these fixtures every bound is below 0.23 lr and 95 % are below 0.01 lr (checked on the CPU,
    test_word2vec_fixture_adam_restated): a missing or wrong-signed update, about lr in size, fails.  --head logsoftmax is held to
    the same bounds, so the two heads' losses agree within twice the loss bound."""
    import word2vec as w2v
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    g = golden(f"word2vec_{kind}")
    lr, steps = 0.001, int(g["cfg"][4])
    losses = {}
    for head in w2v.HEADS:
        model, named = w2v_model(w2v, kind, g, head)
        opt = Adam(model.parameters(), lr=lr)
        loss_fn = nn.NLLLoss()
        losses[head], step_scales = [], []
        for s in range(steps):
            ids = T(g[f"ids{s}"], dtype=np.int16, requires_grad=False)
            labels = T(g[f"labels{s}"], dtype=np.int16, requires_grad=False)
            opt.zero_grad()
            log_probs = model(ids)
            loss = loss_fn(log_probs, labels)
            assert loss.op == ("nll_log_softmax" if head == "logsoftmax" else "nll") and loss.shape == ()
            loss.backward()
            ref_loss = float(g[f"loss{s}"])
            losses[head].append(loss.item())
            refs = [g[f"g{s}_{n}"] for n, _ in named]
            gscale = grad_list_scale(refs)
            worst = max(ratio(host(p.grad).reshape(r.shape), r, scaled_bound(r) + 1e-4 * gscale) for (_, p), r in zip(named, refs))
            print(f"\n[word2vec {kind} {head} step {s}] loss {loss.item():.7f} vs {ref_loss:.7f}; worst gradient error / bound {worst:.3f}")
            assert abs(loss.item() - ref_loss) < 1e-6 * abs(ref_loss)
            np.testing.assert_allclose(host(log_probs.data), g[f"logp{s}"], rtol=1e-4, atol=1e-5)
            for (n, p), r in zip(named, refs):
                assert_close_scaled(host(p.grad).reshape(r.shape), r, err_msg=f"{kind} {head} step {s} grad {n}", scale=gscale)
            opt.step()
            step_scales.append(gscale)
            worst, n_unclear, n_all = 0.0, 0, 0
            for n, p in named:
                ref = g[f"p{s}_{n}"].astype(np.float64)
                bound, untouched, clear = R.adam_param_bounds([g[f"g{k}_{n}"] for k in range(s + 1)], step_scales, lr)[s]
                got = host(p.data).reshape(ref.shape)
                assert np.array_equal(got[untouched], g[f"{n}_init"][untouched]), f"{kind} {head} parameter {n}: an element Adam never touched moved"
                bound = bound + 2 * (s + 1) * 2.0 ** -24 * np.abs(ref)
                live = ~untouched
                worst = max(worst, ratio(got[live], ref[live], bound[live]))
                if s == 0:                              # the first-step rule's condition: few gradients of unclear sign
                    n_unclear, n_all = n_unclear + int((live & ~clear).sum()), n_all + ref.size
                assert_within(got[live], ref[live], bound[live], f"{kind} {head} parameter {n} after step {s}")
            print(f"[word2vec {kind} {head} step {s}] parameters after Adam: worst error / bound {worst:.3f}")
            assert s > 0 or n_unclear < 0.05 * n_all
    for a, b in zip(losses["softmax-log"], losses["logsoftmax"]):       # both heads within 1e-6 of the reference's loss: within 2e-6 of each other
        assert abs(a - b) < 2e-6 * abs(a)


def test_word2vec_example_runs_and_learns(hip, capsys):
    """main(["--epochs", "2", "--model", "both"]) runs both models on the whole sonnet and the summed loss falls."""
    import word2vec as w2v
    results = w2v.main(["--epochs", "2", "--model", "both"])
    out = capsys.readouterr().out
    assert set(results) == {"cbow", "skipgram"} and out.count('Embedding of the word "beauty"') == 2 and "steps/s" in out
    for kind, totals in results.items():
        assert len(totals) == 2 and np.isfinite(totals).all() and totals[1] < totals[0], (kind, totals)
