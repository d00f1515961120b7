"""CPU: the remaining activations and losses of neunet.nn (ABI 222) -- the float64 restatements of tests/act_ref.py reproduce every
new fixture under tests/golden/ (what the reference computed in float32), the fixtures meet the conditions their generator asserts,
every argument error of the eight new C entries is a status code raised before any device call, and the Python layer exports the ten
names and raises its constructor / argument errors without a device."""
import os
import sys

import numpy as np
import pytest

import act_ref as R

# the fixtures are the reference's own float32 results: its worst error against the float64 closed forms is 4.9e-6 absolute (the
# TanhExp backward), so 1e-5 holds them
FIX = dict(rtol=1e-5, atol=1e-5)
ACT_FIXTURES = [("softplus", "softplus", 0.1), ("softsign", "softsign", 0.1), ("mish", "mish", 0.1), ("tanhexp", "tanhexp", 0.1),
                ("elu_a0.1", "elu", 0.1), ("elu_a1.0", "elu", 1.0), ("selu", "selu", 0.1)]
EINVAL, EALIGN = -1, -2
D = 0x1000          # non-null, 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    import neunet_hip
    from neunet_hip import _lib
    neunet_hip.load_library()
    return _lib


# ===================================================================================================== fixtures vs float64
@pytest.mark.parametrize("tag,kind,alpha", ACT_FIXTURES, ids=[t for t, _, _ in ACT_FIXTURES])
def test_activation_fixture_vs_float64(golden, tag, kind, alpha):
    g = golden(f"act_{tag}")
    X = g["X"]
    assert X.shape == (8, 64) and X.dtype == np.float32
    assert X[0, 0] == 0 and not np.signbit(X[0, 0]) and X[0, 1] == 0 and np.signbit(X[0, 1]) and X[0, 2] == 10 and X[0, 3] == -10
    if kind == "elu":
        assert float(g["alpha"]) == alpha
    np.testing.assert_allclose(g["Y"], R.act_forward(kind, X, alpha), **FIX)
    np.testing.assert_allclose(g["dX"], R.act_backward(kind, X, g["dY"], alpha), **FIX)


@pytest.mark.parametrize("tag", ["last", "axis1_2d", "axis1_4d"])
def test_logsoftmax_fixture_vs_float64(golden, tag):
    g, s = golden(f"logsoftmax_{tag}"), golden(f"softmax_{tag}")
    axis = int(g["axis"])
    assert g["X"].shape == s["X"].shape and axis == int(s["axis"])
    Y = R.logsoftmax_forward(g["X"], axis)
    np.testing.assert_allclose(g["Y"], Y, **FIX)
    np.testing.assert_allclose(g["dX"], R.logsoftmax_backward(Y, g["dY"], axis), **FIX)


def test_log_tape_fixture_vs_float64(golden):
    g = golden("log_tape")
    assert g["X"].min() > 0
    np.testing.assert_allclose(g["Y"], R.act_forward("log", g["X"]), **FIX)
    np.testing.assert_allclose(g["dX"], R.act_backward("log", g["X"], g["dY"]), **FIX)


@pytest.mark.parametrize("dims,shape", [("2d", (6, 50)), ("4d", (2, 5, 3, 4))])
@pytest.mark.parametrize("red", ["mean", "sum", "none"])
def test_nll_fixture_vs_float64(golden, red, dims, shape):
    g = golden(f"nll_{red}_{dims}")
    X, labels, ign = g["X"], g["labels"], int(g["ignore_index"])
    C = shape[1]
    assert X.shape == shape and labels.shape == (shape[0],) + shape[2:] and g["W"].shape == (C,)
    assert 0 <= ign < C and (labels == ign).sum() >= 1 and labels.min() >= 0 and labels.max() < C
    logp = R.logsoftmax_forward(X, 1)
    np.testing.assert_allclose(g["logp"], logp, **FIX)
    loss, dlogp, _ = R.nll(logp.reshape(shape[0], C, -1), labels, g["W"], ign, red)
    ref_loss = g["loss"]
    if red == "none":
        assert ref_loss.shape == ((shape[0], 1) if dims == "2d" else labels.shape)        # what the reference returns
        loss = loss.reshape(ref_loss.shape)
    np.testing.assert_allclose(ref_loss, loss, **FIX)
    np.testing.assert_allclose(g["dlogp"], dlogp.reshape(shape), **FIX)
    np.testing.assert_allclose(g["dX"], R.logsoftmax_backward(logp, dlogp.reshape(shape), 1), **FIX)


@pytest.mark.parametrize("red", ["mean", "sum", "none"])
def test_l1_fixture_vs_float64(golden, red):
    g = golden(f"l1_{red}")
    P, Y = g["P"], g["Y"]
    assert P.shape == (4, 5) and Y.min() >= 0.1 and Y.max() <= 1.0 and not (P == Y).any()
    loss, dP = R.l1(P, Y, red)
    np.testing.assert_allclose(g["loss"], loss, **FIX)
    np.testing.assert_allclose(g["dP"], dP, **FIX)


@pytest.mark.parametrize("tag", ["lin", "log"])
@pytest.mark.parametrize("red", ["mean", "batchmean", "sum", "none"])
def test_kldiv_fixture_vs_float64(golden, red, tag):
    g = golden(f"kldiv_{red}_{tag}")
    P, Y = g["P"], g["Y"]
    assert P.shape == (4, 5) and Y.min() >= 0.1 and Y.max() <= 1.0 and bool(g["log_target"]) == (tag == "log")
    loss, dP = R.kldiv(P, Y, red, tag == "log")
    np.testing.assert_allclose(g["loss"], loss, **FIX)
    np.testing.assert_allclose(g["dP"], dP, **FIX)


@pytest.mark.parametrize("kind", ["cbow", "skipgram"])
def test_word2vec_fixture_conditions_and_first_step(golden, kind):
    """The two conditions the generator asserts, on the stored arrays -- no linear1 pre-activation within 1e-4 of the ReLU kink, every
    probability at a label >= 1e-6 -- and the first step's forward, loss and head gradients restated in float64 from the stored
    initial parameters."""
    g = golden(f"word2vec_{kind}")
    V, dim, cs, hidden, steps = (int(v) for v in g["cfg"])
    assert steps == 3 and g["E_init"].shape == (V, dim) and g["W1_init"].shape[0] == hidden
    for s in range(steps):
        ids, labels, logp = g[f"ids{s}"], g[f"labels{s}"], g[f"logp{s}"]
        assert ids.dtype == np.int16 and labels.dtype == np.int16
        assert ids.shape == ((2 * cs,) if kind == "cbow" else (1,)) and labels.shape == ((1,) if kind == "cbow" else (2 * cs,))
        assert logp.shape == (len(labels), V)
        assert np.abs(g[f"pre{s}"]).min() >= 1e-4
        assert np.exp(logp[np.arange(len(labels)), labels]).min() >= 1e-6
    E, W1, b1, W2, b2 = (g[f"{n}_init"].astype(np.float64) for n in ("E", "W1", "b1", "W2", "b2"))
    ids, labels = g["ids0"], g["labels0"].astype(np.int64)
    pre = E[ids].reshape(1, -1) @ W1.T + b1.reshape(1, -1)
    np.testing.assert_allclose(g["pre0"], pre, rtol=1e-12, atol=1e-12)
    h = np.maximum(pre, 0)
    logits = (h @ W2.T + b2.reshape(1, -1)).reshape(len(labels), V)
    logp = R.logsoftmax_forward(logits, 1)
    np.testing.assert_allclose(g["logp0"], logp, rtol=1e-4, atol=1e-5)
    loss, dlogp, _ = R.nll(logp[:, :, None], labels, None, -100, "mean")
    np.testing.assert_allclose(float(g["loss0"]), loss, rtol=1e-5)
    dlogits = R.logsoftmax_backward(logp, dlogp[:, :, 0], 1).reshape(1, -1)
    np.testing.assert_allclose(g["g0_b2"].reshape(-1), dlogits.reshape(-1), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(g["g0_W2"], dlogits.T @ h, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("kind", ["cbow", "skipgram"])
def test_word2vec_fixture_adam_restated(golden, kind):
    """What the GPU step test's parameter bounds rest on: Adam restated in float64 from the stored gradients reproduces the stored
    parameters of all three steps (to float32 rounding: 1e-6, as test_gan_step_vs_reference holds its restatement), elements whose
    gradient has been exactly 0 so far keep their initial bits, at the first step no other element's gradient sign is unclear, and the
    bounds of act_ref.adam_param_bounds are far below the size of an update (every one below lr / 4, 95 % below lr / 100)."""
    g = golden(f"word2vec_{kind}")
    lr, steps, names = 0.001, int(g["cfg"][4]), ("E", "W1", "b1", "W2", "b2")
    scales = [float(np.median([np.sqrt(np.mean(g[f"g{s}_{n}"].astype(np.float64) ** 2)) for n in names])) for s in range(steps)]
    n_all = n_loose = 0
    for n in names:
        grads = [g[f"g{s}_{n}"].astype(np.float64) for s in range(steps)]
        prev = g[f"{n}_init"].astype(np.float64)
        for s, (bound, untouched, clear) in enumerate(R.adam_param_bounds(grads, scales, lr)):
            ref = g[f"p{s}_{n}"].astype(np.float64)
            np.testing.assert_allclose(prev - R.adam_update(grads[:s + 1], lr), ref, rtol=0, atol=1e-6)
            assert np.array_equal(g[f"p{s}_{n}"][untouched], g[f"{n}_init"][untouched])
            assert np.all(bound[untouched] == 0) and np.all(bound[~untouched] > 0) and bound.max() < lr / 4
            if s == 0:
                assert np.all(clear | untouched)
            if s == steps - 1:
                n_all, n_loose = n_all + bound.size, n_loose + int((bound > lr / 100).sum())
            prev = ref
    assert n_loose < 0.05 * n_all


NEW_FIXTURES = ([f"act_{t}" for t, _, _ in ACT_FIXTURES] + [f"logsoftmax_{t}" for t in ("last", "axis1_2d", "axis1_4d")] + ["log_tape"] +
                [f"nll_{r}_{d}" for r in ("mean", "sum", "none") for d in ("2d", "4d")] + [f"l1_{r}" for r in ("mean", "sum", "none")] +
                [f"kldiv_{r}_{t}" for r in ("mean", "batchmean", "sum", "none") for t in ("lin", "log")] +
                ["word2vec_cbow", "word2vec_skipgram"])


def test_every_new_fixture_is_small():
    from conftest import GOLDEN
    assert len(NEW_FIXTURES) == 30
    for name in NEW_FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 100 * 1024, name


# ===================================================================================================== the C ABI without a device
def test_version_is_222(lib):
    assert lib.load_hip_function("nnhipVersion")() >= 222


def status(lib, name, *args):
    rc = lib.load_hip_function(name)(*args, None)
    assert rc == 0 or name in lib.last_error(), (name, lib.last_error())
    return rc


def test_activation_argument_errors(lib):
    for kind in range(7):
        assert status(lib, "nnhipActivationForward", kind, D, D, 0.1, 0) == 0                      # size 0: a no-op, no launch
        assert status(lib, "nnhipActivationBackward", kind, D, D, D, 0.1, 0) == 0
        assert status(lib, "nnhipActivationForward", kind, D, D, 0.1, -1) == EINVAL and "negative size" in lib.last_error()
        assert status(lib, "nnhipActivationBackward", kind, D, D, D, 0.1, -1) == EINVAL and "negative size" in lib.last_error()
    for kind in (-1, 7, 100):
        assert status(lib, "nnhipActivationForward", kind, D, D, 0.1, 16) == EINVAL and "unknown kind" in lib.last_error()
        assert status(lib, "nnhipActivationBackward", kind, D, D, D, 0.1, 16) == EINVAL and "unknown kind" in lib.last_error()
    for ptrs in ((None, D), (D, None)):
        assert status(lib, "nnhipActivationForward", 0, *ptrs, 0.1, 16) == EINVAL and "null" in lib.last_error()
    for ptrs in ((None, D, D), (D, None, D), (D, D, None)):
        assert status(lib, "nnhipActivationBackward", 0, *ptrs, 0.1, 16) == EINVAL and "null" in lib.last_error()
    assert status(lib, "nnhipActivationForward", 0, D + 2, D, 0.1, 16) == EALIGN


def test_logsoftmax_argument_errors(lib):
    for name, ptrs in (("nnhipLogSoftmaxForward", (D, D)), ("nnhipLogSoftmaxBackward", (D, D, D))):
        assert status(lib, name, *ptrs, 0, 8, 1) == 0 and status(lib, name, *ptrs, 8, 0, 1) == 0   # a zero size is a no-op, as for Softmax
        assert status(lib, name, *ptrs, -1, 8, 1) == EINVAL and status(lib, name, *ptrs, 8, -1, 1) == EINVAL
        assert "negative size" in lib.last_error()
        assert status(lib, name, *ptrs, 8, 8, 0) == EINVAL and "stride" in lib.last_error()
        for k in range(len(ptrs)):
            bad = tuple(None if i == k else D for i in range(len(ptrs)))
            assert status(lib, name, *bad, 8, 8, 1) == EINVAL and "null" in lib.last_error()


def test_nll_argument_errors(lib):
    def nll(logp=D, labels=D, lb=4, cw=None, ign=-100, outer=4, C=5, inner=1, red=b"m", loss=D, dlogp=None, pg=None):
        return status(lib, "nnhipNLLLossForwardBackward", logp, labels, lb, cw, ign, outer, C, inner, red, loss, dlogp, pg)

    assert nll(red=b"x") == EINVAL and "reduction" in lib.last_error()
    assert nll(red=b"b") == EINVAL
    for lb in (0, 1, 3, 16):
        assert nll(lb=lb) == EINVAL and "label_bytes" in lib.last_error()
    for kw in (dict(outer=-1), dict(C=-1), dict(inner=-1)):
        assert nll(**kw) == EINVAL and "negative size" in lib.last_error()
    for kw in (dict(logp=None), dict(labels=None), dict(loss=None)):
        assert nll(**kw) == EINVAL and "null" in lib.last_error()
    assert nll(outer=1 << 40, C=1 << 20, inner=1 << 10) == EINVAL and "overflows" in lib.last_error()

    def fold(dx=D, y=D, labels=D, lb=4, pg=D, up=None, rows=4, cols=5):
        return status(lib, "nnhipLogSoftmaxNLLBackward", dx, y, labels, lb, pg, up, rows, cols)

    assert fold(rows=0) == 0 and fold(cols=0) == 0
    assert fold(rows=-1) == EINVAL and fold(cols=-1) == EINVAL and "negative size" in lib.last_error()
    for lb in (0, 1, 3, 16):
        assert fold(lb=lb) == EINVAL and "label_bytes" in lib.last_error()
    for kw in (dict(dx=None), dict(y=None), dict(labels=None), dict(pg=None)):
        assert fold(**kw) == EINVAL and "null" in lib.last_error()


def test_l1_kldiv_argument_errors(lib):
    def l1(p=D, t=D, loss=D, dp=None, n=8, red=b"m"):
        return status(lib, "nnhipL1LossForwardBackward", p, t, loss, dp, n, red)

    def kl(p=D, t=D, loss=D, dp=None, n=8, batch=2, log_target=0, red=b"m"):
        return status(lib, "nnhipKLDivLossForwardBackward", p, t, loss, dp, n, batch, log_target, red)

    for f in (l1, kl):
        assert f(n=-1) == EINVAL and f(n=0) == EINVAL and "n must be > 0" in lib.last_error()
        assert f(red=b"x") == EINVAL and "reduction" in lib.last_error()
        for kw in (dict(p=None), dict(t=None), dict(loss=None)):
            assert f(**kw) == EINVAL and "null" in lib.last_error()
    assert l1(red=b"b") == EINVAL                                  # batchmean is KLDivLoss's alone
    assert kl(red=b"b", batch=0) == EINVAL and "batch" in lib.last_error()


# ===================================================================================================== the Python layer without a device
NAMES = ("Softplus", "Softsign", "Mish", "TanhExp", "ELU", "SELU", "LogSoftmax", "NLLLoss", "L1Loss", "KLDivLoss")


def test_nn_exports_the_ten_names():
    import neunet_hip.nn as nn
    from neunet_hip.nn.modules import Module
    for n in NAMES:
        assert isinstance(getattr(nn, n)(), Module), n
    assert nn.ELU().alpha == 0.1 and nn.ELU(1.0).alpha == 1.0 and nn.LogSoftmax().axis == 1 and nn.LogSoftmax(-1).axis == -1
    assert nn.SELU().alpha == R.SELU_ALPHA and nn.SELU().lmbda == R.SELU_LAMBDA
    loss = nn.NLLLoss()
    assert (loss.weight, loss.ignore_index, loss.reduction) == (None, -100, "mean")
    assert nn.L1Loss().reduction == "mean" and (nn.KLDivLoss().reduction, nn.KLDivLoss().log_target) == ("mean", False)
    from neunet_hip import Tensor
    assert callable(Tensor.log)


def test_constructor_and_argument_errors():
    import neunet_hip.nn as nn
    from neunet_hip import Tensor
    for cls in (nn.NLLLoss, nn.L1Loss, nn.KLDivLoss):
        with pytest.raises(ValueError, match="Reduction"):
            cls(reduction="avg")
    with pytest.raises(ValueError, match="Reduction"):
        nn.L1Loss(reduction="batchmean")
    nn.KLDivLoss(reduction="batchmean")
    logp = Tensor(np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="Weight shape"):                                   # losses.py:98
        nn.NLLLoss(weight=np.ones(4, np.float32))(logp, Tensor(np.zeros(4), dtype=np.int32, requires_grad=False))
    with pytest.raises(TypeError, match="int dtype"):                                       # losses.py:100
        nn.NLLLoss()(logp, Tensor(np.zeros(4), dtype=np.float32, requires_grad=False))
    with pytest.raises(TypeError, match="tensors"):
        nn.NLLLoss()(logp, np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="cuda"):                                           # no CPU fallback
        nn.NLLLoss()(logp, Tensor(np.zeros(4), dtype=np.int32, requires_grad=False))
    for cls in (nn.L1Loss, nn.KLDivLoss):
        with pytest.raises(TypeError, match="tensors"):
            cls()(logp, np.zeros((4, 5), np.float32))
        with pytest.raises(ValueError, match="equal shapes"):
            cls()(logp, Tensor(np.zeros((4, 6), np.float32)))
        with pytest.raises(NotImplementedError):
            cls()(logp, Tensor(np.zeros((4, 5), np.float32)))
    for act in (nn.Softplus(), nn.ELU(), nn.LogSoftmax()):
        with pytest.raises(NotImplementedError):
            act(logp)
    with pytest.raises(NotImplementedError):
        logp.log()


def test_word2vec_example_pairs_and_vocabulary():
    """The example's pairs are the notebook's (two words before, nearest first, wrapping at the start; two after) over a SORTED vocabulary."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import word2vec as w2v
    vocab, pairs = w2v.make_pairs(w2v.SONNET)
    assert vocab == sorted(set(w2v.SONNET)) and "beauty" in vocab and len(pairs) == len(w2v.SONNET) - 2
    words = [vocab[i] for i in pairs[0][0]]
    assert words == ["cold.", "it", "forty", "winters"] and vocab[pairs[0][1]] == "When"
    assert [vocab[i] for i in pairs[2][0]] == ["forty", "When", "shall", "besiege"] and vocab[pairs[2][1]] == "winters"
