"""GPU: nn.LSTM on the one-launch recurrence kernels (csrc/recurrent.hip) against the reference's fixtures and, at the notebook's
size and beyond, against the float64 restatement (tests/lstm_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lstm_ref import lstm_backward, lstm_forward
from test_lstm import CASES, NAMES
from test_hip_parity import assert_close_scaled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def make_layer(hip, n_in, H, params, **kw):
    import torch
    import neunet_hip.nn as nn
    m = nn.LSTM(n_in, H, **kw)
    for p, a in zip(m.parameters(), params):
        p.data.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    return m


def host(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_lstm_fixture(hip, golden, name):
    import torch
    f = golden(name)
    B, T, n_in, H, calls = (int(v) for v in f["cfg"])
    nl, rnl, rs = (str(v) for v in f["modes"])
    rs = {"True": True, "False": False}.get(rs, rs)
    m = make_layer(hip, n_in, H, [f[f"p{i}"] for i in range(12)], nonlinearity=nl, recurrent_nonlinearity=rnl,
                   return_sequences=rs, cycled_states=calls > 1)
    for c in range(calls):
        x = hip.Tensor(f[f"X{c}"], device="cuda")
        if "h0" in f:
            out = m(x, torch.from_numpy(f["h0"]).cuda(), torch.from_numpy(f["c0"]).cuda())
        else:
            out = m(x)
        outs = out if isinstance(out, tuple) else (out,)
        for k, o in enumerate(outs):
            np.testing.assert_allclose(host(o.data), f[f"Y{c}_{k}"], rtol=1e-4, atol=1e-4, err_msg=f"Y{c}_{k}")
            o.backward(torch.from_numpy(f[f"dY{c}_{k}"]).cuda())
        assert tuple(x.grad.shape) == f[f"X{c}"].shape
        assert_close_scaled(host(x.grad), f[f"dX{c}"], err_msg=f"dX{c}")
    for i, p in enumerate(m.parameters()):
        assert_close_scaled(host(p.grad), f[f"g{i}"], err_msg=NAMES[i])


def run_layer(hip, X, params, dY, dYl, **kw):
    import torch
    B, T, n_in = X.shape
    H = params[4].shape[0]
    m = make_layer(hip, n_in, H, params, **kw)
    x = hip.Tensor(X, device="cuda")
    Y, last = m(x)
    Y.backward(torch.from_numpy(dY).cuda())
    last.backward(torch.from_numpy(dYl.reshape(B, 1, H)).cuda())
    return host(Y.data), host(x.grad), [host(p.grad) for p in m.parameters()]


@pytest.mark.parametrize("n_in,H", [(28, 128), (128, 128), (64, 256), (32, 512)])
def test_lstm_notebook_size_vs_float64(hip, n_in, H):
    """B = 100, T = 28: the recurrent digits classifier's layers (in 28 / 128, H = 128, W_h register-resident) and wider layers whose
    W_h is re-read from L2 every step."""
    rng = np.random.default_rng(H + n_in)
    B, T = 100, 28
    s = 1 / np.sqrt(H)
    params = [rng.uniform(-s, s, (n_in, H)) for _ in range(4)] + [rng.uniform(-s, s, (H, H)) for _ in range(4)] + \
             [rng.uniform(-s, s, H) for _ in range(4)]
    params = [a.astype(np.float32) for a in params]
    X = rng.uniform(-1, 1, (B, T, n_in)).astype(np.float32)
    dY = rng.uniform(-1, 1, (B, T, H)).astype(np.float32)
    dYl = rng.uniform(-1, 1, (B, H)).astype(np.float32)
    Y, dX, grads = run_layer(hip, X, params, dY, dYl)
    Yr, cache = lstm_forward(X, params)
    dXr, gr = lstm_backward(cache, dY, dYl)
    np.testing.assert_allclose(Y, Yr, rtol=1e-4, atol=1e-4)
    assert_close_scaled(dX, dXr, err_msg="dX")
    for i in range(12):
        assert_close_scaled(grads[i], gr[i], err_msg=NAMES[i])
    # bit-identical across runs: no atomics anywhere in the forward, the recurrence or the reductions
    Y2, dX2, grads2 = run_layer(hip, X, params, dY, dYl)
    np.testing.assert_array_equal(Y2, Y)
    np.testing.assert_array_equal(dX2, dX)
    for a, b in zip(grads2, grads):
        np.testing.assert_array_equal(a, b)


class Classifier:
    def __init__(self, H, nn):
        self.lstm1 = nn.LSTM(28, H, return_sequences=True)
        self.lstm2 = nn.LSTM(H, H, return_sequences=False)
        self.fc1 = nn.Linear(H, 10)
        self.sigmoid = nn.Sigmoid()

    def parameters(self):
        return self.lstm1.parameters() + self.lstm2.parameters() + self.fc1.parameters()

    def __call__(self, x):
        h = self.lstm2(self.lstm1(x))
        return self.sigmoid(self.fc1(h.reshape(h.shape[0], -1)))


def test_lstm_classifier_two_adam_steps(hip, golden):
    import torch
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    f = golden("lstm_classifier")
    model = Classifier(32, nn)
    ps = model.parameters()
    assert len(ps) == int(f["n_params"])
    for i, p in enumerate(ps):
        p.data.copy_(torch.from_numpy(f[f"p{i}"]))
    opt = Adam(ps, lr=0.001)
    loss_fn = nn.MSELoss()
    for st in range(2):
        opt.zero_grad()
        out = model(hip.Tensor(f["X"][st], device="cuda"))
        loss = loss_fn(out, hip.Tensor(f["T"][st], device="cuda", requires_grad=False))
        loss.backward()
        opt.step()
        assert abs(loss.item() - f["losses"][st]) < 1e-5
        np.testing.assert_allclose(host(out.data), f["outs"][st], rtol=1e-4, atol=1e-5)
    for i, p in enumerate(ps):
        np.testing.assert_allclose(host(p.data), f[f"pf{i}"], rtol=1e-4, atol=1e-5, err_msg=str(i))


def test_lstm_graphed_step_matches_eager(hip):
    """The notebook-size classifier (B 100, T 28, H 128) replayed from a hipGraph is bit-identical to the eager step for 3 steps;
    a cycled-state LSTM in the same model carries its state across replays as it does across eager calls."""
    import torch
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    rng = np.random.default_rng(5)
    B = 100
    xs = [rng.uniform(-1, 1, (B, 28, 28)).astype(np.float32) for _ in range(6)]
    ts = [np.eye(10, dtype=np.float32)[rng.integers(0, 10, B)] for _ in range(6)]

    def make():
        np.random.seed(7)
        model = Classifier(128, nn)
        model.lstm1 = nn.LSTM(28, 128, return_sequences=True, cycled_states=True)
        x = hip.Tensor(xs[0], device="cuda", requires_grad=False)
        t = hip.Tensor(ts[0], device="cuda", requires_grad=False)
        loss_fn = nn.MSELoss()

        def fb():
            loss = loss_fn(model(x), t)
            loss.backward()
            return loss

        opt = Adam(model.parameters(), lr=1e-3)
        return model, x, t, fb, opt

    m1, x1, t1, fb1, opt1 = make()
    losses1 = []
    for k in [0, 0] + list(range(1, 4)):                    # the graphed run warms up twice on batch 0
        x1.data.copy_(torch.from_numpy(xs[k]).cuda())
        t1.data.copy_(torch.from_numpy(ts[k]).cuda())
        opt1.zero_grad()
        losses1.append(fb1().item())
        opt1.step()
    m2, x2, t2, fb2, opt2 = make()
    g = GraphedTrainStep(fb2, opt2, GradBucket(m2.parameters()), warmup=2)
    losses2 = []
    for k in range(1, 4):
        x2.data.copy_(torch.from_numpy(xs[k]).cuda())
        t2.data.copy_(torch.from_numpy(ts[k]).cuda())
        losses2.append(g().item())
    torch.cuda.synchronize()
    assert losses2 == losses1[2:]
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        np.testing.assert_array_equal(host(p2.data), host(p1.data))
    np.testing.assert_array_equal(host(m2.lstm1.hprev), host(m1.lstm1.hprev))
    np.testing.assert_array_equal(host(m2.lstm1.cprev), host(m1.lstm1.cprev))
    g.release()


def test_recurrent_classifier_example_learns():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "recurrent_classifier.py"), "--steps", "50"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [float(l.split("loss")[1].split()[0]) for l in r.stdout.splitlines() if "loss" in l]
    assert len(losses) >= 2 and losses[-1] < losses[0], r.stdout
