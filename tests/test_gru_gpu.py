"""GPU: nn.GRU, nn.RNN and nn.Bidirectional on the one-launch recurrence kernels (csrc/recurrent_gru.hip) against the reference's
fixtures (tools/gen_golden.py: gen_gru, gen_rnn, gen_bidirectional), the notebook's model through the example's class, and hipGraph
replays against eager calls.  tests/test_gru_tiers_gpu.py walks the kernel instances through the C ABI."""
import importlib.util
import os

import numpy as np
import pytest

from test_gru import BI_CASES, GRU_CASES, GRU_NAMES, RNN_CASES, RNN_NAMES, parse_rs
from test_hip_parity import assert_close_scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def host(t):
    return t.detach().cpu().numpy()


def load_params(m, arrays):
    import torch
    ps = m.parameters()
    assert len(ps) == len(arrays)
    for p, a in zip(ps, arrays):
        p.data.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    return ps


def run_case(hip, f, m, n_params, names, state=False):
    """Every call of a fixture through the module: outputs rtol = atol = 1e-4, gradients assert_close_scaled(1e-4)."""
    import torch
    ps = load_params(m, [f[f"p{i}"] for i in range(n_params)])
    calls = int(f["cfg"][4])
    for c in range(calls):
        x = hip.Tensor(f[f"X{c}"], device="cuda")
        out = m(x, torch.from_numpy(f["h0"]).cuda()) if state else m(x)
        outs = out if isinstance(out, tuple) else (out,)
        assert len(outs) == len([k for k in f if k.startswith(f"Y{c}_")])
        for k, o in enumerate(outs):
            assert tuple(o.shape) == f[f"Y{c}_{k}"].shape
            np.testing.assert_allclose(host(o.data), f[f"Y{c}_{k}"], rtol=1e-4, atol=1e-4, err_msg=f"Y{c}_{k}")
            if f"dY{c}_{k}" in f:
                o.backward(torch.from_numpy(f[f"dY{c}_{k}"]).cuda())
        if f"dX{c}" in f:
            assert tuple(x.grad.shape) == f[f"X{c}"].shape
            assert_close_scaled(host(x.grad), f[f"dX{c}"], err_msg=f"dX{c}")
    if "g0" in f:
        for i, p in enumerate(ps):
            assert_close_scaled(host(p.grad), f[f"g{i}"], err_msg=f"{names[i % len(names)]} ({i})")
    return ps


@pytest.mark.parametrize("name", GRU_CASES)
def test_gru_fixture(hip, golden, name):
    import neunet_hip.nn as nn
    f = golden(name)
    B, T, n_in, H, calls = (int(v) for v in f["cfg"])
    m = nn.GRU(n_in, H, nonlinearity=str(f["modes"][0]), recurrent_nonlinearity=str(f["modes"][1]), return_sequences=parse_rs(f["modes"][2]),
               cycled_states=calls > 1)
    run_case(hip, f, m, 9, GRU_NAMES, state="h0" in f)


@pytest.mark.parametrize("name", RNN_CASES)
def test_rnn_fixture(hip, golden, name):
    import neunet_hip.nn as nn
    f = golden(name)
    B, T, n_in, H, calls = (int(v) for v in f["cfg"])
    m = nn.RNN(n_in, H, nonlinearity=str(f["modes"][0]), return_sequences=parse_rs(f["modes"][2]), cycled_states=calls > 1)
    run_case(hip, f, m, 3, RNN_NAMES)


@pytest.mark.parametrize("name", BI_CASES)
def test_bidirectional_fixture(hip, golden, name):
    """bi_gru_both is forward only in the fixture (the reference's backward raises); here its two outputs also back-propagate, and
    the result is the sum of the two single-output backward passes."""
    import torch
    import neunet_hip.nn as nn
    f = golden(name)
    B, T, n_in, H, _ = (int(v) for v in f["cfg"])
    kind, merge, rs = str(f["modes"][0]), str(f["modes"][1]), parse_rs(f["modes"][2])
    make = lambda r: nn.Bidirectional(getattr(nn, kind)(n_in, H, return_sequences=r), merge_mode=merge)   # noqa: E731
    n = 18 if kind == "GRU" else 6
    ps = run_case(hip, f, make(rs), n, GRU_NAMES if kind == "GRU" else RNN_NAMES)
    if name != "bi_gru_both":
        return
    rng = np.random.default_rng(3)
    dA = torch.from_numpy(rng.uniform(-1, 1, (B, T, H)).astype(np.float32)).cuda()
    dL = torch.from_numpy(rng.uniform(-1, 1, (B, 1, H)).astype(np.float32)).cuda()
    arrays = [f[f"p{i}"] for i in range(n)]
    got = {}
    for tag, r in (("both", "both"), ("all", "all"), ("last", "last")):
        m = make(r)
        ps = load_params(m, arrays)
        x = hip.Tensor(f["X0"], device="cuda")
        out = m(x)
        if tag == "both":
            out[0].backward(dA)
            out[1].backward(dL)
        else:
            out.backward(dA if tag == "all" else dL)
        got[tag] = [host(x.grad)] + [host(p.grad) for p in ps]
    for i, (b, a, l) in enumerate(zip(got["both"], got["all"], got["last"])):
        assert_close_scaled(b, a.astype(np.float64) + l, err_msg=f"both vs all + last: tensor {i}")


@pytest.mark.parametrize("kind", ["GRU", "RNN"])
def test_state_shape_errors(hip, kind):
    """hprev (and the GRU's cprev) must be (batch, hidden); the checks sit behind the device-tensor check, so they need a device."""
    import torch
    import neunet_hip.nn as nn
    B, T, n_in, H = 3, 4, 5, 16
    m = getattr(nn, kind)(n_in, H, return_sequences="all")
    x = hip.Tensor(np.zeros((B, T, n_in), np.float32), device="cuda")
    good = torch.zeros((B, H), device="cuda")
    for bad in (torch.zeros((B, 1, H), device="cuda"), torch.zeros((B + 1, H), device="cuda"), torch.zeros((B, H + 1), device="cuda")):
        with pytest.raises(ValueError, match="hprev shape"):
            m(x, bad)
        if kind == "GRU":
            with pytest.raises(ValueError, match="cprev shape"):
                m(x, good, bad)
            with pytest.raises(ValueError, match="cprev shape"):
                m(x, None, bad)
    with pytest.raises(ValueError, match="input_size"):
        m(hip.Tensor(np.zeros((B, T, n_in + 1), np.float32), device="cuda"))
    assert tuple(m(x, good).shape) == (B, T, H)


def test_gru_cprev_is_accepted_and_unused(hip, golden):
    """A right-shaped cprev changes nothing: outputs, dX and every gradient are those of the call without it, bit for bit (in the
    reference it only fills cell_states[:, -1], which nothing reads: gru.py:266)."""
    import torch
    import neunet_hip.nn as nn
    f = golden("gru_state")
    B, T, n_in, H, _ = (int(v) for v in f["cfg"])
    h0 = torch.from_numpy(f["h0"]).cuda()
    c0 = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (B, H)).astype(np.float32)).cuda()
    dY = torch.from_numpy(f["dY0_0"]).cuda()
    got = []
    for args in ((h0,), (h0, c0), (h0, hip.Tensor(c0, device="cuda"))):
        m = nn.GRU(n_in, H, return_sequences=False)
        ps = load_params(m, [f[f"p{i}"] for i in range(9)])
        x = hip.Tensor(f["X0"], device="cuda")
        out = m(x, *args)
        out.backward(dY)
        got.append([host(out.data), host(x.grad)] + [host(p.grad) for p in ps])
    np.testing.assert_allclose(got[0][0], f["Y0_0"], rtol=1e-4, atol=1e-4)
    for other in got[1:]:
        for a, b in zip(got[0], other):
            np.testing.assert_array_equal(a, b)


def example_module():
    spec = importlib.util.spec_from_file_location("recurrent_sequences", os.path.join(ROOT, "examples", "recurrent_sequences.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sequence_classifier_two_adam_steps(hip, golden):
    """The notebook's model through the example's class: one Adam step on each of two sentences of different true length (five words;
    two words and three padding zeros), the loss, every gradient and every parameter after each step against the reference."""
    import torch
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    f = {**golden("seqcls_step_0"), **golden("seqcls_step_1")}
    model = example_module().SequenceClassifier()
    ps = model.parameters()
    assert len(ps) == int(f["n_params"])
    for i, p in enumerate(ps):
        p.data.copy_(torch.from_numpy(f[f"p{i}"]))
    opt = Adam(ps, lr=0.001)
    loss_fn = nn.MSELoss()
    for st in range(2):
        opt.zero_grad()
        out = model(hip.Tensor(f["tokens"][st], dtype=np.int32, device="cuda", requires_grad=False))
        assert tuple(out.shape) == (1, 1, 1)
        label = hip.Tensor(np.full((1, 1, 1), f["labels"][st], np.float32), device="cuda", requires_grad=False)
        loss = loss_fn(out, label)
        loss.backward()
        assert abs(loss.item() - f["losses"][st]) < 1e-5
        np.testing.assert_allclose(host(out.data), f["outs"][st], rtol=1e-4, atol=1e-5)
        grads = [f[f"g{st}_{i}"] for i in range(len(ps))]
        for i, p in enumerate(ps):
            assert_close_scaled(host(p.grad), grads[i], err_msg=f"step {st} gradient {i}")
        opt.step()
        for i, p in enumerate(ps):
            np.testing.assert_allclose(host(p.data), f[f"pf{st}_{i}"], rtol=1e-4, atol=1e-5, err_msg=f"step {st} parameter {i}")


@pytest.mark.parametrize("what", ["gru", "bidirectional"])
def test_graph_replay_is_bit_identical_to_eager(hip, what):
    """One layer / one Bidirectional layer with cycled states, forward and backward captured in a hipGraph and replayed twice: outputs,
    dX and parameter gradients are bit-identical to three eager calls' (the capture's warm-up call included), and the carried state
    advances per replay."""
    import torch
    import neunet_hip.nn as nn
    rng = np.random.default_rng(11)
    B, T, n_in, H = 5, 7, 6, 50
    xs = [rng.uniform(-1, 1, (B, T, n_in)).astype(np.float32) for _ in range(3)]
    dY = torch.from_numpy(rng.uniform(-1, 1, (B, T, H)).astype(np.float32)).cuda()

    def make():
        np.random.seed(9)
        layer = nn.GRU(n_in, H, return_sequences="all", cycled_states=True)
        m = layer if what == "gru" else nn.Bidirectional(layer, merge_mode="mul")
        x = hip.Tensor(xs[0], device="cuda")
        return m, x

    def step(m, x):
        x.grad = None
        for p in m.parameters():
            p.grad = None
        y = m(x)
        y.backward(dY)
        return y

    def state_of(m):
        return host(m.hprev if what == "gru" else m._state).copy()

    def snapshot(m, x, y):
        return [host(y.data).copy(), host(x.grad).copy(), state_of(m)] + [host(p.grad).copy() for p in m.parameters()]

    m1, x1 = make()
    eager = []
    for k in range(3):
        x1.data.copy_(torch.from_numpy(xs[k]).cuda())
        eager.append(snapshot(m1, x1, step(m1, x1)))
    assert not np.array_equal(eager[0][2], eager[1][2]) and not np.array_equal(eager[1][2], eager[2][2])

    import gc
    from neunet_hip._lib import call_hip_function
    m2, x2 = make()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        y = step(m2, x2)                                          # warm-up on xs[0]: grows the workspace, creates the state buffer
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    for a, b in zip(snapshot(m2, x2, y), eager[0]):
        np.testing.assert_array_equal(a, b)
    graph = torch.cuda.CUDAGraph()
    gc.collect()
    gc.disable()                                                  # a collection inside the capture region may free an earlier graph's pool
    try:
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            y = step(m2, x2)
    finally:
        gc.enable()
    call_hip_function("nnhipWorkspaceLock", 1)                    # the captured kernels hold workspace addresses
    try:
        held = [y.data, x2.grad] + [p.grad for p in m2.parameters()]
        for k in (1, 2):
            x2.data.copy_(torch.from_numpy(xs[k]).cuda())
            graph.replay()
            torch.cuda.synchronize()
            got = [host(held[0]), host(held[1]), state_of(m2)] + [host(g) for g in held[2:]]
            for i, (a, b) in enumerate(zip(got, eager[k])):
                np.testing.assert_array_equal(a, b, err_msg=f"replay {k}, tensor {i}")
    finally:
        call_hip_function("nnhipWorkspaceLock", 0)
        del graph
