"""GPU: SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax and NAdam on the kernels of csrc/optim_rules.hip -- against fixtures recorded
from the reference (tools/gen_golden.py: gen_optim_rules) and against its float32 restatement (tests/optim_ref.py) at the sizes
where the kernel changes path; the plumbing the classes share with Adam (skipped parameters, strided gradients, grad_scale, the
device gradient divisor, hipGraph replay); a training trajectory; the example.

Tolerances: test_adam_golden's (rtol 1e-5; atol 1e-6 parameters, 1e-7 first state, 1e-8 second state)."""
import importlib.util
import os

import numpy as np
import pytest

import optim_ref
from optim_ref import CLASS_NAMES, N_STATE, RULES
from test_optim import ATOL_P, ATOL_S, RTOL, RULE_ID, check_against_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_NAMES = "mv"


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                 # a copy: the shared test data stays read-only


def host(t):
    return t.detach().cpu().numpy()


def make_params(hip, arrays):
    from neunet_hip.nn import Parameter
    return [Parameter(hip.Tensor(a, device="cuda")) for a in arrays]


def make_opt(rule, params, **kw):
    from neunet_hip import optim
    return getattr(optim, CLASS_NAMES[rule])(params, **kw)


def opt_states(opt, i):
    return [getattr(opt, n)[i] for n in STATE_NAMES[:opt.n_state]]


def assert_matches(opt, params, ref_p, ref_s, idx=None, what=""):
    """Device parameters and states against the restatement's, at the tolerances above.  idx: per tensor, flat indices to compare
    (None: all)."""
    for i, p in enumerate(params):
        sel = slice(None) if idx is None or idx[i] is None else idx[i]
        np.testing.assert_allclose(host(p.data).reshape(-1)[sel], ref_p[i].reshape(-1), rtol=RTOL, atol=ATOL_P, err_msg=f"{what} p[{i}]")
        for k, s in enumerate(opt_states(opt, i)):
            np.testing.assert_allclose(host(s).reshape(-1)[sel], ref_s[i][k].reshape(-1), rtol=RTOL, atol=ATOL_S[k],
                                       err_msg=f"{what} {STATE_NAMES[k]}[{i}]")


# ------------------------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("rule", RULES)
def test_golden_through_the_class(hip, golden, rule):
    g = golden(f"optim_{rule}")
    n = int(g["n_tensors"])
    params = make_params(hip, [g[f"p0_{i}"] for i in range(n)])
    opt = make_opt(rule, params)                                   # the reference's defaults, as recorded
    assert opt.lr == float(g["lr"])
    for s in range(3):
        for i, p in enumerate(params):
            p.grad = dev(g[f"g{s}_{i}"])
        opt.step()
        check_against_fixture(g, s, [host(p.data) for p in params], [[host(t) for t in opt_states(opt, i)] for i in range(n)])


@pytest.mark.parametrize("rule", RULES)
def test_golden_through_the_per_tensor_entry(hip, golden, rule):
    import torch
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    g = golden(f"optim_{rule}")
    n = int(g["n_tensors"])
    c1, c2, eps = optim_ref.coefficients(rule, {})
    ps = [dev(g[f"p0_{i}"]) for i in range(n)]
    ss = [[torch.zeros_like(p) for _ in range(N_STATE[rule])] for p in ps]
    for s in range(3):
        for i in range(n):
            s1 = ss[i][0] if N_STATE[rule] >= 1 else None          # state pointers the rule does not have: NULL
            s2 = ss[i][1] if N_STATE[rule] >= 2 else None
            call_hip_function("nnhipOptimizerRuleStep", RULE_ID[rule], ps[i], dev(g[f"g{s}_{i}"]), s1, s2, ps[i].numel(), float(g["lr"]),
                              c1, c2, eps, s + 1, 1.0, get_current_stream_ptr())
        check_against_fixture(g, s, [host(p) for p in ps], [[host(t) for t in ss[i]] for i in range(n)])


# ----------------------------------------------------------------------------------- the sizes where the kernel changes path
# small-chunk plan (2048 elements per block): tails of 1-3 elements, a chunk boundary and one element past it, a chunk of which
# only some threads take the unrolled rounds
EDGE_SHAPES = [(1000, 333), (7,), (16385,), (1,), (2048,), (2049,)]
# >= 2^22 elements in all: the 16384-element chunk
LARGE_SHAPES = [(2048, 2048), (16385,), (3,)]
_data_cache = {}


def shape_data(shapes):
    """Initial values and three steps of gradients (standard normal), shared by the rules and left unchanged."""
    key = tuple(shapes)
    if key not in _data_cache:
        rng = np.random.default_rng(2210)
        p0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
        gs = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(3)]
        for a in p0 + [x for step in gs for x in step]:
            a.setflags(write=False)
        _data_cache[key] = (p0, gs)
    return _data_cache[key]


def run_against_ref(hip, rule, shapes, idx=None, grad_scale=1.0):
    p0, gs = shape_data(shapes)
    params = make_params(hip, p0)
    opt = make_opt(rule, params)
    opt.grad_scale = grad_scale
    pick = (lambda i, a: a.reshape(-1).copy()) if idx is None else (lambda i, a: a.reshape(-1)[idx[i]].copy() if idx[i] is not None else a.reshape(-1).copy())
    ref_p = [pick(i, a) for i, a in enumerate(p0)]
    ref_s = [optim_ref.init_state(rule, a) for a in ref_p]
    for s in range(3):
        for i, p in enumerate(params):
            p.grad = dev(gs[s][i])
            optim_ref.step(rule, ref_p[i], pick(i, gs[s][i]), ref_s[i], s + 1, grad_scale=grad_scale)
        opt.step()
        assert_matches(opt, params, ref_p, ref_s, idx, what=f"{rule} step {s + 1}")
    return opt, params


@pytest.mark.parametrize("rule", RULES)
def test_edge_shapes_against_ref(hip, rule):
    assert sum(int(np.prod(s)) for s in EDGE_SHAPES) < 1 << 22
    run_against_ref(hip, rule, EDGE_SHAPES)


@pytest.mark.parametrize("rule", RULES)
def test_large_chunk_against_ref(hip, rule):
    """The 16384-element chunk.  The rules are elementwise: the restatement runs on a sample of the large tensor (its first and last
    chunk whole, every 1021st element between), and on the two small tensors in full."""
    n0 = int(np.prod(LARGE_SHAPES[0]))
    assert n0 + 16385 + 3 >= 1 << 22
    sample = np.unique(np.concatenate([np.arange(16384 + 8), np.arange(n0 - 16384 - 8, n0), np.arange(0, n0, 1021)]))
    run_against_ref(hip, rule, LARGE_SHAPES, idx=[sample, None, None])


@pytest.mark.parametrize("rule", RULES)
def test_unaligned_views_take_the_scalar_path_bit_for_bit(hip, rule):
    """Parameter, gradient and states that start one float into their buffers (4-byte alignment only) against the aligned run."""
    import torch
    rng = np.random.default_rng(2211)
    sizes = [2051, 7]
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    gs = [[rng.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(3)]

    def shifted(a):
        buf = torch.zeros(a.size + 5, dtype=torch.float32, device="cuda")
        view = buf[1:1 + a.size]
        view.copy_(dev(a))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    results = []
    for unaligned in (False, True):
        params = make_params(hip, p0)
        opt = make_opt(rule, params)
        if unaligned:
            for i, p in enumerate(params):
                p.data = shifted(p0[i])
                for n in STATE_NAMES[:opt.n_state]:
                    getattr(opt, n)[i] = shifted(np.zeros(sizes[i], np.float32))
        for s in range(3):
            for i, p in enumerate(params):
                p.grad = shifted(gs[s][i]) if unaligned else dev(gs[s][i])
            opt.step()
        if unaligned:
            assert all(p.data.data_ptr() % 16 == 4 for p in params)
        results.append([[host(p.data)] + [host(t) for t in opt_states(opt, i)] for i, p in enumerate(params)])
    for a, b in zip(*results):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    assert not np.array_equal(results[0][0][0], p0[0])


# ------------------------------------------------------------------------------------------------ what the classes share with Adam
@pytest.mark.parametrize("rule", RULES)
def test_skipped_parameters_and_strided_gradients(hip, rule):
    import torch
    rng = np.random.default_rng(2212)
    shapes = [(33, 17), (40,), (17, 33)]
    p0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    g0 = rng.standard_normal(shapes[0]).astype(np.float32)
    g2 = rng.standard_normal((33, 17)).astype(np.float32)          # handed over as its transpose: a strided (17, 33) view
    params = make_params(hip, p0)
    opt = make_opt(rule, params)
    sentinel = [0.25, 0.5]
    for k, n in enumerate(STATE_NAMES[:opt.n_state]):
        getattr(opt, n)[1].fill_(sentinel[k])
    params[0].grad = dev(g0)
    params[1].grad = None
    strided = dev(g2).t()
    assert not strided.is_contiguous()
    params[2].grad = strided
    opt.step()
    torch.cuda.synchronize()
    # no gradient: the parameter and its states are as they were
    np.testing.assert_array_equal(host(params[1].data), p0[1])
    for k, t in enumerate(opt_states(opt, 1)):
        np.testing.assert_array_equal(host(t), np.full(shapes[1], sentinel[k], np.float32))
    # the others: one step of the restatement, the strided gradient as its contiguous copy
    for i, g in ((0, g0), (2, np.ascontiguousarray(g2.T))):
        ref_p = p0[i].copy()
        ref_s = optim_ref.init_state(rule, ref_p)
        optim_ref.step(rule, ref_p, g, ref_s, 1)
        np.testing.assert_allclose(host(params[i].data), ref_p, rtol=RTOL, atol=ATOL_P)
        for k, t in enumerate(opt_states(opt, i)):
            np.testing.assert_allclose(host(t), ref_s[k], rtol=RTOL, atol=ATOL_S[k])
    assert opt.t == 1


@pytest.mark.parametrize("rule", RULES)
def test_grad_scale_and_device_divisor(hip, rule):
    """grad_scale = 0.5 and a device gradient divisor of 4: the run on gradients multiplied by 0.125 beforehand."""
    import torch
    shapes = [(37, 19), (2049,)]
    p0, gs = shape_data(shapes)
    params = make_params(hip, p0)
    opt = make_opt(rule, params)
    opt.grad_scale = 0.5
    opt.grad_divisor = torch.full((1,), 4.0, dtype=torch.float32, device="cuda")
    ref_p = [a.copy() for a in p0]
    ref_s = [optim_ref.init_state(rule, a) for a in ref_p]
    for s in range(3):
        for i, p in enumerate(params):
            p.grad = dev(gs[s][i])
            optim_ref.step(rule, ref_p[i], gs[s][i] * np.float32(0.125), ref_s[i], s + 1)
        opt.step()
        assert_matches(opt, params, ref_p, ref_s, what=f"{rule} step {s + 1}")


def test_error_messages_name_the_optimizer(hip):
    from neunet_hip.nn import Parameter
    from neunet_hip.optim import RMSprop, SGD
    with pytest.raises(ValueError, match="SGD only supports parameters on the HIP device"):
        SGD([Parameter(hip.Tensor(np.zeros(4, np.float32)))])
    p = Parameter(hip.Tensor(np.zeros(4, np.float32), device="cuda"))
    p.data = p.data.double()
    with pytest.raises(ValueError, match="RMSprop only supports float32"):
        RMSprop([p])


# ------------------------------------------------------------------------------------------------------- a training trajectory
def make_mlp(hip, g):
    import neunet_hip.nn as nn

    class MLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.l1, self.relu, self.l2 = nn.Linear(20, 16), nn.ReLU(), nn.Linear(16, 4)

        def forward(self, x):
            return self.l2(self.relu(self.l1(x)))

    model = MLP()
    for p, n in zip(model.parameters(), ("W1", "b1", "W2", "b2")):
        assert tuple(p.data.shape) == g[n].shape
        p.data.copy_(dev(g[n]))
    return model


@pytest.mark.parametrize("rule", RULES)
def test_mlp_trajectory_golden(hip, golden, rule):
    """Three training steps of the Linear - ReLU - Linear MLP against the reference's, at test_mlp_c1_trajectory_golden's tolerances
    (losses 1e-4 absolute; weights rtol 1e-4, atol 1e-5).  The model is the one whose backward launch can wait for an optimizer and
    apply ADAM in its epilogue: that must never happen for these rules."""
    import neunet_hip.nn as nn
    g = golden("mlp_optim_rules")
    model = make_mlp(hip, g)
    opt = make_opt(rule, model.parameters())
    loss_fn = nn.CrossEntropyLoss()
    for s in range(3):
        opt.zero_grad()
        loss = loss_fn(model(hip.Tensor(g["X"][s], device="cuda", requires_grad=False)),
                       hip.Tensor(g["Y"][s], dtype=np.int32, device="cuda", requires_grad=False))
        loss.backward()
        assert not getattr(opt, "_stepped_in_backward", False)
        opt.step()
        assert not getattr(opt, "_stepped_in_backward", False)
        assert abs(loss.item() - g[f"{rule}_losses"][s]) < 1e-4
    for p, n in zip(model.parameters(), ("W1", "b1", "W2", "b2")):
        np.testing.assert_allclose(host(p.data), g[f"{rule}_{n}_final"], rtol=1e-4, atol=1e-5, err_msg=n)


@pytest.mark.parametrize("rule", ["sgd", "rmsprop", "nadam"])          # one rule per state count; NAdam is bias-corrected
def test_graph_replay_equals_eager(hip, golden, rule):
    """GraphedTrainStep with the new classes: 6 replayed steps leave exactly the parameters of 6 eager steps (the step count, lr and
    the bias corrections come from device memory in the replays, from the host in the eager loop); a new opt.lr between replays
    takes effect."""
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    g = golden("mlp_optim_rules")
    rng = np.random.default_rng(2213)
    warm, steps = 2, 6
    data = [(rng.uniform(-1, 1, (8, 20)).astype(np.float32), rng.integers(0, 4, 8).astype(np.int32)) for _ in range(warm + steps + 1)]

    def make():
        model = make_mlp(hip, g)
        x = hip.Tensor(data[0][0], device="cuda", requires_grad=False)
        y = hip.Tensor(data[0][1], dtype=np.int32, device="cuda", requires_grad=False)
        loss_fn = nn.CrossEntropyLoss()

        def fb():
            loss = loss_fn(model(x), y)
            loss.backward()
            return loss

        return model, x, y, fb, make_opt(rule, model.parameters())

    def feed(x, y, item):
        x.data.copy_(dev(item[0]))
        y.data.copy_(dev(item[1]))

    m0, x0, y0, fb0, opt0 = make()

    def eager(item):
        feed(x0, y0, item)
        opt0.zero_grad()
        fb0()
        opt0.step()

    for item in data[:warm + steps]:
        eager(item)
    want = [host(p.data) for p in m0.parameters()]

    m1, x1, y1, fb1, opt1 = make()
    warm_items = iter(data[:warm])

    def fb_warm():
        item = next(warm_items, None)
        if item is not None:                                       # the eager warm-up steps read items 0 and 1
            feed(x1, y1, item)
        return fb1()

    step = GraphedTrainStep(fb_warm, opt1, GradBucket(m1.parameters()), warmup=warm)
    try:
        assert opt1.device_step
        for item in data[warm:warm + steps]:
            feed(x1, y1, item)
            step()
        for a, b in zip([host(p.data) for p in m1.parameters()], want):
            np.testing.assert_array_equal(a, b)
        assert not np.array_equal(want[0], g["W1"])
        # an LR schedule between replays
        opt0.lr = opt1.lr = opt0.lr * 0.25
        eager(data[-1])
        feed(x1, y1, data[-1])
        step()
        for p1, p0 in zip(m1.parameters(), m0.parameters()):
            np.testing.assert_array_equal(host(p1.data), host(p0.data))
    finally:
        step.release()


# ------------------------------------------------------------------------------------------------------------------ the example
def test_example_descends(hip):
    spec = importlib.util.spec_from_file_location("optimizers_example", os.path.join(ROOT, "examples", "optimizers.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    results = ex.run(ex.himmelblau, 10)
    assert sorted(results) == sorted(["Adam", "AdamW", "SGD", "Momentum", "RMSprop", "Adagrad", "Adadelta", "Adamax", "NAdam"])
    for name, (points, values) in results.items():
        assert points.shape == (11, 2) and tuple(points[0]) == ex.STARTING_POINT
        assert np.isfinite(values).all() and np.isfinite(points).all(), name
        assert values[-1] < values[0], (name, values[0], values[-1])
