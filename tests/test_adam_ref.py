"""CPU: the references of tests/test_adam_tiers_gpu.py (tests/adam_ref.py).  The float32 restatement reproduces the recorded Adam /
AdamW fixtures, and on exactly the inputs of every GPU test that compares with float64 it stays within 0.75 of the project's
tolerances of the float64 evaluation -- so a kernel held to both keeps headroom and the float64 comparison is a fair one."""
import numpy as np
import pytest

import adam_ref
from adam_ref import DECOUPLED, L2_ON_GRAD, MODES, RTOL, SCENARIO_NAMES, Trace, scenario

HEADROOM = 0.75


@pytest.mark.parametrize("name", ["adam_wd0", "adam_wd1e-2", "adamw_wd0", "adamw_wd1e-2"])
def test_step32_reproduces_the_fixtures(golden, name):
    g = golden(name)
    mode = DECOUPLED if name.startswith("adamw") else L2_ON_GRAD
    n = int(g["n_tensors"])
    p = [g[f"p0_{i}"].copy() for i in range(n)]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    for s in range(3):
        for i in range(n):
            adam_ref.step32(mode, p[i], g[f"g{s}_{i}"], m[i], v[i], s + 1, float(g["lr"]), (0.9, 0.999), 1e-8, float(g["wd"]))
            np.testing.assert_array_equal(p[i], g[f"p{s + 1}_{i}"])
            np.testing.assert_array_equal(m[i], g[f"m{s + 1}_{i}"])
            np.testing.assert_array_equal(v[i], g[f"v{s + 1}_{i}"])


def test_step32_scales_the_gradient_first():
    rng = np.random.default_rng(5)
    p0, g = rng.standard_normal(50).astype(np.float32), rng.standard_normal(50).astype(np.float32)
    for mode in MODES:
        a, b = [p0.copy(), np.zeros(50, np.float32), np.zeros(50, np.float32)], [p0.copy(), np.zeros(50, np.float32), np.zeros(50, np.float32)]
        adam_ref.step32(mode, a[0], g, a[1], a[2], 1, 1e-2, (0.9, 0.999), 1e-8, 1e-2, grad_scale=0.125)
        adam_ref.step32(mode, b[0], g * np.float32(0.125), b[1], b[2], 1, 1e-2, (0.9, 0.999), 1e-8, 1e-2)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert not np.array_equal(a[0], p0) and g.flags.writeable and np.array_equal(g, g.copy())


def test_step64_starts_from_the_rounded_hyper_parameters():
    lr, b1, b2, omb1, omb2, eps, wd, bc1, bc2, gs = adam_ref.rounded_hyper(3, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.3)
    f = np.float32
    assert lr == float(f(1e-3)) != 1e-3 and b1 == float(f(0.9)) and b2 == float(f(0.999)) and eps == float(f(1e-8)) and wd == float(f(1e-2))
    assert omb1 == float(f(1.0 - 0.9)) != 1.0 - float(f(0.9))               # 1 - beta in double first, then rounded
    assert omb2 == float(f(1.0 - 0.999))
    assert bc1 == float(f(1.0 - 0.9 ** 3)) and bc2 == float(f(1.0 - 0.999 ** 3)) and gs == float(f(0.3))
    # one element by hand
    p, m, v = np.array([0.5]), np.array([0.25]), np.array([0.125])
    adam_ref.step64(L2_ON_GRAD, p, np.array([2.0], np.float32), m, v, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.3)
    g = 2.0 * gs + wd * 0.5
    m_, v_ = b1 * 0.25 + omb1 * g, b2 * 0.125 + omb2 * g * g
    assert m[0] == m_ and v[0] == v_ and p[0] == 0.5 - lr * (m_ / bc1) / (np.sqrt(v_ / bc2) + eps)
    p, m, v = np.array([0.5]), np.array([0.25]), np.array([0.125])
    adam_ref.step64(DECOUPLED, p, np.array([2.0], np.float32), m, v, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.3)
    g, pd = 2.0 * gs, 0.5 - lr * wd * 0.5
    m_, v_ = b1 * 0.25 + omb1 * g, b2 * 0.125 + omb2 * g * g
    assert m[0] == m_ and v[0] == v_ and p[0] == pd - lr * (m_ / bc1) / (np.sqrt(v_ / bc2) + eps)


def test_plan():
    assert adam_ref.plan([1]) == (2048, 1)
    assert adam_ref.plan([2048, 2049, 0, 5]) == (2048, 4)
    assert adam_ref.plan([(1 << 22) - 1]) == (2048, 2048)
    assert adam_ref.plan([(1 << 22) - 1, 1]) == (16384, 257)
    assert adam_ref.plan([int(np.prod(s)) for s in adam_ref.TAIL_SHAPES]) == (2048, 177)
    assert adam_ref.plan([int(np.prod(s)) for s in adam_ref.LARGE_SHAPES]) == (16384, 256 + 2 + 1)


def test_worst_ratio_is_allclose():
    b = np.array([1.0, -2.0, 0.0])
    a = b + np.array([0.9, -0.9, 0.9]) * (1e-6 + 1e-5 * np.abs(b))
    assert 0.89 < adam_ref.worst_ratio(a, b, 1e-6) < 0.91
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=1e-6)
    assert adam_ref.worst_ratio(b + 1.1 * (1e-6 + 1e-5 * np.abs(b)), b, 1e-6) > 1.0


@pytest.mark.parametrize("mode", MODES, ids=["adamw", "adam"])
@pytest.mark.parametrize("name", SCENARIO_NAMES)
def test_step32_keeps_headroom_to_float64_on_the_gpu_tests_inputs(name, mode):
    sc = scenario(name, mode)
    assert len(sc.grads) <= 8                                      # beyond that float32 accumulates past the tolerances itself
    tr = Trace(sc)
    worst = [0.0, 0.0, 0.0]
    for _ in sc.grads:
        tr.step()
        worst = [max(w, r) for w, r in zip(worst, tr.ratios())]
    print(f"step32 vs step64, {name}, mode {mode}, steps {sc.t0 + 1}..{tr.t}: worst ratio p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    assert max(worst) <= HEADROOM, worst
    assert all(a.dtype == np.float32 for a in tr.p32 + tr.m32 + tr.v32)
    for i, a in enumerate(tr.p32):                                 # every tensor moved (a skipped one in its other steps)
        assert a.size == 0 or not np.array_equal(a, tr.pick(i, sc.p0[i]))
