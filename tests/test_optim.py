"""CPU: the seven optimizer rules of csrc/optim_rules.hip (SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax, NAdam; ABI 221) -- the
float32 restatement the GPU tests use (tests/optim_ref.py) against fixtures recorded from the reference (tools/gen_golden.py:
gen_optim_rules), the new exports and their argument errors (all checked before the first device call), and the classes' signatures;
the references of tests/test_optim_rules_tiers_gpu.py -- step64, the restated plan and trips, and the restatement's headroom to
float64 on that module's inputs."""
import ctypes
import inspect

import numpy as np
import pytest

import optim_ref
from optim_ref import CLASS_NAMES, N_STATE, RULES
from test_abi import lib  # noqa: F401 -- the fixture that loads (and if need be builds) the library

# test_adam_golden's tolerances (tests/test_hip_parity.py): parameters, first state, second state
RTOL, ATOL_P, ATOL_S = 1e-5, 1e-6, (1e-7, 1e-8)
RULE_ID = {r: i for i, r in enumerate(RULES)}          # include/neunet_hip.h: NNHIP_OPT_SGD ... NNHIP_OPT_NADAM


def check_against_fixture(g, s, params, states):
    for i, p in enumerate(params):
        np.testing.assert_allclose(p, g[f"p{s + 1}_{i}"], rtol=RTOL, atol=ATOL_P, err_msg=f"p step {s + 1} tensor {i}")
        for k, name in enumerate("mv"[:len(states[i])]):
            np.testing.assert_allclose(states[i][k], g[f"{name}{s + 1}_{i}"], rtol=RTOL, atol=ATOL_S[k], err_msg=f"{name} step {s + 1} tensor {i}")


@pytest.mark.parametrize("rule", RULES)
def test_restatement_reproduces_the_reference(golden, rule):
    g = golden(f"optim_{rule}")
    n = int(g["n_tensors"])
    assert int(g["n_state"]) == N_STATE[rule]
    assert float(g["lr"]) == optim_ref.DEFAULTS[rule]["lr"]
    params = [g[f"p0_{i}"].copy() for i in range(n)]
    states = [optim_ref.init_state(rule, p) for p in params]
    for s in range(3):
        for i in range(n):
            optim_ref.step(rule, params[i], g[f"g{s}_{i}"], states[i], s + 1)
        check_against_fixture(g, s, params, states)


def test_mlp_fixture_layout(golden):
    g = golden("mlp_optim_rules")
    assert g["X"].shape == (3, 8, 20) and g["Y"].shape == (3, 8) and g["W1"].shape == (16, 20) and g["W2"].shape == (4, 16)
    for rule in RULES:
        assert g[f"{rule}_losses"].shape == (3,) and np.isfinite(g[f"{rule}_losses"]).all()
        for n in ("W1", "b1", "W2", "b2"):
            assert g[f"{rule}_{n}_final"].shape == g[n].shape and not np.array_equal(g[f"{rule}_{n}_final"], g[n])
    # the same first batch and initial weights under every rule: the same first loss
    assert len({float(g[f"{rule}_losses"][0]) for rule in RULES}) == 1


def test_version_is_221(lib):
    from neunet_hip import _lib
    assert _lib.load_hip_function("nnhipVersion")() >= 221


def test_new_exports_bind(lib):
    from neunet_hip import _lib
    for name in ("nnhipOptimizerRuleStep", "nnhipOptimizerRuleMultiTensorStep"):
        assert hasattr(lib, name)
        f = _lib.load_hip_function(name)
        assert f.restype is ctypes.c_int
    assert len(_lib._SIGNATURES["nnhipOptimizerRuleStep"][1]) == 13
    assert len(_lib._SIGNATURES["nnhipOptimizerRuleMultiTensorStep"][1]) == 15


def test_rule_ids_match_header():
    import re
    from test_abi import HEADER
    from neunet_hip import optim
    text = open(HEADER).read()
    for rule in RULES:
        value = int(re.search(r"NNHIP_OPT_%s\s*=\s*(\d+)" % rule.upper(), text).group(1))
        assert value == RULE_ID[rule] == getattr(optim, CLASS_NAMES[rule]).rule
        assert getattr(optim, CLASS_NAMES[rule]).n_state == N_STATE[rule]


def test_per_tensor_argument_errors(lib):
    """Every check precedes the first device call: the pointers here are never dereferenced."""
    from neunet_hip._lib import NeunetHipError, call_hip_function
    D = 0x1000                                                  # non-null, 16-byte aligned, never dereferenced

    def call(rule, p=D, g=D, s1=D, s2=D, n=16, step=1):
        return call_hip_function("nnhipOptimizerRuleStep", rule, p, g, s1, s2, n, 0.01, 0.9, 0.999, 1e-8, step, 1.0, None)

    for bad in (-1, 7, 100):
        with pytest.raises(NeunetHipError, match="unknown rule"):
            call(bad)
    for rule in RULES:
        r = RULE_ID[rule]
        with pytest.raises(NeunetHipError, match="negative size"):
            call(r, n=-1)
        for step in (0, -3):
            with pytest.raises(NeunetHipError, match="step >= 1"):
                call(r, step=step)
        if N_STATE[rule] >= 1:
            with pytest.raises(NeunetHipError, match="null state pointer"):
                call(r, s1=None)
        if N_STATE[rule] >= 2:
            with pytest.raises(NeunetHipError, match="null state pointer"):
                call(r, s2=None)
        with pytest.raises(NeunetHipError, match="null pointer"):
            call(r, p=None)
        assert call(r, p=None, g=None, s1=None, s2=None, n=0) == 0          # nothing to do: no launch, no pointer needed


def test_multi_tensor_argument_errors(lib):
    from ctypes import POINTER, c_int64, c_void_p, cast
    from neunet_hip._lib import NeunetHipError, call_hip_function, load_hip_function
    opt = load_hip_function("nnhipCreateFusedOptimizer")()
    assert opt
    D = 0x1000
    tab = cast((c_void_p * 2)(D, D), POINTER(c_void_p))
    sizes = cast((c_int64 * 2)(16, 5), POINTER(c_int64))
    neg = cast((c_int64 * 2)(16, -5), POINTER(c_int64))

    def call(rule, handle=opt, n=2, p=tab, g=tab, s1=tab, s2=tab, sz=sizes, step=1):
        return call_hip_function("nnhipOptimizerRuleMultiTensorStep", handle, rule, n, p, g, s1, s2, sz, 0.01, 0.9, 0.999, 1e-8, step,
                                 1.0, None)

    try:
        with pytest.raises(NeunetHipError, match="null optimizer handle"):
            call(0, handle=None)
        for bad in (-1, 7):
            with pytest.raises(NeunetHipError, match="unknown rule"):
                call(bad)
        for rule in RULES:
            r = RULE_ID[rule]
            with pytest.raises(NeunetHipError, match="negative size"):
                call(r, sz=neg)
            with pytest.raises(NeunetHipError, match="SetStep"):          # device-driven stepping was never set up on this handle
                call(r, step=0)
            with pytest.raises(NeunetHipError, match="bad n_tensors/step"):
                call(r, step=-1)
            with pytest.raises(NeunetHipError, match="bad n_tensors/step"):
                call(r, n=-1)
            if N_STATE[rule] >= 1:
                with pytest.raises(NeunetHipError, match="null state table"):
                    call(r, s1=None)
            if N_STATE[rule] >= 2:
                with pytest.raises(NeunetHipError, match="null state table"):
                    call(r, s2=None)
            with pytest.raises(NeunetHipError, match="null table"):
                call(r, p=None)
            assert call(r, n=0, p=None, g=None, s1=None, s2=None, sz=None) == 0
    finally:
        load_hip_function("nnhipDestroyFusedOptimizer")(opt)


def test_rule_device_stepping_needs_a_prepared_handle(lib):
    """nnhipOptimizerRuleMultiTensorStep with step == 0 on a handle that never saw SetStep / SetHyper: the message names the entry and
    comes before the plan is built -- sizes the plan builder refuses do not change it -- so no device call precedes it."""
    from ctypes import POINTER, c_int64, c_void_p, cast
    from neunet_hip._lib import NeunetHipError, call_hip_function, load_hip_function
    opt = load_hip_function("nnhipCreateFusedOptimizer")()
    assert opt
    tab = cast((c_void_p * 2)(0x1000, 0x1000), POINTER(c_void_p))
    try:
        for sizes in ((16, 5), (1 << 62, 5)):
            sz = cast((c_int64 * 2)(*sizes), POINTER(c_int64))
            for rule in RULES:
                with pytest.raises(NeunetHipError, match="nnhipOptimizerRuleMultiTensorStep: step == 0 needs nnhipFusedOptimizerSetStep and SetHyper first"):
                    call_hip_function("nnhipOptimizerRuleMultiTensorStep", opt, RULE_ID[rule], 2, tab, tab, tab, tab, sz, 0.01, 0.9, 0.999,
                                      1e-8, 0, 1.0, None)
        with pytest.raises(NeunetHipError, match="nnhipOptimizerRuleMultiTensorStep: too many chunks"):
            call_hip_function("nnhipOptimizerRuleMultiTensorStep", opt, 0, 2, tab, tab, None, None, sz, 0.01, 0.0, 0.0, 0.0, 1, 1.0, None)
    finally:
        load_hip_function("nnhipDestroyFusedOptimizer")(opt)


def test_adam_device_stepping_needs_a_prepared_handle(lib):
    """nnhipFusedAdamWMultiTensorStep with step == 0 (device-side stepping) on a handle that never saw nnhipFusedOptimizerSetStep /
    SetHyper: the documented error, raised with the other argument checks -- before the plan is built and uploaded, so no device call
    precedes it and the pointers are never dereferenced."""
    from ctypes import POINTER, c_int64, c_void_p, cast
    from neunet_hip._lib import NeunetHipError, call_hip_function, load_hip_function
    opt = load_hip_function("nnhipCreateFusedOptimizer")()
    assert opt
    tab = cast((c_void_p * 2)(0x1000, 0x1000), POINTER(c_void_p))
    sizes = cast((c_int64 * 2)(16, 5), POINTER(c_int64))
    try:
        for mode in (0, 1):
            with pytest.raises(NeunetHipError, match="step == 0 needs nnhipFusedOptimizerSetStep and SetHyper first"):
                call_hip_function("nnhipFusedAdamWMultiTensorStep", opt, 2, tab, tab, tab, tab, sizes, 0.01, 0.9, 0.999, 1e-8, 0.01, 0,
                                  mode, 1.0, None)
        with pytest.raises(NeunetHipError, match="bad n_tensors/step"):
            call_hip_function("nnhipFusedAdamWMultiTensorStep", opt, 2, tab, tab, tab, tab, sizes, 0.01, 0.9, 0.999, 1e-8, 0.01, -1, 0, 1.0,
                              None)
    finally:
        load_hip_function("nnhipDestroyFusedOptimizer")(opt)


# ------------------------------------------------------------------- the references of tests/test_optim_rules_tiers_gpu.py
HEADROOM = 0.75


def test_step64_starts_from_the_rounded_hyper_parameters():
    f = np.float32
    h = optim_ref.rounded_hyper("nadam", 3, 0.3, lr=1e-3)
    assert h["lr"] == float(f(1e-3)) != 1e-3 and h["c1"] == float(f(0.9)) and h["c2"] == float(f(0.999)) and h["eps"] == float(f(1e-8))
    assert h["omc1"] == float(f(1.0 - 0.9)) != 1.0 - float(f(0.9))          # 1 - beta in double first, then rounded
    assert h["bc1"] == float(f(1.0 - 0.9 ** 3)) and h["bc2"] == float(f(1.0 - 0.999 ** 3)) and h["gs"] == float(f(0.3))
    assert optim_ref.rounded_hyper("rmsprop", 1, alpha=0.5)["c1"] == 0.5 and optim_ref.rounded_hyper("adadelta", 1)["eps"] == float(f(1e-6))
    # one element by hand, per rule
    g32, gs = np.array([2.0], np.float32), h["gs"]
    g = 2.0 * gs
    for rule in RULES:
        hr = optim_ref.rounded_hyper(rule, 3, 0.3)
        lr, c1, c2, o1, o2, eps, bc1, bc2 = (hr[k] for k in ("lr", "c1", "c2", "omc1", "omc2", "eps", "bc1", "bc2"))
        p, st = np.array([0.5]), [np.array([0.25]), np.array([0.125])][:N_STATE[rule]]
        optim_ref.step64(rule, p, g32, st, 3, grad_scale=0.3)
        if rule == "sgd":
            want = (0.5 - lr * g,)
        elif rule == "momentum":
            m = c1 * 0.25 + o1 * g
            want = (0.5 - m * lr, m)
        elif rule == "rmsprop":
            m = c1 * 0.25 + o1 * (g * g)
            want = (0.5 - lr * g / (np.sqrt(m) + eps), m)
        elif rule == "adagrad":
            m = 0.25 + g * g
            want = (0.5 - lr * g / (np.sqrt(m) + eps), m)
        elif rule == "adadelta":
            m = c1 * 0.25 + o1 * (g * g)
            dx = -(np.sqrt(0.125 + eps) / np.sqrt(m + eps)) * g
            want = (0.5 + dx, m, c1 * 0.125 + o1 * (dx * dx))
        elif rule == "adamax":
            m, v = c1 * 0.25 + o1 * g, max(c2 * 0.125, abs(g))
            want = (0.5 - lr * (m / bc1) / (v + eps), m, v)
        else:
            m, v = c1 * 0.25 + o1 * g, c2 * 0.125 + o2 * (g * g)
            want = (0.5 - lr * (m / bc1 + o1 * g / bc1) / (np.sqrt(v / bc2) + eps), m, v)
        assert (p[0],) + tuple(s[0] for s in st) == want, rule


def test_trips_cover_every_element_exactly_once():
    """rule_span restated: over all threads of a grid the trips touch each of n elements once, for both unrolls, at sizes around
    every loop level's threshold; and the counts trips() returns are those of the elements."""
    stride = 8
    for U in (2, 4):
        for n in list(range(0, 4 * stride * (2 * U + 1) + 4)) + [4 * stride * 3 * U + 3]:
            seen = []
            for first in range(stride):
                el = optim_ref.span_elements(n, first, stride, U)
                a, b, c, tail = optim_ref.trips(n, first, stride, U)
                assert len(el) == 4 * (U * a + 2 * b + c) + tail and (U > 2 or b == 0) and c <= 1 and b <= 1 and tail <= 1
                seen += el
            assert sorted(seen) == list(range(n)), (U, n)
    # the loop levels by name: 7 float4 for one thread of 1 are 4 + 2 + 1 under U = 4 and 2 + 2 + 2 + 1 under U = 2
    assert optim_ref.trips(4 * 7 + 1, 0, 1, 4) == (1, 1, 1, 1) and optim_ref.trips(4 * 7 + 1, 0, 1, 2) == (3, 0, 1, 1)
    assert optim_ref.trips(3, 0, 256, 4) == (0, 0, 0, 1) and optim_ref.trips(3, 3, 256, 4) == (0, 0, 0, 0)
    assert optim_ref.UNROLL == {0: 4, 1: 2, 2: 2}                                     # csrc/optim_rules.hip: RULE_UNR0 / 1 / 2


def test_plan_and_grid_restated():
    """The chunk counts and strides the GPU module asserts."""
    sz = lambda shapes: [int(np.prod(s)) for s in shapes]  # noqa: E731
    assert optim_ref.plan([1]) == (2048, 1) and optim_ref.plan([2048, 2049, 0, 5]) == (2048, 4)
    assert optim_ref.plan([(1 << 22) - 1]) == (2048, 2048) and optim_ref.plan([(1 << 22) - 1, 1]) == (16384, 257)
    assert optim_ref.plan(sz(optim_ref.TAIL_SHAPES)) == (2048, 9 + 2 + 3 + 163)
    assert sum(sz(optim_ref.LARGE_SHAPES)) >= 1 << 22 and optim_ref.plan(sz(optim_ref.LARGE_SHAPES)) == (16384, 257 + 2 + 1)
    assert optim_ref.chunks(sz(optim_ref.LARGE_SHAPES)[0], 16384)[-2:] == [16384, optim_ref.LARGE_LAST]
    assert optim_ref.plan(sz(optim_ref.ZERO_MID_SHAPES)) == (2048, 3) and optim_ref.plan(sz(optim_ref.DEV_SHAPES)) == (2048, 4)
    assert optim_ref.plan(sz(optim_ref.DEV_SHAPES[1:])) == (2048, 2)
    assert [optim_ref.plan_bytes(r, [300, 0, 2049]) for r in ("sgd", "rmsprop", "nadam")] == [48 + 24 + 24, 72 + 24 + 24, 96 + 24 + 24]
    # the per-tensor launch: one thread per float4 and one block for the tail, capped
    assert optim_ref.per_tensor_grid(1, True) == 256 and optim_ref.per_tensor_grid(1027, True) == 512
    assert optim_ref.per_tensor_grid(4 * 256 * 2048, True) == 2048 * 256 == optim_ref.STRIDE4
    assert all(optim_ref.per_tensor_grid(n, True) == optim_ref.STRIDE4 and n % 4 == 3 for n in optim_ref.PT_N.values())
    assert optim_ref.per_tensor_grid(optim_ref.PT_SCALAR_N, False) == optim_ref.STRIDE4
    assert optim_ref.per_tensor_grid(300, False) == 512


@pytest.mark.parametrize("name", optim_ref.SCENARIO_NAMES)
def test_step_keeps_headroom_to_float64_on_the_gpu_tests_inputs(name):
    """On exactly the inputs and step counts of the GPU tests that compare with float64, the float32 restatement stays within 0.75
    of the tolerances of step64: a kernel held to both keeps headroom, and the float64 comparison is a fair one."""
    sc = optim_ref.scenario(name)
    assert len(sc.grads) <= 8
    assert optim_ref.rules_of(name)
    for rule in optim_ref.rules_of(name):
        tr = optim_ref.Trace(rule, sc)
        worst = [0.0] * (1 + N_STATE[rule])
        for _ in sc.grads:
            tr.step()
            worst = [max(w, r) for w, r in zip(worst, tr.ratios(RTOL, ATOL_P, ATOL_S))]
        print(f"step vs step64, {name}, {rule}, steps {sc.t0 + 1}..{tr.t}: worst ratio " + " ".join(f"{x:.3f}" for x in worst))
        assert max(worst) <= HEADROOM, (rule, worst)
        assert all(a.dtype == np.float32 for a in tr.p32 + [s for st in tr.s32 for s in st])
        for i, a in enumerate(tr.p32):                             # every tensor moved (a skipped one in its other steps)
            assert a.size == 0 or not np.array_equal(a, tr.pick(i, sc.p0[i])), (rule, i)


# The reference's constructors (neunet/optim.py:76-244): parameter names and defaults, in order.
REFERENCE_SIGNATURES = {
    "SGD": [("params", inspect.Parameter.empty), ("lr", 0.01)],
    "Momentum": [("params", inspect.Parameter.empty), ("lr", 0.01), ("momentum", 0.9)],
    "RMSprop": [("params", inspect.Parameter.empty), ("lr", 0.01), ("alpha", 0.99), ("eps", 1e-8)],
    "Adagrad": [("params", inspect.Parameter.empty), ("lr", 0.01), ("eps", 1e-8)],
    "Adadelta": [("params", inspect.Parameter.empty), ("lr", 1.0), ("rho", 0.9), ("eps", 1e-6)],
    "Adamax": [("params", inspect.Parameter.empty), ("lr", 0.002), ("betas", (0.9, 0.999)), ("eps", 1e-8)],
    "NAdam": [("params", inspect.Parameter.empty), ("lr", 0.002), ("betas", (0.9, 0.999)), ("eps", 1e-8)],
}


@pytest.mark.parametrize("name", sorted(REFERENCE_SIGNATURES))
def test_class_signatures_equal_the_reference(name):
    from neunet_hip import optim
    cls = getattr(optim, name)
    sig = inspect.signature(cls)
    assert [(p.name, p.default) for p in sig.parameters.values()] == REFERENCE_SIGNATURES[name]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    for method in ("step", "zero_grad", "use_device_step", "sync_device_hyper"):
        assert callable(getattr(cls, method))
    # never part of the optimizer-in-backward path
    assert cls.can_fuse_into_backward(object.__new__(cls)) is False
    assert cls.pending_update_args(object.__new__(cls), [], 1) is None
    assert not hasattr(cls, "fuse_backward") and not hasattr(cls, "take_pending_backward")


def test_defaults_table_matches_signatures():
    for rule in RULES:
        want = dict(REFERENCE_SIGNATURES[CLASS_NAMES[rule]][1:])
        assert optim_ref.DEFAULTS[rule] == want
