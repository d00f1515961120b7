"""GPU: SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax and NAdam of csrc/optim_rules.hip on every kernel path -- rule_span's U-round,
2-round and single-round loops and its scalar tail under both chunk plans of the multi-tensor entry and beyond the grid cap of the
per-tensor entry (nnhipOptimizerRuleStep); the scalar path beyond its own cap; one arithmetic in four inlining sites, bit for bit;
special values; the 2-, 3- and 4-table plan blobs with an empty tensor, NULL unused state tables and every refusal; device-side
stepping (csrc/adam_device.h) driven directly -- resumed at a step, betas / coefficients / block count / hyper-parameters changed
between launches -- and captured; the plan re-uploaded at every step.

Every test checks p and every state stream the rule has.  References (tests/optim_ref.py): `step`, the reference's float32 arithmetic,
and `step64`, the float64 value of what the kernel is asked to compute; tolerances tests/test_optim_gpu.py's (rtol 1e-5; atol 1e-6 p,
1e-7 first state, 1e-8 second state).  Float64 comparisons run for at most 6 steps on standard-normal data (tests/test_optim.py holds
`step` itself to 0.75 of the tolerances on exactly those inputs); longer runs compare device with device, bit for bit.  Every size
aimed at a loop level asserts through optim_ref.trips / plan that it reaches it.

Measured on an MI355X, worst |kernel - step64| / (atol + rtol |step64|) over all float64 comparisons below (every test prints its own,
the module its maximum):
    p 0.032 (RMSprop, third step of the small-chunk matrix)   m 0.317 (Adamax, step 99995 of the resumed run)   v 0.030 (NAdam, step 99995)
`step` against `step64` on the same inputs (tests/test_optim.py): p 0.032, m 0.317, v 0.030 -- the kernels are as close to float64 as
the reference's own float32 arithmetic is, with no sign of contraction or of a non-IEEE division or square root.

Groups: 1 small-chunk plan, 2 large-chunk plan, 3 per-tensor entry (vector and scalar path beyond the grid cap), 4 same bits in four
sites, 5 special values, 6 table edges and refusals, 7 device-side stepping, 8 capture, 9 plan churn.  Each deliberate one-line break
of the library below was tried on a scratch copy, and these groups were seen to fail:
    the scalar tail starts one element late                 1, 2, 3 (vector path), 4, 6, 7, 9
    the U-round loop advances by U - 1 strides              1 (not SGD: 2048-element chunks never reach its 4-round loop), 2, 3 (the
                                                            long sizes), 4, 6, 7, 9
    the 2-round fallback removed (`if constexpr (false)`)   none, and no result can show it: the single-round loop then takes the
                                                            same float4 with the same arithmetic, only with fewer loads in flight.
                                                            The trips assertions state which sizes are aimed at that loop
    Adamax's maximum replaced by fmaxf                      5 (both Adamax tests)
    `#pragma clang fp contract(off)` removed from rule1     4 (Momentum, RMSprop, Adadelta, Adamax, NAdam; SGD and Adagrad keep their
                                                            bits: the compiler contracts them alike in every site)
    `cached` forced true in adam_dev_resolve                7 (Adamax, NAdam), 8 (Adamax)
    a plan re-sent only when its byte size changes          1, 2, 4, 5, 6, 7, 8, 9 (every test that hands a handle new buffers)"""
import numpy as np
import pytest

import optim_ref
from optim_ref import BETA_RULES, CLASS_NAMES, COEF_NAME, N_STATE, RULES, Trace, scenario, unroll
from test_optim import RULE_ID
from test_optim_gpu import ATOL_P, ATOL_S, RTOL, make_mlp

pytestmark = pytest.mark.gpu
by_rule = pytest.mark.parametrize("rule", RULES)
STATE_NAMES = "mv"
STREAMS = ("p", "m", "v")
ATOL = (ATOL_P,) + tuple(ATOL_S)
SENTINEL = np.float32(-7.25)
GUARD = 8
_worst = {}                                                         # stream -> (ratio, where), over the module's float64 comparisons


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    yield neunet_hip
    print("\nworst kernel vs step64 over the module: " + "; ".join(f"{k} {r:.3f} ({w})" for k, (r, w) in sorted(_worst.items())))


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                 # a copy: the shared test data stays read-only


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sizes_of(shapes):
    return [int(np.prod(s)) for s in shapes]


def make_params(hip, arrays):
    from neunet_hip.nn import Parameter
    return [Parameter(hip.Tensor(a, device="cuda")) for a in arrays]


def opt_states(opt, i):
    return [getattr(opt, n)[i] for n in STATE_NAMES[:opt.n_state]]


def make_opt(hip, rule, sc, **kw):
    """(optimizer, parameters) on a scenario's initial values, states and step count; the rule's default hyper-parameters."""
    from neunet_hip import optim
    params = make_params(hip, sc.p0)
    opt = getattr(optim, CLASS_NAMES[rule])(params, **kw)
    assert opt.n_state == N_STATE[rule] and opt.rule == RULE_ID[rule]
    if sc.m0 is not None:
        for i in range(len(params)):
            for k, src in enumerate((sc.m0, sc.v0)[:opt.n_state]):
                opt_states(opt, i)[k].copy_(dev(src[i]))
    opt.t = sc.t0
    return opt, params


def apply_over(opt, rule, over):
    """A scenario step's hyper-parameters, assigned as a training loop would."""
    h = dict(optim_ref.DEFAULTS[rule], **optim_ref.hyper_of(rule, over))
    opt.grad_scale = h.pop("grad_scale", 1.0)
    for k, v in h.items():
        assert hasattr(opt, k)
        setattr(opt, k, v)


def feed(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else dev(g)


def snapshot(opt, params):
    return [[host(p.data)] + [host(t) for t in opt_states(opt, i)] for i, p in enumerate(params)]


def assert_same_bits(a, b, what=""):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for k in range(len(x)):
            np.testing.assert_array_equal(bits(x[k]), bits(y[k]), err_msg=f"{what} {STREAMS[k]}[{i}]")


def assert_moved(snap, p0):
    for i, x in enumerate(snap):
        if x[0].size:
            assert not np.array_equal(x[0].reshape(-1), np.asarray(p0[i]).reshape(-1)), f"p[{i}] did not move"
            assert all(np.any(s != 0) for s in x[1:]), f"a state of tensor {i} is still zero"


def check(tr, snap, what):
    """Device p and states against both references at the tolerances above; prints the worst ratio to float64 per stream."""
    ns = N_STATE[tr.rule]
    worst = [0.0] * (1 + ns)
    for i, x in enumerate(snap):
        assert len(x) == 1 + ns
        for k, r64 in enumerate([tr.p64[i]] + tr.s64[i]):
            worst[k] = max(worst[k], optim_ref.worst_ratio(tr.pick(i, x[k]), r64, ATOL[k], RTOL))
    print(f"kernel vs step64, {what}: worst ratio " + " ".join(f"{STREAMS[k]} {w:.3f}" for k, w in enumerate(worst)))
    for k, w in enumerate(worst):
        if w > _worst.get(STREAMS[k], (-1.0, ""))[0]:
            _worst[STREAMS[k]] = (w, what)
    for i, x in enumerate(snap):
        for k, (r32, r64) in enumerate(zip([tr.p32[i]] + tr.s32[i], [tr.p64[i]] + tr.s64[i])):
            got = tr.pick(i, x[k])
            np.testing.assert_allclose(got, r32, rtol=RTOL, atol=ATOL[k], err_msg=f"{what}: {STREAMS[k]}[{i}] vs step")
            np.testing.assert_allclose(got, r64, rtol=RTOL, atol=ATOL[k], err_msg=f"{what}: {STREAMS[k]}[{i}] vs step64")


def run_scenario(hip, rule, name):
    """The scenario through the class (the multi-tensor entry), checked after every step."""
    sc = scenario(name)
    assert rule in optim_ref.rules_of(name)
    opt, params = make_opt(hip, rule, sc)
    tr = Trace(rule, sc)
    for grads, over in zip(sc.grads, sc.over):
        apply_over(opt, rule, over)
        feed(params, grads)
        opt.step()
        tr.step()
        check(tr, snapshot(opt, params), f"{name} {rule} step {tr.t}")
    assert opt.t == tr.t
    return sc, opt, params


# ------------------------------------------------------------------------------------------ 1, 2: the multi-tensor entry's two plans
@by_rule
def test_tail_and_round_matrix_small_chunks(hip, rule):
    """2048-element chunks, one block of 256 threads each: a thread owns at most two float4.  Whole chunk: every thread one 2-round
    trip (SGD: its 2-round fallback, never the 4-round loop).  1500 elements (375 float4): threads 0-118 a 2-round trip, 119-255 a
    single round.  1027: 256 float4, single rounds, threads 0-2 the tail.  1, 3: the tail alone; 4: one float4; 5: one float4 and a
    tail element; 2049 / 4099: one / three elements in a last chunk."""
    sizes = sizes_of(optim_ref.TAIL_SHAPES)
    assert sizes[:11] == [1, 3, 4, 5, 1023, 1027, 1500, 2047, 2048, 2049, 4099] and sum(sizes) < 1 << 22
    assert optim_ref.plan(sizes) == (2048, 9 + 2 + 3 + 163)
    U = unroll(rule)
    two = (1, 0, 0, 0) if U == 2 else (0, 1, 0, 0)
    assert optim_ref.trip_classes(2048, 256, U) == {two: 256}
    assert optim_ref.trip_classes(1500, 256, U) == {two: 119, (0, 0, 1, 0): 137}
    assert optim_ref.trip_classes(1027, 256, U) == {(0, 0, 1, 1): 3, (0, 0, 1, 0): 253}
    assert optim_ref.trip_classes(3, 256, U) == {(0, 0, 0, 1): 3, (0, 0, 0, 0): 253}
    assert optim_ref.trip_classes(5, 256, U) == {(0, 0, 1, 1): 1, (0, 0, 0, 0): 255}
    assert optim_ref.chunks(4099, 2048) == [2048, 2048, 3]
    _, opt, params = run_scenario(hip, rule, "tail")
    assert_moved(snapshot(opt, params), scenario("tail").p0)


@by_rule
def test_large_chunk_plan(hip, rule):
    """16384-element chunks (>= 2^22 elements in all): 16 float4 per thread in a whole chunk -- SGD four 4-round trips, the others
    eight 2-round trips.  The long tensor ends in a chunk of 4 * (7 * 256 + 100) + 3 elements, 1892 float4: threads 100-255 own
    seven -- SGD a 4-round trip, a 2-round trip and a single round, the others three 2-round trips and a single round --, threads
    0-99 eight (SGD two 4-round trips, the others four 2-round trips), threads 0-2 a tail element.  The 16385-element tensor ends in
    a chunk of one element.  The long tensor is compared on its first and last chunk whole, 8 elements beyond each, and every 1021st
    element between; the small tensors in full."""
    sizes = sizes_of(optim_ref.LARGE_SHAPES)
    assert sum(sizes) >= 1 << 22 and optim_ref.plan(sizes) == (16384, 257 + 2 + 1)
    last = optim_ref.chunks(sizes[0], 16384)[-1]
    assert last == optim_ref.LARGE_LAST == 4 * (7 * 256 + 100) + 3
    if unroll(rule) == 4:
        assert optim_ref.trip_classes(16384, 256, 4) == {(4, 0, 0, 0): 256}
        assert optim_ref.trip_classes(last, 256, 4) == {(2, 0, 0, 1): 3, (2, 0, 0, 0): 97, (1, 1, 1, 0): 156}
    else:
        assert optim_ref.trip_classes(16384, 256, 2) == {(8, 0, 0, 0): 256}
        assert optim_ref.trip_classes(last, 256, 2) == {(4, 0, 0, 1): 3, (4, 0, 0, 0): 97, (3, 0, 1, 0): 156}
    sc = scenario("large")
    idx = sc.idx[0]
    assert idx[16384 + 7] == 16384 + 7 and idx[-(16384 + 8)] == sizes[0] - 16384 - 8 and sizes[0] - last - 8 in idx and sc.idx[1] is None
    run_scenario(hip, rule, "large")


# ------------------------------------------------------------------------------------------------------ 3: the per-tensor entry
def guarded(a, shift=0):
    """(buffer, view): a device copy of `a` with GUARD sentinel floats before and at least as many after it; shift = 1: the view
    starts one float off a 16-byte boundary."""
    import torch
    a = np.asarray(a, np.float32).reshape(-1)
    buf = torch.full((a.size + 2 * GUARD + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
    view = buf[GUARD + shift:GUARD + shift + a.size]
    view.copy_(dev(a))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
    return buf, view


def assert_guards(pairs, what=""):
    for buf, view in pairs:
        off, h = (view.data_ptr() - buf.data_ptr()) // 4, host(buf)
        assert off >= GUARD and h.size - off - view.numel() >= GUARD
        np.testing.assert_array_equal(h[:off], SENTINEL, err_msg=f"{what}: guard before")
        np.testing.assert_array_equal(h[off + view.numel():], SENTINEL, err_msg=f"{what}: guard after")


def per_tensor_call(rule, p, g, states, n, t, grad_scale=1.0, **hyper):
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    c1, c2, eps = optim_ref.coefficients(rule, hyper)
    lr = dict(optim_ref.DEFAULTS[rule], **hyper)["lr"]
    s1 = states[0] if len(states) >= 1 else None                   # state pointers the rule does not have: NULL
    s2 = states[1] if len(states) >= 2 else None
    return call_hip_function("nnhipOptimizerRuleStep", RULE_ID[rule], p, g, s1, s2, n, lr, c1, c2, eps, t, grad_scale,
                             get_current_stream_ptr())


def run_per_tensor(rule, name, shift):
    sc = scenario(name)
    tr = Trace(rule, sc)
    ps = [guarded(a, shift) for a in sc.p0]
    ss = [[guarded(np.zeros(a.size, np.float32), shift) for _ in range(N_STATE[rule])] for a in sc.p0]
    for grads in sc.grads:
        gd = [guarded(g, shift) for g in grads]
        for i, (p, g) in enumerate(zip(ps, gd)):
            per_tensor_call(rule, p[1], g[1], [s[1] for s in ss[i]], p[1].numel(), tr.t + 1)
        tr.step()
        check(tr, [[host(p[1])] + [host(s[1]) for s in ss[i]] for i, p in enumerate(ps)], f"{name} {rule} per-tensor step {tr.t}")
        assert_guards(ps + [s for st in ss for s in st], f"{name} {rule} step {tr.t}")
        for (_, view), g in zip(gd, grads):                        # the gradient is read only
            np.testing.assert_array_equal(host(view), g.reshape(-1))
    return sc


PT_CASES = [(r, n) for r in RULES for n in ("pt_small",) + tuple(f"pt_{k}" for k in optim_ref.PT_STRIDES[N_STATE[r]])]
# (unroll, strides): the trips of threads 0-299 and of the others
PT_TRIPS = {(2, 2): ((1, 0, 1), (1, 0, 0)), (2, 3): ((2, 0, 0), (1, 0, 1)), (4, 3): ((1, 0, 0), (0, 1, 1)), (4, 5): ((1, 1, 0), (1, 0, 1))}


@pytest.mark.parametrize("rule,name", PT_CASES, ids=[f"{r}-{n}" for r, n in PT_CASES])
def test_per_tensor_entry_beyond_the_grid_cap(hip, rule, name):
    """nnhipOptimizerRuleStep caps its grid at 2048 blocks: a stride of s = 524 288 float4.  n >> 2 = k s + 300, n % 4 == 3.
    Two-round rules: k = 2, threads 0-299 a 2-round trip and a single round, the others a 2-round trip; k = 3, threads 0-299 two
    2-round trips, the others one and a single round.  SGD: k = 3, threads 0-299 a 4-round trip, the others a 2-round trip and a
    single round; k = 5, threads 0-299 a 4-round and a 2-round trip, the others a 4-round trip and a single round.  Threads 0-2 take
    the tail.  pt_small: n = 1, 3, 4, 1027 (grids of 1, 1, 1 and 2 blocks).  The long tensor is compared on 16 K elements at both
    ends and every 1021st between; guard words around p and every state stay intact."""
    sc = scenario(name)
    if name != "pt_small":
        k, n, U = int(name[3:]), sc.shapes[0][0], unroll(rule)
        s = optim_ref.per_tensor_grid(n, True)
        assert s == 2048 * 256 and n % 4 == 3 and n >> 2 == k * s + 300
        low, high = PT_TRIPS[U, k]
        assert {optim_ref.trips(n, f, s, U) for f in (0, 1, 2)} == {low + (1,)}
        assert {optim_ref.trips(n, f, s, U) for f in (3, 150, 299)} == {low + (0,)}
        assert {optim_ref.trips(n, f, s, U) for f in (300, 301, s // 2, s - 1)} == {high + (0,)}
        assert sc.idx[0][16383] == 16383 and sc.idx[0][-16384] == n - 16384 and sc.idx[0].size > 2 * 16384 + n // 1021 - 40
    else:
        assert sizes_of(sc.shapes) == [1, 3, 4, 1027]
        assert [optim_ref.per_tensor_grid(n, True) for n in (1, 3, 4, 1027)] == [256, 256, 256, 512]
    run_per_tensor(rule, name, shift=0)


@by_rule
def test_per_tensor_scalar_path_beyond_its_grid_cap(hip, rule):
    """Everything one float off a 16-byte boundary: one element per thread and round, the grid capped at 2048 x 256 threads.
    n = 2 * 524288 + 300: threads 0-299 take three elements, the others two.  Then n = 1, 3, 4, 1027 the same way."""
    n = scenario("pt_scalar").shapes[0][0]
    s = optim_ref.per_tensor_grid(n, False)
    assert s == 2048 * 256 and n == 2 * s + 300
    assert len(range(299, n, s)) == 3 and len(range(300, n, s)) == 2
    run_per_tensor(rule, "pt_scalar", shift=1)
    run_per_tensor(rule, "pt_small", shift=1)


# ------------------------------------------------------------------------------------------- 4: one arithmetic, four sites, same bits
def shifted(a):
    """A contiguous device copy that starts one float into its buffer: 4-byte alignment only."""
    import torch
    a = np.asarray(a)
    buf = torch.zeros(a.size + 5, dtype=torch.float32, device="cuda")
    view = buf[1:1 + a.size]
    view.copy_(dev(a.reshape(-1)))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@by_rule
def test_vector_and_scalar_paths_of_both_entries_give_the_same_bits(hip, rule):
    """rule1 is inlined into the vector rounds, the tail and the scalar loop of two kernels (fp contract(off)).  Baseline: the
    multi-tensor entry with everything 16-byte aligned.  The same bits in p and the states: the multi-tensor entry with p, g and all
    states one float into their buffers, with ONLY the gradient so, with ONLY one state so (each in turn: the vector path must be
    refused for the whole tensor); the per-tensor entry aligned and misaligned."""
    from neunet_hip import optim
    rng = np.random.default_rng(2402)
    sizes = [2051, 7, 4096]
    ns = N_STATE[rule]
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    gs = [[rng.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(3)]
    assert optim_ref.plan(sizes) == (2048, 2 + 1 + 2)

    def place(a, off):
        t = shifted(a) if off else dev(a)
        assert t.data_ptr() % 16 == (4 if off else 0)
        return t

    def run(entry, off):
        if entry == "multi":
            params = make_params(hip, p0)
            opt = getattr(optim, CLASS_NAMES[rule])(params)
            for i, p in enumerate(params):
                if "p" in off:
                    p.data = shifted(p0[i])
                for name in STATE_NAMES[:ns]:
                    if name in off:
                        getattr(opt, name)[i] = shifted(np.zeros(sizes[i], np.float32))
            for s in range(3):
                for i, p in enumerate(params):
                    p.grad = place(gs[s][i], "g" in off)
                opt.step()
            for i, p in enumerate(params):
                assert p.data.data_ptr() % 16 == (4 if "p" in off else 0)
                for k, t in enumerate(opt_states(opt, i)):
                    assert t.data_ptr() % 16 == (4 if STATE_NAMES[k] in off else 0)
            return snapshot(opt, params)
        ps = [place(a, "p" in off) for a in p0]
        ss = [[place(np.zeros(n, np.float32), STATE_NAMES[k] in off) for k in range(ns)] for n in sizes]
        for s in range(3):
            for i in range(len(sizes)):
                per_tensor_call(rule, ps[i], place(gs[s][i], "g" in off), ss[i], sizes[i], s + 1)
        return [[host(ps[i])] + [host(t) for t in ss[i]] for i in range(len(sizes))]

    want = run("multi", "")
    assert_moved(want, p0)
    everything = "pg" + STATE_NAMES[:ns]
    cases = [("multi", everything), ("multi", "g"), ("single", ""), ("single", everything), ("single", "g")]
    cases += [(entry, name) for name in STATE_NAMES[:ns] for entry in ("multi", "single")]
    for entry, off in cases:
        assert_same_bits(run(entry, off), want, f"{rule} {entry} entry, unaligned '{off}'")


# ------------------------------------------------------------------------------------------------------------ 5: special values
SPECIAL = np.array([0.0, 0.0, 0.0, 1e-30, -1e-30, 1e18, -1e18, 1e20, -1e20, np.inf, -np.inf, np.nan, np.nan], np.float32)
DIVIDES_BY_SECOND_MOMENT = {"rmsprop": 0, "adagrad": 0, "adadelta": 0, "nadam": 1}      # rule -> the state that g * g overflows


def special_run(hip, rule, p0, gs, state0=None, **hyper):
    """Two steps through the class; after each, NaN, +inf and -inf where the restatement has them and the finite entries within
    the tolerances.  Returns (device snapshot, restatement) after the last step."""
    from neunet_hip import optim
    params = make_params(hip, [p0])
    opt = getattr(optim, CLASS_NAMES[rule])(params, **hyper)
    ref = [p0.copy()] + optim_ref.init_state(rule, p0)
    if state0 is not None:
        for k, a in enumerate(state0):
            ref[1 + k][...] = a
            opt_states(opt, 0)[k].copy_(dev(a))
    for s, g in enumerate(gs):
        feed(params, [g])
        opt.step()
        with np.errstate(all="ignore"):
            optim_ref.step(rule, ref[0], g, ref[1:], s + 1, **hyper)
        got = snapshot(opt, params)[0]
        for k in range(len(ref)):
            what = f"{rule} step {s + 1} {STREAMS[k]}"
            np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=what)
            np.testing.assert_array_equal(np.isposinf(got[k]), np.isposinf(ref[k]), err_msg=what)
            np.testing.assert_array_equal(np.isneginf(got[k]), np.isneginf(ref[k]), err_msg=what)
            fin = np.isfinite(ref[k])
            np.testing.assert_allclose(got[k][fin], ref[k][fin], rtol=RTOL, atol=ATOL[k], err_msg=what)
    return got, ref


@by_rule
def test_special_values(hip, rule):
    """Gradients 0, +-1e-30 (g * g underflows), +-1e18, +-1e20 (g * g overflows), +-inf, NaN and parameters 0, -0 among ordinary
    ones, two steps; the second NaN gradient is an ordinary number in the second step.  The cases are what they claim: g * g = inf
    freezes the parameter where the rule divides by the second moment (RMSprop, Adagrad, Adadelta, NAdam), 1e18 moves it; a zero
    gradient leaves the states zero and, under SGD, Momentum and Adamax, p bit-identical (-0 stays -0); Adamax keeps the NaN a NaN
    gradient left in v when the next gradient is finite (np.maximum: a != a)."""
    rng = np.random.default_rng(2404)
    n = 64
    p0 = rng.standard_normal(n).astype(np.float32)
    p0[0], p0[1] = 0.0, -0.0                                     # with a zero gradient; p0[2] is an ordinary value with a zero gradient
    p0[20], p0[21] = 0.0, -0.0                                   # with an ordinary gradient
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    for g in gs:
        g[:SPECIAL.size] = SPECIAL
    gs[1][12] = 0.75
    got, ref = special_run(hip, rule, p0, gs)
    ns = N_STATE[rule]
    assert np.isfinite(ref[0][:9]).all() and np.isfinite(ref[0][13:]).all() and not np.isfinite(ref[0][9:12]).any()
    for k in range(1, 1 + ns):                                   # a zero gradient leaves the states zero
        np.testing.assert_array_equal(bits(got[k][:3]), 0)
    if rule in ("sgd", "momentum", "adamax"):
        np.testing.assert_array_equal(bits(got[0][:3]), bits(p0[:3]))
        assert bits(got[0][:3])[1] == 0x80000000
    assert np.all(got[0][20:22] != 0)
    assert np.all(got[0][5:7] != p0[5:7])                        # 1e18: g * g is finite, the parameter moved
    if rule in DIVIDES_BY_SECOND_MOMENT:
        assert np.isposinf(got[1 + DIVIDES_BY_SECOND_MOMENT[rule]][7:9]).all()
        np.testing.assert_array_equal(bits(got[0][7:9]), bits(p0[7:9]))
    else:
        assert np.all(got[0][7:9] != p0[7:9])
    if rule == "adamax":
        assert np.isnan(got[2][11:13]).all() and np.isfinite(gs[1][12])
        assert np.isposinf(got[2][9:11]).all() and np.isnan(got[0][9:13]).all()


def test_adamax_from_a_state_with_nan_and_inf(hip):
    """v holds a NaN and an inf before the first step, the gradients there are ordinary: beta2 * NaN stays NaN (a != a), beta2 * inf
    stays inf and freezes its parameter."""
    rng = np.random.default_rng(2405)
    n = 64
    p0 = rng.standard_normal(n).astype(np.float32)
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    m0, v0 = rng.standard_normal(n).astype(np.float32), np.abs(rng.standard_normal(n)).astype(np.float32)
    v0[30], v0[31] = np.nan, np.inf
    got, ref = special_run(hip, "adamax", p0, gs, state0=[m0, v0])
    assert np.isnan(got[2][30]) and np.isposinf(got[2][31]) and np.isnan(got[0][30])
    assert bits(got[0][31:32])[0] == bits(p0[31:32])[0] and np.isfinite(got[1]).all()
    assert np.isfinite(got[0][:30]).all() and np.all(got[0][:30] != p0[:30])


@pytest.mark.parametrize("rule", ["rmsprop", "adagrad"])
def test_zero_gradient_with_eps_zero(hip, rule):
    """eps = 0 and g = 0: lr * 0 / (sqrt(0) + 0) is NaN, as NumPy gives it; the state stays zero."""
    rng = np.random.default_rng(2406)
    p0 = rng.standard_normal(16).astype(np.float32)
    gs = [rng.standard_normal(16).astype(np.float32) for _ in range(2)]
    for g in gs:
        g[:4] = 0.0
    got, ref = special_run(hip, rule, p0, gs, eps=0.0)
    assert np.isnan(ref[0][:4]).all() and np.isnan(got[0][:4]).all() and np.isfinite(got[0][4:]).all()
    np.testing.assert_array_equal(bits(got[1][:4]), 0)


# ------------------------------------------------------------------------------------------------------------- 6: table edges
def table(ts):
    from ctypes import POINTER, c_void_p, cast
    return cast((c_void_p * len(ts))(*[t.data_ptr() if t is not None and t.numel() else None for t in ts]), POINTER(c_void_p))


def multi_call(handle, rule, n, p, g, s1, s2, sizes, t, **hyper):
    from ctypes import POINTER, c_int64, cast
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    c1, c2, eps = optim_ref.coefficients(rule, hyper)
    lr = dict(optim_ref.DEFAULTS[rule], **hyper)["lr"]
    sz = None if sizes is None else cast((c_int64 * len(sizes))(*sizes), POINTER(c_int64))
    return call_hip_function("nnhipOptimizerRuleMultiTensorStep", handle, RULE_ID[rule], n, p, g, s1, s2, sz, lr, c1, c2, eps, t, 1.0,
                             get_current_stream_ptr())


@pytest.fixture
def handle(hip):
    from neunet_hip._lib import load_hip_function
    h = load_hip_function("nnhipCreateFusedOptimizer")()
    assert h
    yield h
    load_hip_function("nnhipDestroyFusedOptimizer")(h)


@by_rule
def test_empty_tensor_and_null_state_tables(hip, handle, rule):
    """The C entry with sizes {300, 0, 2049}, null pointers in the empty tensor's slots and NULL for the state tables the rule does
    not have (SGD both, the one-state rules s2): status 0, no block for the empty tensor, its neighbours updated -- the blob of
    2, 3 or 4 pointer tables.  n_tensors == 0 with every table NULL returns 0."""
    import torch
    sc = scenario("zero_mid")
    sizes, ns = sizes_of(sc.shapes), N_STATE[rule]
    assert sizes == [300, 0, 2049] and optim_ref.plan(sizes) == (2048, 3)
    assert optim_ref.plan_bytes(rule, sizes) == 24 * (2 + ns) + 24 + 24
    assert multi_call(handle, rule, 0, None, None, None, None, None, 1) == 0
    ps = [dev(a) for a in sc.p0]
    ss = [[torch.zeros_like(p) for p in ps] for _ in range(ns)]
    tr = Trace(rule, sc)
    for s, grads in enumerate(sc.grads):
        gd = [dev(g) for g in grads]
        tabs = [table(ps), table(gd)] + [table(x) for x in ss] + [None] * (2 - ns)
        assert all(t is None or (not t[1] and t[0] and t[2]) for t in tabs) and tabs[2:].count(None) == 2 - ns
        assert multi_call(handle, rule, 3, *tabs, sizes, s + 1) == 0
        tr.step()
        check(tr, [[host(ps[i])] + [host(x[i]) for x in ss] for i in range(3)], f"zero_mid {rule} step {tr.t}")
    torch.cuda.synchronize()


def refused(entry, call):
    """The call answers NNHIP_EINVAL (-1) with a message that names the entry."""
    from neunet_hip._lib import NeunetHipError
    with pytest.raises(NeunetHipError, match=rf"{entry} failed with status -1: {entry}: ") as e:
        call()
    return str(e.value)


@by_rule
def test_refusals_write_nothing(hip, handle, rule):
    """A NULL required state table / pointer, an unknown rule (-1 and 7), a negative size, step < 1 on the per-tensor entry and a NULL
    pointer for a non-empty tensor: NNHIP_EINVAL, the entry named, and p, the states and their guard words as they were."""
    import torch
    rng = np.random.default_rng(2407)
    ns, sizes = N_STATE[rule], [300, 2049]
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    s0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    ps = [guarded(a) for a in p0]
    ss = [[guarded(a) for a in s0] for _ in range(ns)]
    gd = [dev(rng.standard_normal(n).astype(np.float32)) for n in sizes]
    P, G = [p[1] for p in ps], gd
    S = [[x[1] for x in st] for st in ss] + [None, None]
    tabs = lambda: [table(P), table(G)] + [None if s is None else table(s) for s in S[:2]]  # noqa: E731
    M, T = "nnhipOptimizerRuleMultiTensorStep", "nnhipOptimizerRuleStep"

    def multi(rule_id=RULE_ID[rule], n=2, t=None, sz=sizes, step=1):
        from ctypes import POINTER, c_int64, cast
        from neunet_hip._lib import call_hip_function, get_current_stream_ptr
        t = tabs() if t is None else t
        c1, c2, eps = optim_ref.coefficients(rule, {})
        return call_hip_function(M, handle, rule_id, n, *t, cast((c_int64 * len(sz))(*sz), POINTER(c_int64)), 0.01, c1, c2, eps, step, 1.0,
                                 get_current_stream_ptr())

    def single(rule_id=RULE_ID[rule], p=P[0], g=G[0], s1=S[0] and S[0][0], s2=S[1] and S[1][0], n=sizes[0], step=1):
        from neunet_hip._lib import call_hip_function, get_current_stream_ptr
        c1, c2, eps = optim_ref.coefficients(rule, {})
        return call_hip_function(T, rule_id, p, g, s1, s2, n, 0.01, c1, c2, eps, step, 1.0, get_current_stream_ptr())

    for bad in (-1, 7):
        assert "unknown rule" in refused(M, lambda: multi(rule_id=bad))
        assert "unknown rule" in refused(T, lambda: single(rule_id=bad))
    assert "negative size" in refused(M, lambda: multi(sz=[300, -5]))
    assert "negative size" in refused(T, lambda: single(n=-1))
    for step in (0, -1):
        assert "step >= 1" in refused(T, lambda: single(step=step))
    assert "bad n_tensors/step" in refused(M, lambda: multi(step=-1))
    assert "bad n_tensors/step" in refused(M, lambda: multi(n=-1))
    for k in range(ns):                                          # a state table / pointer the rule needs
        t = tabs()
        t[2 + k] = None
        assert "null state table" in refused(M, lambda: multi(t=t))
        assert "null state pointer" in refused(T, lambda: single(**{f"s{k + 1}": None}))
    for k in range(2 + ns):                                      # a NULL pointer in a non-empty tensor's slot, in each table
        t = tabs()
        t[k] = table([([P, G] + S)[k][0], None])
        assert "null tensor pointer" in refused(M, lambda: multi(t=t))
    assert "null table" in refused(M, lambda: multi(t=[None, table(G)] + tabs()[2:]))
    assert "null pointer" in refused(T, lambda: single(p=None))
    assert "null pointer" in refused(T, lambda: single(g=None))
    torch.cuda.synchronize()
    assert_guards(ps + [x for st in ss for x in st], rule)
    for i in range(2):
        np.testing.assert_array_equal(bits(host(P[i])), bits(p0[i]))
        for st in S[:ns]:
            np.testing.assert_array_equal(bits(host(st[i])), bits(s0[i]))
    # the handle and the buffers are good for a step afterwards
    assert multi() == 0 and single(step=2) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(host(P[1]), p0[1])
    assert_guards(ps + [x for st in ss for x in st], rule)


# ------------------------------------------------------------------------------------- 7: device-side stepping, driven directly, eager
def step_pair(hip, rule, name):
    """A scenario on two optimizers: one host-stepped, one with use_device_step().  What a step changes (over[s]) is assigned to both
    before it.  The device-stepped one ends every step with the host-stepped one's bits; the host-stepped one follows the references.
    A tensor without a gradient keeps its bits."""
    sc = scenario(name)
    assert optim_ref.plan(sizes_of(sc.shapes)) == (2048, 4)        # 4 blocks: the last one to finish is not always the same
    (h_opt, h_par), (d_opt, d_par) = make_opt(hip, rule, sc), make_opt(hip, rule, sc)
    d_opt.use_device_step()
    assert d_opt.device_step and not h_opt.device_step
    tr = Trace(rule, sc)
    for grads, over in zip(sc.grads, sc.over):
        for opt in (h_opt, d_opt):
            apply_over(opt, rule, over)
        feed(h_par, grads)
        feed(d_par, grads)
        before = snapshot(d_opt, d_par)
        h_opt.step()
        d_opt.step()
        tr.step()
        hs, ds = snapshot(h_opt, h_par), snapshot(d_opt, d_par)
        assert_same_bits(ds, hs, f"{name} {rule} device-stepped, step {tr.t}")
        check(tr, hs, f"{name} {rule} step {tr.t}")
        for i, g in enumerate(grads):
            if g is None:
                assert_same_bits([ds[i]], [before[i]], "skipped")
    assert h_opt.t == d_opt.t == tr.t
    return sc


@by_rule
def test_device_stepping_24_steps(hip, rule):
    """No host read between the steps; the step count (and for Adamax / NAdam the bias corrections) of steps 2..24 come from the
    previous launch's last block.  Bit for bit the host-stepped run."""
    from neunet_hip import optim
    rng = np.random.default_rng(2403)
    shapes = optim_ref.DEV_SHAPES
    assert optim_ref.plan(sizes_of(shapes)) == (2048, 4)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    gs = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(24)]
    snaps = []
    for device in (False, True):
        params = make_params(hip, p0)
        opt = getattr(optim, CLASS_NAMES[rule])(params)
        if device:
            opt.use_device_step()
        for grads in gs:
            feed(params, grads)
            opt.step()
        assert opt.t == 24 and opt.device_step == device
        snaps.append(snapshot(opt, params))
    assert_same_bits(snaps[1], snaps[0], f"{rule}: 24 device-stepped steps")
    assert_moved(snaps[0], p0)


@pytest.mark.parametrize("t0", [1000, 99990])
@pytest.mark.parametrize("rule", BETA_RULES)
def test_device_stepping_resumes_at_a_step(hip, rule, t0):
    """A restored checkpoint: opt.t = t0 and non-zero m, v, then use_device_step() and 5 steps -- steps t0 + 1 .. t0 + 5, against
    float64.  Adamax uses bc1 alone, NAdam bc1 and bc2."""
    sc = step_pair(hip, rule, f"resume_{t0}")
    assert sc.t0 == t0 and len(sc.grads) == 5 and sc.m0 is not None


@pytest.mark.parametrize("rule", BETA_RULES)
def test_device_stepping_betas_change(hip, rule):
    """Other betas for the third and fourth device-stepped step, then the first ones again: the bias corrections the previous step
    left were computed for other betas and must be dropped, both times."""
    sc = step_pair(hip, rule, "dev_betas")
    assert [o.get("betas") for o in sc.over] == [None] * 2 + [(0.8, 0.99)] * 2 + [None] * 2


@pytest.mark.parametrize("rule", sorted(COEF_NAME))
def test_device_stepping_coefficient_change(hip, rule):
    """Momentum's momentum, RMSprop's alpha, Adadelta's rho set to 0.5 before the third eager device-stepped launch: coefficients stay
    launch arguments (use_device_step's docstring), so the new value acts at once -- the host-stepped run's bits."""
    sc = step_pair(hip, rule, "dev_coef")
    assert [o.get("coef") for o in sc.over] == [None, None, 0.5, 0.5, 0.5]


@by_rule
def test_device_stepping_block_count_changes(hip, rule):
    """The second launch has 2 blocks instead of 4 (the two-chunk tensor has no gradient: it keeps its bits), the third 4 again: the
    ticket picks the last block of each, and the counter advances by one per launch -- the steps after show it."""
    sc = step_pair(hip, rule, "dev_blocks")
    assert [g[0] is None for g in sc.grads] == [False, True, False, False]
    assert optim_ref.plan(sizes_of(sc.shapes[1:])) == (2048, 2)


@by_rule
def test_device_stepping_hyper_parameter_changes(hip, rule):
    """opt.lr, then opt.grad_scale change between two device-stepped steps (sync_device_hyper) and hold from the next step on."""
    sc = step_pair(hip, rule, "dev_hyper")
    assert sc.over == [{}, dict(lr=3e-3), dict(lr=3e-3), dict(lr=3e-3, grad_scale=0.5), dict(lr=3e-3, grad_scale=0.5)]


@by_rule
def test_device_stepping_needs_a_prepared_handle(hip, handle, rule):
    """step == 0 on a handle that never saw SetStep / SetHyper is refused before the plan is built, let alone uploaded: a table whose
    sizes the plan builder would refuse ("too many chunks") still gets the step's message, nothing is written, and after SetStep
    alone (no SetHyper) it is refused the same way."""
    import torch
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    M = "nnhipOptimizerRuleMultiTensorStep"
    ns = N_STATE[rule]
    rng = np.random.default_rng(2408)
    a = rng.standard_normal(300).astype(np.float32)
    bufs = [guarded(a) for _ in range(1 + ns)]
    g = dev(a)
    tabs = [table([bufs[0][1]]), table([g])] + [table([b[1]]) for b in bufs[1:]] + [None] * (2 - ns)
    for sizes in ([300], [1 << 62]):
        assert "step == 0 needs nnhipFusedOptimizerSetStep and SetHyper first" in refused(M, lambda: multi_call(handle, rule, 1, *tabs, sizes, 0))
    assert "too many chunks" in refused(M, lambda: multi_call(handle, rule, 1, *tabs, [1 << 62], 1))
    call_hip_function("nnhipFusedOptimizerSetStep", handle, 0, get_current_stream_ptr())
    assert "SetHyper first" in refused(M, lambda: multi_call(handle, rule, 1, *tabs, [300], 0))
    torch.cuda.synchronize()
    assert_guards(bufs, rule)
    for b in bufs:
        np.testing.assert_array_equal(bits(host(b[1])), bits(a))
    call_hip_function("nnhipFusedOptimizerSetHyper", handle, 0.01, 0.0, 1.0, get_current_stream_ptr())
    assert multi_call(handle, rule, 1, *tabs, [300], 0) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(host(bufs[0][1]), a)
    assert_guards(bufs, rule)


# ------------------------------------------------------------------------------------------------------------------ 8: captured
@pytest.mark.parametrize("rule", ["momentum", "adagrad", "adadelta", "adamax"])     # tests/test_optim_gpu.py has the other three
def test_graph_replay_equals_eager(hip, golden, rule):
    """6 replays through GraphedTrainStep (step count, lr and Adamax's bias correction from device memory) leave the p and states of
    6 eager host-stepped steps; then a new opt.lr between replays takes effect (Adadelta has no lr: the same bits again)."""
    import neunet_hip.nn as nn
    from neunet_hip import optim
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    g = golden("mlp_optim_rules")
    rng = np.random.default_rng(2409)
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

        return model, x, y, fb, getattr(optim, CLASS_NAMES[rule])(model.parameters())

    def feed_batch(x, y, item):
        x.data.copy_(dev(item[0]))
        y.data.copy_(dev(item[1]))

    m0, x0, y0, fb0, opt0 = make()

    def eager(item):
        feed_batch(x0, y0, item)
        opt0.zero_grad()
        fb0()
        opt0.step()
        assert not opt0.device_step

    for item in data[:warm + steps]:
        eager(item)
    want = snapshot(opt0, m0.parameters())

    m1, x1, y1, fb1, opt1 = make()
    warm_items = iter(data[:warm])

    def fb_warm():
        item = next(warm_items, None)
        if item is not None:                                       # the eager warm-up steps read items 0 and 1
            feed_batch(x1, y1, item)
        return fb1()

    step = GraphedTrainStep(fb_warm, opt1, GradBucket(m1.parameters()), warmup=warm)
    try:
        assert opt1.device_step
        for item in data[warm:warm + steps]:
            feed_batch(x1, y1, item)
            step()
        assert_same_bits(snapshot(opt1, m1.parameters()), want, f"{rule}: 6 replays")
        assert_moved(want, [g[n] for n in ("W1", "b1", "W2", "b2")])
        # an LR schedule between replays
        opt0.lr = opt1.lr = opt0.lr * 0.25
        eager(data[-1])
        feed_batch(x1, y1, data[-1])
        step()
        assert_same_bits(snapshot(opt1, m1.parameters()), snapshot(opt0, m0.parameters()), f"{rule}: replay after the LR change")
    finally:
        step.release()


# ------------------------------------------------------------------------------------------------------------------ 9: plan churn
CHURN_SIZES = [100, 2049, 3000]


@pytest.mark.parametrize("rule", ["sgd", "rmsprop", "nadam"])      # one rule per table count: 2, 3 and 4 pointer tables
def test_plan_churn(hip, rule):
    """Every one of 8 steps hands over its gradients in buffers of their own (all kept alive: 8 different gradient tables), and
    before the fifth step one state tensor moves to new storage (SGD has none: a parameter does).  The blob keeps its size and block
    count throughout; only its pointers change, twice round the ring of 4 staging buffers.  Bit for bit a run whose gradients arrive
    in the same buffers at every step and whose tensors stay put; and the restatement's values."""
    from neunet_hip import optim
    rng = np.random.default_rng(2410)
    ns, steps = N_STATE[rule], 8
    p0 = [rng.standard_normal(n).astype(np.float32) for n in CHURN_SIZES]
    gs = [[rng.standard_normal(n).astype(np.float32) for n in CHURN_SIZES] for _ in range(steps)]
    assert optim_ref.plan(CHURN_SIZES) == (2048, 1 + 2 + 2) and optim_ref.plan_bytes(rule, CHURN_SIZES) == 24 * (2 + ns) + 24 + 40

    def run(churn):
        params = make_params(hip, p0)
        opt = getattr(optim, CLASS_NAMES[rule])(params)
        keep, seen = [], set()
        fixed = [dev(np.zeros(n, np.float32)) for n in CHURN_SIZES]
        for s in range(steps):
            if churn and s == steps // 2:
                old = params[1].data if ns == 0 else opt_states(opt, 1)[-1]
                new = old.clone()
                assert new.data_ptr() != old.data_ptr()
                keep.append(old)
                if ns == 0:
                    params[1].data = new
                else:
                    getattr(opt, STATE_NAMES[ns - 1])[1] = new
            for i, p in enumerate(params):
                if churn:
                    p.grad = dev(gs[s][i])
                    keep.append(p.grad)
                else:
                    fixed[i].copy_(dev(gs[s][i]))
                    p.grad = fixed[i]
            seen.add(tuple(p.grad.data_ptr() for p in params))
            opt.step()
        assert len(seen) == (steps if churn else 1)
        return snapshot(opt, params)

    got = run(True)
    assert_same_bits(got, run(False), f"{rule}: stable buffers")
    ref = [[a.copy()] + optim_ref.init_state(rule, a) for a in p0]
    for s in range(steps):
        for i in range(len(CHURN_SIZES)):
            optim_ref.step(rule, ref[i][0], gs[s][i], ref[i][1:], s + 1)
    for i in range(len(CHURN_SIZES)):
        for k in range(1 + ns):
            np.testing.assert_allclose(got[i][k], ref[i][k], rtol=RTOL, atol=ATOL[k], err_msg=f"{STREAMS[k]}[{i}]")
    assert_moved(got, p0)
