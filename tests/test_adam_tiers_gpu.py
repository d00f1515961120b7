"""GPU: Adam / AdamW of csrc/optim.hip on every kernel path -- adam_span's unrolled rounds, single rounds and scalar tail under both
chunk plans of the multi-tensor entry and beyond the grid cap of the per-tensor entry; the scalar path, bit for bit against the vector
path in both entries; special values; skipped parameters, strided gradients, an empty tensor in the table, grad_scale and the device
divisor; device-side stepping (csrc/adam_device.h: adam_dev_issue / resolve / finish) driven directly -- resumed at an arbitrary step,
betas / block count / hyper-parameters changed between launches -- and captured; the plan blob re-uploaded at every step.

Every test checks p, m and v.  References (tests/adam_ref.py): step32, the reference's float32 arithmetic, and step64, the float64 value
of what the kernel is asked to compute; tolerances test_adam_golden's (rtol 1e-5; atol 1e-6 p, 1e-7 m, 1e-8 v).  Float64 comparisons run
for at most 8 steps on standard-normal data (tests/test_adam_ref.py holds step32 itself to 0.75 of the tolerances there); longer runs
compare device with device, bit for bit.

Measured on an MI355X, worst |kernel - step64| / (atol + rtol |step64|) over all float64 comparisons below (every test prints its own):
    p 0.044 (AdamW, sixth step of the betas-change run)   m 0.504 (AdamW, step 1005 of the resumed run)   v 0.033 (Adam, step 99995)
step32 against step64 on the same inputs: p 0.035, m 0.390, v 0.037 -- the kernel is as close to float64 as the reference's own float32
arithmetic is, with no sign of contraction or of a non-IEEE division or square root.

Each group was seen to fail under a deliberate one-line break of the library: the tail started one element late, the unrolled loop
advanced by one stride instead of two (both fail groups 1-4, 6, 7, 9), `cached` forced true in adam_dev_resolve (group 7 and 8), a plan
re-uploaded only when its size or block count changed (group 9)."""
import ctypes

import numpy as np
import pytest

import adam_ref
from adam_ref import ATOL, DECOUPLED, L2_ON_GRAD, RTOL, Trace, scenario

pytestmark = pytest.mark.gpu
CLASSES = [("Adam", L2_ON_GRAD), ("AdamW", DECOUPLED)]
by_class = pytest.mark.parametrize("cls,mode", CLASSES, ids=[c for c, _ in CLASSES])
NAMES = "pmv"


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


def make_opt(hip, cls, mode, sc, entry="multi"):
    """(optimizer, parameters) on a scenario's initial values, state and step count."""
    from neunet_hip import optim
    params = make_params(hip, sc.p0)
    if entry == "multi":
        opt = getattr(optim, cls)(params, lr=sc.lr, betas=sc.betas, eps=sc.eps, weight_decay=sc.wd)
    else:
        opt = optim.HIPFusedAdamW(params, lr=sc.lr, betas=sc.betas, eps=sc.eps, weight_decay=sc.wd)
        opt.decay_mode = mode
    assert opt.decay_mode == mode
    for i in range(len(params)):
        if sc.m0 is not None:
            opt.m[i].copy_(dev(sc.m0[i]))
            opt.v[i].copy_(dev(sc.v0[i]))
    opt.t = sc.t0
    return opt, params


def feed(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else dev(g)


def snapshot(opt, params):
    return [[host(p.data), host(opt.m[i]), host(opt.v[i])] for i, p in enumerate(params)]


def assert_same_bits(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        for k in range(3):
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{what} {NAMES[k]}[{i}]")


def assert_moved(snap, sc):
    for i, x in enumerate(snap):
        assert x[0].size == 0 or not np.array_equal(x[0], sc.p0[i])
        assert x[1].size == 0 or (np.any(x[1] != 0) and np.any(x[2] != 0))


def check(tr, snap, what):
    """Device p, m, v against both references at the tolerances above; prints the worst ratio to float64."""
    worst = [0.0, 0.0, 0.0]
    for i, x in enumerate(snap):
        for k, (r32, r64) in enumerate(((tr.p32[i], tr.p64[i]), (tr.m32[i], tr.m64[i]), (tr.v32[i], tr.v64[i]))):
            got = tr.pick(i, x[k])
            worst[k] = max(worst[k], adam_ref.worst_ratio(got, r64, ATOL[k]))
    print(f"kernel vs step64, {what}: worst ratio p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    for i, x in enumerate(snap):
        for k, (r32, r64) in enumerate(((tr.p32[i], tr.p64[i]), (tr.m32[i], tr.m64[i]), (tr.v32[i], tr.v64[i]))):
            got = tr.pick(i, x[k])
            np.testing.assert_allclose(got, r32, rtol=RTOL, atol=ATOL[k], err_msg=f"{what}: {NAMES[k]}[{i}] vs step32")
            np.testing.assert_allclose(got, r64, rtol=RTOL, atol=ATOL[k], err_msg=f"{what}: {NAMES[k]}[{i}] vs step64")


def run_scenario(hip, name, cls, mode, entry="multi"):
    sc = scenario(name, mode)
    opt, params = make_opt(hip, cls, mode, sc, entry)
    tr = Trace(sc)
    for s, grads in enumerate(sc.grads):
        feed(params, grads)
        opt.step()
        tr.step()
        check(tr, snapshot(opt, params), f"{name} {cls} {entry} step {tr.t}")
    assert opt.t == tr.t
    return sc, opt, params


def sizes_of(shapes):
    return [int(np.prod(s)) for s in shapes]


# ------------------------------------------------------------------------------------------ 1, 2: the multi-tensor entry's two plans
@by_class
def test_tail_and_round_matrix_small_chunks(hip, cls, mode):
    """2048-element chunks.  1500 elements: threads 0-118 take the unrolled round, the others single rounds; 1027: 256 float4 and a
    3-element tail; 2049: one element in a second chunk; 1, 3: the tail alone."""
    sizes = sizes_of(adam_ref.TAIL_SHAPES)
    assert sizes[:11] == [1, 3, 4, 5, 1023, 1027, 1500, 2047, 2048, 2049, 4099] and sizes[11] == 333000
    assert adam_ref.plan(sizes) == (2048, 9 + 2 + 3 + 163)
    run_scenario(hip, "tail", cls, mode)


@by_class
def test_large_chunk_plan(hip, cls, mode):
    """16384-element chunks (>= 2^22 elements in all).  The large tensor is compared on its first and last chunk whole, 8 elements
    beyond each, and every 1021st element between; the small tensors in full."""
    sizes = sizes_of(adam_ref.LARGE_SHAPES)
    assert sum(sizes) >= 1 << 22 and adam_ref.plan(sizes) == (16384, 256 + 2 + 1)
    sc = scenario("large", mode)
    assert sc.idx[0][16384 + 7] == 16384 + 7 and sc.idx[0][-(16384 + 8)] == sizes[0] - 16384 - 8 and sc.idx[1] is None
    run_scenario(hip, "large", cls, mode)


# ------------------------------------------------------------------------------------------------------ 3: the per-tensor entry
@pytest.mark.parametrize("name", ["per_tensor", "per_tensor2"])
@by_class
def test_per_tensor_entry_beyond_the_grid_cap(hip, cls, mode, name):
    """nnhipFusedAdamWStep caps its grid at 2048 blocks (a stride of 524 288 float4).  per_tensor: 4 195 507 elements -- every thread
    takes one unrolled trip (two strides), threads 0-299 one more single round, three elements the scalar tail -- and n = 1, 3, 4,
    1027.  per_tensor2: 6 292 659 elements, where threads 0-299 take a SECOND unrolled trip and the others a single round.  The long
    tensor is compared on 16 K elements at both ends and every 1021st between."""
    sc = scenario(name, mode)
    n = sc.shapes[0][0]
    stride4 = 2048 * 256
    assert n % 4 == 3 and (n >> 2) == (2 if name == "per_tensor" else 3) * stride4 + 300
    assert sc.idx[0][16383] == 16383 and sc.idx[0][-16384] == n - 16384 and sc.idx[0].size > 2 * 16384 + n // 1021 - 40
    run_scenario(hip, name, cls, mode, entry="single")


# ------------------------------------------------------------------------------------------- 4: one arithmetic, four kernels, same bits
def shifted(a):
    """A contiguous device copy that starts one float into its buffer: 4-byte alignment only."""
    import torch
    a = np.asarray(a)
    buf = torch.zeros(a.size + 5, dtype=torch.float32, device="cuda")
    view = buf[1:1 + a.size]
    view.copy_(dev(a.reshape(-1)))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@by_class
def test_vector_and_scalar_paths_of_both_entries_give_the_same_bits(hip, cls, mode):
    """adam1 is inlined into the vector rounds, the tail and the scalar loop of two kernels (fp contract(off)): the multi-tensor and the
    per-tensor entry, each with everything 16-byte aligned, with p, g, m, v all one float into their buffers, and with ONLY the
    gradient so (the vector path must be refused then too), leave the same p, m, v."""
    from neunet_hip import optim
    rng = np.random.default_rng(2302)
    sizes = [2051, 7, 4096]
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    gs = [[rng.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(3)]

    def run(entry, off):
        params = make_params(hip, p0)
        if entry == "multi":
            opt = getattr(optim, cls)(params, lr=1e-2, weight_decay=1e-2)
        else:
            opt = optim.HIPFusedAdamW(params, lr=1e-2, weight_decay=1e-2)
            opt.decay_mode = mode
        for i, p in enumerate(params):
            if "p" in off:
                p.data = shifted(p0[i])
            if "m" in off:
                opt.m[i] = shifted(np.zeros(sizes[i], np.float32))
            if "v" in off:
                opt.v[i] = shifted(np.zeros(sizes[i], np.float32))
        for s in range(3):
            for i, p in enumerate(params):
                p.grad = shifted(gs[s][i]) if "g" in off else dev(gs[s][i])
                assert p.grad.data_ptr() % 16 == (4 if "g" in off else 0)
            opt.step()
        for i, p in enumerate(params):
            assert p.data.data_ptr() % 16 == (4 if "p" in off else 0)
            assert opt.m[i].data_ptr() % 16 == (4 if "m" in off else 0) and opt.v[i].data_ptr() % 16 == (4 if "v" in off else 0)
        return snapshot(opt, params)

    want = run("multi", "")
    for i, x in enumerate(want):
        assert not np.array_equal(x[0], p0[i]) and np.all(x[1] != 0) and np.all(x[2] != 0)
    for entry, off in (("multi", "pgmv"), ("single", ""), ("single", "pgmv"), ("multi", "g"), ("single", "g")):
        assert_same_bits(run(entry, off), want, f"{entry} entry, unaligned '{off}'")


# ------------------------------------------------------------------------------------------------------------ 5: special values
@by_class
def test_special_values(hip, cls, mode):
    """Gradients 0, +-1e-30 (g * g underflows), +-1e18, +-1e20 (g * g overflows), +-inf, NaN and parameters 0, -0 among ordinary ones:
    NaN and inf land where step32 puts them, the finite entries hold the tolerances; a zero gradient leaves m = v = 0."""
    rng = np.random.default_rng(2304)
    n, lr, wd = 64, 1e-2, 1e-2
    special = np.array([0.0, 0.0, 0.0, 1e-30, -1e-30, 1e18, -1e18, 1e20, -1e20, np.inf, -np.inf, np.nan], np.float32)
    p0 = rng.standard_normal(n).astype(np.float32)
    p0[0], p0[1] = 0.0, -0.0                                     # with a zero gradient; p0[2] is an ordinary value with a zero gradient
    p0[20], p0[21] = 0.0, -0.0                                   # with an ordinary gradient
    gs = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    for g in gs:
        g[:special.size] = special
    from neunet_hip import optim
    params = make_params(hip, [p0])
    opt = getattr(optim, cls)(params, lr=lr, weight_decay=wd)
    ref = [p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)]
    for s in range(2):
        feed(params, [gs[s]])
        opt.step()
        with np.errstate(all="ignore"):
            adam_ref.step32(mode, ref[0], gs[s], ref[1], ref[2], s + 1, lr, (0.9, 0.999), 1e-8, wd)
        got = snapshot(opt, params)[0]
        for k in range(3):
            what = f"{cls} step {s + 1} {NAMES[k]}"
            np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=what)
            np.testing.assert_array_equal(np.isposinf(got[k]), np.isposinf(ref[k]), err_msg=what)
            np.testing.assert_array_equal(np.isneginf(got[k]), np.isneginf(ref[k]), err_msg=what)
            fin = np.isfinite(ref[k])
            np.testing.assert_allclose(got[k][fin], ref[k][fin], rtol=RTOL, atol=ATOL[k], err_msg=what)
    # the cases are what they claim to be
    assert np.isnan(ref[0][9:12]).all() and np.isinf(ref[2][7:9]).all() and np.isfinite(ref[0][:9]).all() and np.isfinite(ref[0][12:]).all()
    if mode == DECOUPLED:                                                     # 1e-30: v underflowed, m did not (Adam adds wd * p)
        assert np.all(ref[2][3:5] == 0) and np.all(ref[1][3:5] != 0)
    assert np.all(np.abs(ref[0][5:7] - p0[5:7]) > 1e-3)                       # 1e18 moved its parameter; 1e20 (v = inf) did not move it
    zero_grad = [0, 1, 2] if mode == DECOUPLED else [0, 1]                    # Adam folds wd * p into the gradient: only p = +-0 stays out
    for k in (1, 2):
        np.testing.assert_array_equal(got[k][zero_grad], 0.0)
    np.testing.assert_array_equal(got[0][:2], 0.0)
    if mode == DECOUPLED:                                                     # p moves only by the decay
        decayed = np.float32(p0[2])
        for _ in range(2):
            decayed = decayed - np.float32(lr) * np.float32(wd) * decayed
        np.testing.assert_allclose(got[0][2], decayed, rtol=RTOL, atol=ATOL[0])
        assert got[0][2] != p0[2]


# -------------------------------------------------------------------------------------------------- 6: plumbing, states checked
@by_class
def test_skipped_parameter_and_strided_gradient(hip, cls, mode):
    """Tensor 1 has no gradient in the second step: its p, m, v stay as the first step left them, and the third step uses the
    optimizer's step count for it too.  Tensor 2's gradient arrives as a transposed (strided) view."""
    sc = scenario("skip", mode)
    opt, params = make_opt(hip, cls, mode, sc)
    tr = Trace(sc)
    for s, grads in enumerate(sc.grads):
        feed(params, grads)
        params[2].grad = dev(np.ascontiguousarray(grads[2].T)).t()
        assert not params[2].grad.is_contiguous() and tuple(params[2].grad.shape) == sc.shapes[2]
        before = snapshot(opt, params)
        opt.step()
        tr.step()
        after = snapshot(opt, params)
        check(tr, after, f"skip {cls} step {tr.t}")
        if grads[1] is None:
            assert s == 1
            assert_same_bits([after[1]], [before[1]], "skipped")
            assert np.any(before[1][1] != 0)
    assert opt.t == 3


@by_class
def test_empty_tensor_in_the_middle_of_the_table(hip, cls, mode):
    """The C entry with sizes {300, 0, 2049} and null pointers in the empty tensor's slots: status 0, no block for it, its neighbours
    updated."""
    import torch
    from ctypes import POINTER, c_int64, c_void_p, cast
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr, load_hip_function
    sc = scenario("zero_mid", mode)
    sizes = sizes_of(sc.shapes)
    assert sizes == [300, 0, 2049] and adam_ref.plan(sizes) == (2048, 3)
    ps = [dev(a) for a in sc.p0]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    tr = Trace(sc)
    handle = load_hip_function("nnhipCreateFusedOptimizer")()
    assert handle

    def table(ts):
        return cast((c_void_p * 3)(*[t.data_ptr() if t.numel() else None for t in ts]), POINTER(c_void_p))

    try:
        for s, grads in enumerate(sc.grads):
            gd = [dev(g) for g in grads]
            tabs = [table(ps), table(gd), table(ms), table(vs)]
            assert all(not t[1] and t[0] and t[2] for t in tabs)
            rc = call_hip_function("nnhipFusedAdamWMultiTensorStep", handle, 3, *tabs, cast((c_int64 * 3)(*sizes), POINTER(c_int64)),
                                   sc.lr, sc.betas[0], sc.betas[1], sc.eps, sc.wd, s + 1, mode, 1.0, get_current_stream_ptr())
            assert rc == 0
            tr.step()
            check(tr, [[host(ps[i]), host(ms[i]), host(vs[i])] for i in range(3)], f"zero_mid {cls} step {tr.t}")
        torch.cuda.synchronize()
    finally:
        load_hip_function("nnhipDestroyFusedOptimizer")(handle)


@by_class
def test_grad_scale_and_device_divisor(hip, cls, mode):
    """grad_scale = 0.5 and a device divisor of 4: the references with the gradient scaled by 0.125, and bit for bit a run on
    gradients multiplied by 0.125 beforehand."""
    import torch
    sc = scenario("scale", mode)
    assert all(o == dict(grad_scale=0.125) for o in sc.over)
    opt, params = make_opt(hip, cls, mode, sc)
    opt.grad_scale = 0.5
    opt.grad_divisor = torch.full((1,), 4.0, dtype=torch.float32, device="cuda")
    plain, plain_params = make_opt(hip, cls, mode, sc)
    tr = Trace(sc)
    for grads in sc.grads:
        feed(params, grads)
        feed(plain_params, [g * np.float32(0.125) for g in grads])
        opt.step()
        plain.step()
        tr.step()
        check(tr, snapshot(opt, params), f"scale {cls} step {tr.t}")
    assert_same_bits(snapshot(opt, params), snapshot(plain, plain_params), "pre-multiplied")


# ------------------------------------------------------------------------------------- 7: device-side stepping, driven directly, eager
def step_pair(hip, cls, mode, name, actions=None, device_from=0):
    """A scenario on two optimizers: one host-stepped, one with use_device_step().  actions[s](opt): what changes before step s, applied
    to both.  The device-stepped one ends with the host-stepped one's bits; the host-stepped one follows the references."""
    sc = scenario(name, mode)
    assert adam_ref.plan(sizes_of(sc.shapes)) == (2048, 4)         # 4 blocks: the last one to finish is not always the same
    (h_opt, h_par), (d_opt, d_par) = make_opt(hip, cls, mode, sc), make_opt(hip, cls, mode, sc)
    tr = Trace(sc)
    for s, grads in enumerate(sc.grads):
        if s == device_from:
            d_opt.use_device_step()
            assert d_opt.device_step
        for opt in (h_opt, d_opt):
            if actions and actions.get(s):
                actions[s](opt)
        feed(h_par, grads)
        feed(d_par, grads)
        h_opt.step()
        d_opt.step()
        tr.step()
        hs = snapshot(h_opt, h_par)
        assert_same_bits(snapshot(d_opt, d_par), hs, f"{name} {cls} device-stepped, step {tr.t}")
        check(tr, hs, f"{name} {cls} step {tr.t}")
    assert not h_opt.device_step and h_opt.t == d_opt.t == tr.t
    return sc


@by_class
def test_device_stepping_24_steps(hip, cls, mode):
    """No host read between the steps; the bias corrections of steps 2..24 come from the previous launch's last block."""
    from neunet_hip import optim
    rng = np.random.default_rng(2303)
    shapes = adam_ref.DEV_SHAPES
    assert adam_ref.plan(sizes_of(shapes)) == (2048, 4)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    gs = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(24)]
    snaps = []
    for device in (False, True):
        params = make_params(hip, p0)
        opt = getattr(optim, cls)(params, lr=1e-3, weight_decay=1e-2)
        if device:
            opt.use_device_step()
        for grads in gs:
            feed(params, grads)
            opt.step()
        assert opt.t == 24 and opt.device_step == device
        snaps.append(snapshot(opt, params))
    assert_same_bits(snaps[1], snaps[0], "24 device-stepped steps")
    for i, x in enumerate(snaps[0]):
        assert not np.array_equal(x[0], p0[i]) and np.all(x[2] != 0)


@pytest.mark.parametrize("t0", [1000, 99990])
@by_class
def test_device_stepping_resumes_at_a_step(hip, cls, mode, t0):
    """A restored checkpoint: opt.t = t0 and non-zero m, v, then use_device_step() and 5 steps -- steps t0 + 1 .. t0 + 5."""
    sc = step_pair(hip, cls, mode, f"resume_{t0}")
    assert sc.t0 == t0 and len(sc.grads) == 5 and sc.m0 is not None


@by_class
def test_device_stepping_betas_change(hip, cls, mode):
    """Other betas for the third and fourth device-stepped step, then the first ones again: the bias corrections the previous step
    left were computed for other betas and must be dropped, both times."""
    def to(betas):
        def act(opt):
            opt.betas = betas
        return act

    sc = step_pair(hip, cls, mode, "dev_betas", {2: to((0.8, 0.99)), 4: to((0.9, 0.999))})
    assert [o.get("betas", sc.betas) for o in sc.over] == [(0.9, 0.999)] * 2 + [(0.8, 0.99)] * 2 + [(0.9, 0.999)] * 2


@by_class
def test_device_stepping_block_count_changes(hip, cls, mode):
    """The second launch has 2 blocks instead of 4 (the two-chunk tensor has no gradient), the third 4 again: the ticket picks the last
    block of each, and the counter advances by one per launch -- the steps after show it."""
    sc = step_pair(hip, cls, mode, "dev_blocks")
    assert [g[0] is None for g in sc.grads] == [False, True, False, False]
    assert adam_ref.plan(sizes_of(sc.shapes[1:])) == (2048, 2)


@by_class
def test_device_stepping_hyper_parameter_changes(hip, cls, mode):
    """opt.lr, opt.weight_decay and opt.grad_scale each change between two device-stepped steps and hold from the next step on; then a
    device divisor, and its value rewritten in place."""
    import torch
    divisors = {}

    def set_lr(opt):
        opt.lr = 3e-3

    def set_wd(opt):
        opt.weight_decay = 5e-2

    def set_scale(opt):
        opt.grad_scale = 0.5

    def set_divisor(opt):
        divisors[id(opt)] = opt.grad_divisor = torch.full((1,), 4.0, dtype=torch.float32, device="cuda")

    def rewrite_divisor(opt):
        assert opt.grad_divisor is divisors[id(opt)]
        opt.grad_divisor.fill_(2.0)

    sc = step_pair(hip, cls, mode, "dev_hyper", {1: set_lr, 2: set_wd, 3: set_scale, 4: set_divisor, 5: rewrite_divisor})
    assert sc.over[1:] == [dict(lr=3e-3), dict(lr=3e-3, wd=5e-2), dict(lr=3e-3, wd=5e-2, grad_scale=0.5),
                           dict(lr=3e-3, wd=5e-2, grad_scale=0.5 / 4.0), dict(lr=3e-3, wd=5e-2, grad_scale=0.5 / 2.0)]


# ------------------------------------------------------------------------------------------------------------------ 8: captured
def make_mlp3(hip, weights):
    """Three Linear layers: six parameters, so no backward launch can take the Adam update with it -- step() launches the
    multi-tensor kernel, in the eager loop and in the captured step."""
    import neunet_hip.nn as nn

    class MLP3(nn.Module):
        def __init__(self):
            super().__init__()
            self.l1, self.r1, self.l2, self.r2, self.l3 = nn.Linear(20, 16), nn.ReLU(), nn.Linear(16, 12), nn.ReLU(), nn.Linear(12, 4)

        def forward(self, x):
            return self.l3(self.r2(self.l2(self.r1(self.l1(x)))))

    model = MLP3()
    ps = model.parameters()
    assert len(ps) == 6
    for p, w in zip(ps, weights):
        assert tuple(p.data.shape) == w.shape
        p.data.copy_(dev(w))
    return model


@pytest.mark.parametrize("cls,kw", [("Adam", dict(weight_decay=1e-2)), ("AdamW", {})], ids=["Adam", "AdamW"])
def test_graph_replay_equals_eager(hip, cls, kw):
    """6 replays through GraphedTrainStep (step count, lr, weight decay and bias corrections from device memory) leave the p, m, v of 6
    eager host-stepped steps; then a new opt.lr between replays takes effect."""
    import neunet_hip.nn as nn
    from neunet_hip import optim
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    rng = np.random.default_rng(2305)
    warm, steps = 2, 6
    weights = [(rng.standard_normal(s) * 0.3).astype(np.float32) for s in ((16, 20), (1, 16), (12, 16), (1, 12), (4, 12), (1, 4))]
    data = [(rng.uniform(-1, 1, (8, 20)).astype(np.float32), rng.integers(0, 4, 8).astype(np.int32)) for _ in range(warm + steps + 1)]

    def make():
        model = make_mlp3(hip, weights)
        x = hip.Tensor(data[0][0], device="cuda", requires_grad=False)
        y = hip.Tensor(data[0][1], dtype=np.int32, device="cuda", requires_grad=False)
        loss_fn = nn.CrossEntropyLoss()

        def fb():
            loss = loss_fn(model(x), y)
            loss.backward()
            return loss

        return model, x, y, fb, getattr(optim, cls)(model.parameters(), lr=1e-2, **kw)

    def feed_batch(x, y, item):
        x.data.copy_(dev(item[0]))
        y.data.copy_(dev(item[1]))

    m0, x0, y0, fb0, opt0 = make()

    def eager(item):
        feed_batch(x0, y0, item)
        opt0.zero_grad()
        fb0()
        opt0.step()
        assert not opt0._stepped_in_backward and not opt0.device_step

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
        assert_same_bits(snapshot(opt1, m1.parameters()), want, "6 replays")
        for x, w in zip(want, weights):
            assert not np.array_equal(x[0], w) and np.any(x[1] != 0) and np.any(x[2] != 0)
        # an LR schedule between replays
        opt0.lr = opt1.lr = opt0.lr * 0.25
        eager(data[-1])
        feed_batch(x1, y1, data[-1])
        step()
        assert_same_bits(snapshot(opt1, m1.parameters()), snapshot(opt0, m0.parameters()), "replay after the LR change")
    finally:
        step.release()


# ------------------------------------------------------------------------------------------------------------------ 9: plan churn
CHURN_SIZES = [100, 700, 1300, 2048, 2049, 3000, 4100, 5000]
CHURN_SUBSETS = [(0,), (0, 1, 2), (3, 4), (0, 1, 2, 3, 4, 5, 6, 7), (7,), (1, 3, 5, 7), (0, 2, 4, 6), (5, 6, 7), (0, 1, 2, 3, 4, 5, 6), (2, 7)]


@by_class
def test_plan_churn(hip, cls, mode):
    """The set of parameters with a gradient differs at each of 10 steps, so every step uploads a new plan blob: the ring of 4 pinned
    staging buffers wraps twice and the device buffer is regrown after launches have used it.  No host synchronisation between the
    steps.  Every tensor ends where the steps it took part in, at the optimizer's step counts, put it (step32: up to 6 steps per
    tensor here, 10 step counts), and bit for bit where a run that synchronises after every step ends."""
    import torch
    from neunet_hip import optim
    assert len(CHURN_SUBSETS) == 10 and all(a != b for a, b in zip(CHURN_SUBSETS, CHURN_SUBSETS[1:]))
    assert any(len(s) == 1 for s in CHURN_SUBSETS) and any(len(s) == len(CHURN_SIZES) for s in CHURN_SUBSETS)
    # the blob: 4 pointer tables and the sizes (40 bytes per tensor), two int32 per block; the device buffer is regrown to twice the
    # bytes whenever a blob does not fit
    cap, regrown = 0, 0
    for sub in CHURN_SUBSETS:
        chunk, blocks = adam_ref.plan([CHURN_SIZES[i] for i in sub])
        assert chunk == 2048
        nbytes = 40 * len(sub) + 8 * blocks
        if nbytes > cap:
            regrown, cap = regrown + 1, 2 * nbytes
    assert regrown >= 3                                            # the first allocation and two regrowths
    rng = np.random.default_rng(2306)
    p0 = [rng.standard_normal(n).astype(np.float32) for n in CHURN_SIZES]
    gs = [{i: rng.standard_normal(CHURN_SIZES[i]).astype(np.float32) for i in sub} for sub in CHURN_SUBSETS]
    lr, wd = 1e-3, 1e-2

    def run(sync):
        params = make_params(hip, p0)
        opt = getattr(optim, cls)(params, lr=lr, weight_decay=wd)
        staged = [{i: dev(g) for i, g in step.items()} for step in gs]       # every upload before the first step
        torch.cuda.synchronize()
        for step in staged:
            for i, p in enumerate(params):
                p.grad = step.get(i)
            opt.step()
            if sync:
                torch.cuda.synchronize()
        return snapshot(opt, params)

    got = run(False)
    ref = [[a.copy(), np.zeros_like(a), np.zeros_like(a)] for a in p0]
    for s, step in enumerate(gs):
        for i, g in step.items():
            adam_ref.step32(mode, ref[i][0], g, ref[i][1], ref[i][2], s + 1, lr, (0.9, 0.999), 1e-8, wd)
    for i in range(len(CHURN_SIZES)):
        for k in range(3):
            np.testing.assert_allclose(got[i][k], ref[i][k], rtol=RTOL, atol=ATOL[k], err_msg=f"{NAMES[k]}[{i}]")
        assert not np.array_equal(got[i][0], p0[i])
    assert_same_bits(run(True), got, "synchronised after every step")
