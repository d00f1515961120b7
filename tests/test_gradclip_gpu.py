"""GPU: gradient clipping by global norm (ABI 226; csrc/grad_norm.hip) through the C ABI and through the Python layer, against the
float64 restatement of tests/gradclip_ref.py.

nnhipGradNormMultiTensor on every row of the case table (both chunk sizes, chunk edges, an empty tensor, 64 and 257 blocks, the
scalar-load path, the README MLP) for both norms, grad_scale 1 / 0.5, divisor_in none / 4, max_norm above / below the norm: the L2
norm inside the DERIVED bound (gradclip_ref.l2_rel_bound; the test prints what it measured) and bit-identical to the float32
emulation of the kernel's summation order, the max norm exact, the divisor word within 4 * 2^-24 of its float32 recomputation and
equal to divisor_in bit for bit when nothing clips.  The in-launch finish: three calls on the same buffers with new data each time
(a finisher that read stale slots would reproduce the previous value), then a repeat that must give the same bits.  NaN / inf / zero
/ empty edges, every refusal with the words untouched, nnhipScaleMultiTensor, the nine optimizers armed against the same class on
pre-divided gradients, the README MLP's waiting backward, a captured step, and nn.utils.clip_grad_norm_.

Measured on an MI355X: worst |L2 norm - float64| / float64 over the module 0.73 x 2^-24 (`[2048] * 64`, second refill) against derived
bounds of 10.5 x 2^-24 (2048-element chunks) and 17.5 x 2^-24 (16384-element chunks); every L2 word equal to the emulation's bits."""
import ctypes

import numpy as np
import pytest

import gradclip_ref as R

pytestmark = pytest.mark.gpu
EINVAL, EALIGN = -1, -2
OPTIMIZERS = ["Adam", "AdamW", "SGD", "Momentum", "RMSprop", "Adagrad", "Adadelta", "Adamax", "NAdam"]
NORMS = [R.NORM_L2, R.NORM_INF]
SENTINEL = np.float32(-7.25)
by_norm = pytest.mark.parametrize("norm_type", NORMS, ids=["l2", "inf"])
_worst = {"l2": (0.0, "")}


@pytest.fixture(scope="module")
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    yield neunet_hip
    print("\nworst |L2 norm - norm64| / norm64 over the module: %.2f x 2^-24 (%s)" % (_worst["l2"][0] / R.EPS, _worst["l2"][1]))


@pytest.fixture
def handle(hip):
    from neunet_hip import _lib
    opt = _lib.load_hip_function("nnhipCreateFusedOptimizer")()
    assert opt
    yield opt
    _lib.load_hip_function("nnhipDestroyFusedOptimizer")(opt)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                 # a copy: the shared test data stays read-only


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def ulps(a, b):
    """Distance in float32 steps between two arrays (finite values)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def divisor_close(div, norm_word, max_norm, d_in=None):
    """The divisor word against its float32 recomputation from the returned norm word: gradclip_ref.DIVISOR_RTOL."""
    want = float(R.divisor32(norm_word, max_norm, d_in))
    return abs(float(div) - want) <= R.DIVISOR_RTOL * want


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def device_grads(name, grads):
    """The case's gradients on the device; the first tensor of a case with an offset is a view that starts that many elements past
    a 16-byte boundary."""
    import torch
    _, _, offset = R.case(name)
    out = []
    for i, g in enumerate(grads):
        if i == 0 and offset:
            base = torch.zeros(g.size + 8, dtype=torch.float32, device="cuda")
            view = base[offset:offset + g.size]
            view.copy_(torch.from_numpy(g))
            assert view.data_ptr() % 16 == 4 * offset
            out.append(view)
        else:
            out.append(dev(g))
    return out


def tables(tensors):
    n = len(tensors)
    ptrs, sizes = (ctypes.c_void_p * max(1, n))(), (ctypes.c_int64 * max(1, n))()
    for i, t in enumerate(tensors):
        ptrs[i], sizes[i] = (t.data_ptr() if t.numel() else None), t.numel()
    return ptrs, sizes


def call_norm(opt, tensors, norm_type, max_norm, d_in, words, step=1, grad_scale=1.0):
    from neunet_hip import _lib
    ptrs, sizes = tables(tensors)
    return _lib.load_hip_function("nnhipGradNormMultiTensor")(
        opt, len(tensors), ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(sizes, ctypes.POINTER(ctypes.c_int64)), norm_type,
        max_norm, None if d_in is None else d_in.data_ptr(), step, grad_scale, words.data_ptr(), stream())


def call_scale(opt, tensors, divisor):
    from neunet_hip import _lib
    ptrs, sizes = tables(tensors)
    return _lib.load_hip_function("nnhipScaleMultiTensor")(
        opt, len(tensors), ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(sizes, ctypes.POINTER(ctypes.c_int64)),
        divisor.data_ptr(), stream())


def fresh_words():
    return dev(np.array([SENTINEL, SENTINEL, SENTINEL, 123.0], np.float32))


def check_words(w, grads, norm_type, max_norm, grad_scale, d_in, where):
    """The four words of one call against the restatement."""
    sizes = [g.size for g in grads]
    ref, ref_div, ref_flag = R.words64(grads, norm_type, max_norm, grad_scale, d_in)
    if norm_type == R.NORM_L2:
        err = abs(float(w[0]) - ref) / ref if ref else abs(float(w[0]))
        if err > _worst["l2"][0]:
            _worst["l2"] = (err, where)
        print(f"{where}: L2 {err / R.EPS:.2f} x 2^-24 off float64, bound {R.l2_rel_bound(sizes) / R.EPS:.1f} x 2^-24")
        assert err <= R.l2_rel_bound(sizes), where
        assert bits(w[0]) == bits(R.emulate_l2(grads, grad_scale, d_in)), where       # the summation order, bit for bit
    else:
        assert bits(w[0]) == bits(R.inf_norm32(grads, grad_scale, d_in)), where      # exact
    assert divisor_close(w[1], w[0], max_norm, d_in), where
    assert abs(float(w[1]) - ref_div) <= (R.DIVISOR_RTOL + R.l2_rel_bound(sizes)) * ref_div, where
    if ref + 1e-6 < max_norm * (1 - 1e-5):
        assert bits(w[1]) == bits(np.float32(1.0 if d_in is None else d_in)), where   # nothing clipped: divisor_in itself
    else:
        assert float(w[1]) > (1.0 if d_in is None else d_in), where
    assert w[2] == ref_flag == 0.0 and w[3] == np.float32(123.0), where


# ------------------------------------------------------------------------------------------------------------- the case table
@by_norm
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_table(hip, handle, name, norm_type):
    grads = R.make_grads(name, 0)
    tensors = device_grads(name, grads)
    four = dev(np.array([4.0], np.float32))
    for grad_scale in (1.0, 0.5):
        for d_in in (None, 4.0):
            base = R.norm64(grads, norm_type, grad_scale, d_in)
            for factor in (2.0, 0.3):                                            # max_norm above the norm, then below it
                words = fresh_words()
                rc = call_norm(handle, tensors, norm_type, factor * base, None if d_in is None else four, words, grad_scale=grad_scale)
                assert rc == 0
                check_words(host(words), grads, norm_type, factor * base, grad_scale, d_in,
                            f"{name} norm {norm_type} gs {grad_scale} d_in {d_in} max_norm {factor} x norm")
    for t, g in zip(tensors, grads):
        np.testing.assert_array_equal(host(t), g)                                # the gradients are only read


# --------------------------------------------------------------------------------------------- last arriver, stale data, reruns
@by_norm
@pytest.mark.parametrize("name", ["blocks64", "big_tail"])
def test_every_call_reduces_its_own_data(hip, handle, name, norm_type):
    """Three calls on the SAME buffers, refilled in place with other data (other magnitudes too) between them: every result is
    its own data's.  The slots and the ticket are reused from call to call, so a finisher that read stale slots, or a ticket that
    did not return to zero, shows as the previous call's value or as words never written.  A fourth call on unchanged data gives
    the third call's bits."""
    import torch
    tensors = device_grads(name, R.make_grads(name, 1))
    results = []
    for k, scale in ((1, 1.0), (2, 3.0), (3, 0.25)):
        grads = R.make_grads(name, k, scale)
        for t, g in zip(tensors, grads):
            t.copy_(torch.from_numpy(g))
        words = fresh_words()
        assert call_norm(handle, tensors, norm_type, 1.0, None, words) == 0
        w = host(words)
        check_words(w, grads, norm_type, 1.0, 1.0, None, f"{name} norm {norm_type} call {k}")
        results.append(w)
    assert len({r[0].tobytes() for r in results}) == 3
    words = fresh_words()
    assert call_norm(handle, tensors, norm_type, 1.0, None, words) == 0
    np.testing.assert_array_equal(bits(host(words)), bits(results[-1]))


# ------------------------------------------------------------------------------------------------------ non-finite, zero, empty
@by_norm
def test_nonfinite_zero_and_empty(hip, handle, norm_type):
    import torch
    name = "chunk_edges"                                                          # the last tensor's last chunk is a 1-element tail
    grads = R.make_grads(name, 2)
    four = dev(np.array([4.0], np.float32))
    tensors = device_grads(name, grads)
    tensors[-1][-1] = float("nan")
    words = fresh_words()
    assert call_norm(handle, tensors, norm_type, 1.0, None, words) == 0
    w = host(words)
    assert np.isnan(w[0]) and w[2] == 1.0 and np.isnan(w[1])
    tensors[-1][-1] = 0.5
    tensors[1][77] = float("-inf")
    words = fresh_words()
    assert call_norm(handle, tensors, norm_type, 1.0, four, words) == 0
    w = host(words)
    assert w[0] == np.inf and w[2] == 1.0 and w[1] == np.inf
    for t in tensors:
        t.zero_()
    words = fresh_words()
    assert call_norm(handle, tensors, norm_type, 1.0, four, words, grad_scale=0.5) == 0
    np.testing.assert_array_equal(bits(host(words)), bits([0.0, 4.0, 0.0, 123.0]))
    # nothing to reduce: the identity words, from one launch all the same
    empty = torch.zeros(0, dtype=torch.float32, device="cuda")
    for tensors_, d_in, want in (([], None, 1.0), ([], four, 4.0), ([empty, empty], four, 4.0)):
        words = fresh_words()
        assert call_norm(handle, tensors_, norm_type, 1.0, d_in, words) == 0
        np.testing.assert_array_equal(bits(host(words)), bits([0.0, want, 0.0, 123.0]))


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_words_untouched(hip, handle):
    import torch
    from neunet_hip import _lib
    f = _lib.load_hip_function("nnhipGradNormMultiTensor")
    a, b = dev(np.ones(8, np.float32)), dev(np.ones(8, np.float32))
    words, four = fresh_words(), dev(np.array([4.0, 4.0], np.float32))
    W, D, s = words.data_ptr(), four.data_ptr(), stream()

    def call(opt=handle, n=2, g=(a.data_ptr(), b.data_ptr()), sizes=(8, 8), norm=0, max_norm=1.0, d_in=None, step=1, w=W, null_tables=False):
        ptrs, sz = (ctypes.c_void_p * 2)(*g), (ctypes.c_int64 * 2)(*sizes)
        gp = None if null_tables else ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
        rc = f(opt, n, gp, ctypes.cast(sz, ctypes.POINTER(ctypes.c_int64)), norm, max_norm, d_in, step, 1.0, w, s)
        return rc, _lib.last_error()

    for kw, code, text in (
            (dict(opt=None), EINVAL, "null optimizer handle"), (dict(w=None), EINVAL, "null words"),
            (dict(sizes=(8, -1)), EINVAL, "negative size"), (dict(g=(a.data_ptr(), None)), EINVAL, "null tensor pointer"),
            (dict(null_tables=True), EINVAL, "null table"), (dict(n=-1), EINVAL, "n_tensors"),
            (dict(norm=2), EINVAL, "norm_type"), (dict(norm=-1), EINVAL, "norm_type"),
            (dict(max_norm=0.0), EINVAL, "max_norm"), (dict(max_norm=-2.0), EINVAL, "max_norm"), (dict(max_norm=float("nan")), EINVAL, "max_norm"),
            (dict(step=-1), EINVAL, "step"), (dict(step=0), EINVAL, "SetStep"),
            (dict(g=(a.data_ptr() + 2, b.data_ptr())), EALIGN, "misaligned"), (dict(w=W + 2), EALIGN, "misaligned"),
            (dict(d_in=D + 1), EALIGN, "misaligned")):
        rc, msg = call(**kw)
        assert rc == code and text in msg and "nnhipGradNormMultiTensor" in msg, (kw, rc, msg)
    # SetStep alone is not enough for step == 0; SetStep + SetHyper is, and then max_norm comes from words[3]
    assert _lib.load_hip_function("nnhipFusedOptimizerSetStep")(handle, 0, s) == 0
    assert call(step=0)[0] == EINVAL
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(host(words)), bits([SENTINEL, SENTINEL, SENTINEL, 123.0]))
    assert _lib.load_hip_function("nnhipFusedOptimizerSetHyper")(handle, 0.1, 0.0, 0.5, s) == 0
    assert call(step=0, max_norm=float("nan"), d_in=D)[0] == 0                   # the argument is ignored; grad_scale 0.5 is the handle's
    w = host(words)
    np.testing.assert_array_equal(bits(w), bits([0.125 * 4.0, R.divisor32(np.float32(0.5), 123.0, 4.0), 0.0, 123.0]))


# ------------------------------------------------------------------------------------------------------ nnhipScaleMultiTensor
@pytest.mark.parametrize("name", R.CASE_NAMES[:4] + ["misaligned"])
def test_scale_multi_tensor(hip, handle, name):
    grads = R.make_grads(name, 3)
    tensors = device_grads(name, grads)
    assert call_scale(handle, tensors, dev(np.array([1.0], np.float32))) == 0
    for t, g in zip(tensors, grads):
        np.testing.assert_array_equal(bits(host(t)), bits(g))                    # a divisor of 1 leaves the bits
    d = np.float32(3.7)
    assert call_scale(handle, tensors, dev(np.array([d], np.float32))) == 0
    for t, g in zip(tensors, grads):
        if g.size:
            assert ulps(host(t), g / d).max() <= 1


# ------------------------------------------------------------------------------------------------------------ optimizer parity
PARITY_SIZES = [2049, 5, 128]


@pytest.mark.parametrize("cls", OPTIMIZERS)
def test_armed_optimizer_equals_prescaled_gradients(hip, cls):
    """Three armed steps (the first two clip, the third does not) against the same class, unarmed, on gradients the host divided by
    the divisor word the armed run produced; tests/test_hip_parity.py case 6's tolerance.  Then clipping is switched off and the old
    words are overwritten with 1e30: the next step must not see them."""
    from neunet_hip import optim
    from neunet_hip.nn import Parameter
    rng = np.random.default_rng(226)
    p0 = [rng.standard_normal(n).astype(np.float32) for n in PARITY_SIZES]
    scales = (1.0, 0.5, 0.01, 1.0)
    gs = [[(rng.standard_normal(n) * s).astype(np.float32) for n in PARITY_SIZES] for s in scales]
    max_norm = 5.0
    assert R.norm64(gs[1], R.NORM_L2) > 2 * max_norm and R.norm64(gs[2], R.NORM_L2) < 0.5 * max_norm

    def make():
        params = [Parameter(hip.Tensor(a, device="cuda")) for a in p0]
        return params, getattr(optim, cls)(params)

    pa, armed = make()
    armed.max_grad_norm = max_norm
    divisors = []
    for k in range(3):
        for p, g in zip(pa, gs[k]):
            p.grad = dev(g)
        armed.step()
        norm, div, flag = host(armed.last_grad_norm)[0], host(armed._clip_words)[1], host(armed.last_grad_nonfinite)[0]
        ref = R.norm64(gs[k], R.NORM_L2)
        assert abs(norm - ref) <= R.l2_rel_bound(PARITY_SIZES) * ref and flag == 0.0
        assert divisor_close(div, norm, max_norm)
        assert (div > 1.0) == (k < 2) and (k < 2 or bits(div) == bits(1.0))
        divisors.append(np.float32(div))
    pb, plain = make()
    for k in range(3):
        for p, g in zip(pb, gs[k]):
            p.grad = dev(g / divisors[k])
        plain.step()
    for a, b, start in zip(pa, pb, p0):
        np.testing.assert_allclose(host(a.data), host(b.data), rtol=2e-6, atol=2e-7)
        assert not np.array_equal(host(a.data), start)
    # switched off again: the handle must not keep pointing at the word
    armed.max_grad_norm = None
    armed._clip_words.fill_(1e30)
    for p, q, g in zip(pa, pb, gs[3]):
        p.grad, q.grad = dev(g), dev(g)
    before = [host(p.data).copy() for p in pa]
    armed.step()
    plain.step()
    for a, b, c in zip(pa, pb, before):
        np.testing.assert_allclose(host(a.data), host(b.data), rtol=2e-6, atol=2e-7)
        assert np.abs(host(a.data) - c).max() > 1e-6                              # a divisor of 1e30 would have frozen the parameters


# ------------------------------------------------------------------------------------------------------------- the README MLP
def test_readme_mlp_backward_waits_then_runs_plain(hip):
    """tests/test_hip_parity.py's README MLP: its backward launch waits for step() to take the Adam update along.  The norm needs
    every gradient before any update: armed before backward(), the backward does not wait at all; armed between backward() and
    step(), step() runs the waiting launch plainly, then norm + update.  Both leave the parameters of a run whose gradients were
    read between backward() and step()."""
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    rng = np.random.default_rng(23)
    X = rng.uniform(-1, 1, (32, 784)).astype(np.float32)
    Y = rng.integers(0, 10, 32).astype(np.int32)

    def build(arm=True):
        np.random.seed(5)

        class MLP(nn.Module):
            def __init__(self):
                super().__init__()
                self.l1, self.relu, self.l2 = nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)

            def forward(self, x):
                return self.l2(self.relu(self.l1(x)))

        m = MLP()
        opt = Adam(m.parameters(), lr=1e-2)
        opt.max_grad_norm = 0.05 if arm else None
        return m, m.parameters(), opt

    def backward(m):
        loss = nn.CrossEntropyLoss()(m(hip.Tensor(X, device="cuda", requires_grad=False)),
                                     hip.Tensor(Y, dtype=np.int32, device="cuda", requires_grad=False))
        loss.backward()

    m1, ps1, opt1 = build(arm=False)
    backward(m1)
    assert all(p._pending is not None for p in ps1)                               # the launch waits for step() ...
    opt1.max_grad_norm = 0.05                                                     # ... and clipping is armed meanwhile
    assert not opt1.can_fuse_into_backward()
    opt1.step()
    assert all(p._pending is None for p in ps1)
    m4, ps4, opt4 = build()
    backward(m4)
    assert all(p._pending is None for p in ps4)                                   # armed before backward(): nothing waits
    opt4.step()
    m2, ps2, opt2 = build()
    backward(m2)
    grads = [host(p.grad).copy() for p in ps2]                                    # the read: the eager path
    opt2.step()
    for a, b, c in zip(ps1, ps2, ps4):
        np.testing.assert_array_equal(host(a.data), host(b.data))
        np.testing.assert_array_equal(host(c.data), host(b.data))
    for p, g in zip(ps1, grads):
        np.testing.assert_array_equal(host(p.grad), g)
    ref = R.norm64(grads, R.NORM_L2)
    sizes = [g.size for g in grads]
    assert sorted(sizes) == sorted(R.MLP_SIZES)
    norm, div = host(opt1.last_grad_norm)[0], host(opt1._clip_words)[1]
    assert abs(norm - ref) <= R.l2_rel_bound(sizes) * ref
    assert ref > 0.05 and div > 1.0 and divisor_close(div, norm, 0.05)
    # ... and the update really was the clipped one: an unarmed Adam on the pre-divided gradients
    m3, ps3, opt3 = build(arm=False)
    for p, g in zip(ps3, grads):
        p.grad = dev(g / np.float32(div))
    opt3.step()
    for a, b in zip(ps1, ps3):
        np.testing.assert_allclose(host(a.data), host(b.data), rtol=2e-6, atol=2e-7)


# --------------------------------------------------------------------------------------------------------------- graph capture
@pytest.mark.parametrize("cls", ["Adam", "RMSprop"])
def test_captured_step_clips(hip, golden, cls):
    """A GraphedTrainStep of the two-layer MLP with clipping armed: two replays on refilled inputs leave the bits of two eager steps;
    a new max_grad_norm between replays reaches the next replay (word 3, a stream-ordered fill); the graph is kernels only."""
    import neunet_hip.nn as nn
    from neunet_hip import optim
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from test_optim_gpu import make_mlp
    g = golden("mlp_optim_rules")
    rng = np.random.default_rng(2260)
    warm, steps = 2, 2
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

        opt = getattr(optim, cls)(model.parameters())
        opt.max_grad_norm = 0.02
        return model, x, y, fb, opt

    def feed_batch(x, y, item):
        x.data.copy_(dev(item[0]))
        y.data.copy_(dev(item[1]))

    def state(model, opt):
        return [host(p.data) for p in model.parameters()] + [host(opt._clip_words)]

    m0, x0, y0, fb0, opt0 = make()

    def eager(item):
        feed_batch(x0, y0, item)
        opt0.zero_grad()
        fb0()
        opt0.step()
        assert not opt0.device_step

    for item in data[:warm + steps]:
        eager(item)
    want = state(m0, opt0)
    assert want[-1][1] > 1.0 and want[-1][2] == 0.0                              # the last step clipped

    m1, x1, y1, fb1, opt1 = make()
    warm_items = iter(data[:warm])

    def fb_warm():
        item = next(warm_items, None)
        if item is not None:
            feed_batch(x1, y1, item)
        return fb1()

    step = GraphedTrainStep(fb_warm, opt1, GradBucket(m1.parameters()), warmup=warm, count_nodes=True)
    try:
        assert opt1.device_step and step.mode == "single"
        assert step.kernel_nodes is not None and step.kernel_nodes == step.graph_nodes       # no memset, no memcpy node
        for item in data[warm:warm + steps]:
            feed_batch(x1, y1, item)
            step()
        got = state(m1, opt1)
        for a, b in zip(got[:-1], want[:-1]):
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(got[-1][:3]), bits(want[-1][:3]))
        # a new max_grad_norm between replays
        opt0.max_grad_norm = opt1.max_grad_norm = 0.25 * 0.02
        eager(data[-1])
        feed_batch(x1, y1, data[-1])
        step()
        got, want = state(m1, opt1), state(m0, opt0)
        for a, b in zip(got[:-1], want[:-1]):
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(got[-1][:3]), bits(want[-1][:3]))
        assert got[-1][3] == np.float32(0.005) and divisor_close(got[-1][1], got[-1][0], 0.005)
    finally:
        step.release()


# ------------------------------------------------------------------------------------------------------------------ nn.utils
@by_norm
def test_nn_utils_clip_grad_norm(hip, norm_type):
    import torch
    from neunet_hip.nn import Parameter, utils
    rng = np.random.default_rng(2261)
    shapes = [(7, 5), (2049,), (3,), (4, 4)]
    params = [Parameter(hip.Tensor(rng.standard_normal(s).astype(np.float32), device="cuda")) for s in shapes]
    grads = [rng.standard_normal(s).astype(np.float32) for s in shapes[:3]]
    params[0].grad = dev(grads[0].T.copy()).t()                                   # a strided gradient
    assert not params[0].grad.is_contiguous()
    params[1].grad, params[2].grad = dev(grads[1]), dev(grads[2])                 # params[3] has no gradient: skipped
    torch_type = 2.0 if norm_type == R.NORM_L2 else float("inf")
    sizes = [g.size for g in grads]
    ref = R.norm64(grads, norm_type)
    got = host(utils.get_grad_norm(params, torch_type))
    assert got.shape == (1,) and abs(got[0] - ref) <= R.l2_rel_bound(sizes) * ref
    for max_norm in (2.0 * ref, 0.3 * ref):
        strided = params[0].grad
        before = [host(p.grad).copy() for p in params[:3]]
        norm = utils.clip_grad_norm_(params, max_norm, torch_type)
        assert norm.is_cuda and norm.shape == (1,) and bits(host(norm)) == bits(got)      # the norm BEFORE clipping
        now = R.norm64(before, norm_type)
        d = np.float32(R.divisor32(host(norm)[0], max_norm))
        assert abs(host(norm)[0] - now) <= R.l2_rel_bound(sizes) * now
        assert params[0].grad is strided and params[3].grad is None
        for p, b in zip(params[:3], before):
            assert ulps(host(p.grad), b / d).max() <= 1
            np.testing.assert_allclose(host(p.grad), b / R.divisor64(now, max_norm), rtol=R.DIVISOR_RTOL + R.l2_rel_bound(sizes) + 2 * R.EPS, atol=0)
    assert abs(host(utils.get_grad_norm(params, torch_type))[0] - 0.3 * ref) <= 1e-5 * ref      # clipped to max_norm
