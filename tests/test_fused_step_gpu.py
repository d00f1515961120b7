"""GPU: the three one-launch step kernels through the C ABI, every instance, edge and refusal, against tests/fused_step_ref.py.

  nnhipLinearReLULinearBackward[Adam|Fits]   gemm_small_mlp_bwd_kernel<NW> with sg_tile16_dz<NW, U> (csrc/gemm_small.hip)
  nnhipLinearCrossEntropyLoss                linear_ce_small_kernel<VEC, NW> with ce_epilogue's exchange and ticket paths (csrc/rowops.hip)
  nnhipBatchNorm2dLinearSigmoidMSE[Fits]     bn_linear_sigmoid_mse_kernel<8> (csrc/rowops.hip)

The case tables and bounds live in tests/fused_step_ref.py; tests/test_fused_step_ref.py proves on the CPU that the tables reach every
instance and that the float32 oracle sits well inside the bounds.  Here every operand of every call sits in a Buf (NaN on both sides),
`intact()` is asserted for inputs and outputs, and every case prints its largest error / bound ratio before it asserts (run with -s).

The Adam variant is held to no tolerance of its own: its gradients are the plain entry's bits, its p, m, v the bits
nnhipFusedAdamWMultiTensorStep leaves on those gradients (csrc/adam_device.h promises the same bits wherever adam1 is inlined); the
first host-stepped launch of each shape is also held to adam_ref.step64 at test_adam_golden's tolerances.  Its arrival barrier gives
up after 20 s and raises the device error word: an autouse fixture checks the word before and behind every Adam-variant case (the
tests named test_adam_*), and once it was found set every later one fails before it launches.  No case launches a shape the Adam
entry's Fits refuses.

The offset-channel case of the BatchNorm head (a channel with mean 100, standard deviation 0.01): Y is allowed 4 x what the float32
two-pass BatchNorm is off by on the CPU (1.6e-3; 0.69 % of the rms of Y) -- see tests/test_fused_step_ref.py."""
import ctypes
from ctypes import POINTER, c_int64, c_void_p, cast

import numpy as np
import pytest

import adam_ref
import fused_step_ref as F
from rowops_ref import cross_entropy
from test_gemm_tiers_gpu import Buf, call, check, counts, dot_bound_of, status
from test_rowops_tiers_gpu import close_bound, scaled_bound

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, EALIGN, EDEVICE = -1, -2, -5
SENTINEL = -7
_BOARD = {"broken": False}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def fn(name):
    from neunet_hip._lib import load_hip_function
    return load_hip_function(name)


def last_error():
    from neunet_hip._lib import last_error as le
    return le()


@pytest.fixture(autouse=True)
def device_error_word(request, hip):
    """The Adam variant's barrier reports a time-out through the library's device error word: 0 before and behind every such case."""
    adam = request.node.name.startswith("test_adam_")
    if adam:
        if _BOARD["broken"]:
            pytest.fail("an earlier Adam-variant case left the device error word set: not launching")
        assert fn("nnhipDeviceError")() == 0
    yield
    if adam:
        torch.cuda.synchronize()
        if fn("nnhipDeviceError")() != 0:
            _BOARD["broken"] = True
            text = last_error()
            fn("nnhipClearDeviceError")()
            pytest.fail("the device error word was set behind this case: " + text)


@pytest.fixture(scope="module")
def two_streams(hip):
    return torch.cuda.Stream(), torch.cuda.Stream()


def refused(code, fragment, name, *args):
    rc = status(name, *args)
    assert rc == code, (name, rc, last_error())
    assert fragment in last_error(), last_error()


def all_nan(*bufs):
    return all(bool(torch.isnan(b.whole).all()) for b in bufs)


def same_bits(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


# ==================================================================================================== MLP backward, plain entry
class Mlp:
    """The operands of one nnhipLinearReLULinearBackward[Adam] call, each in its own fenced allocation."""
    NAMES = ("dW2", "db2", "dW1", "db1")

    def __init__(self, shape, d):
        self.shape = rows, in1, hid, out2 = shape
        self.d = d
        self.inputs = [Buf(a) for a in d]
        self.out = dict(dW2=Buf(out2 * hid), db2=Buf(out2), dW1=Buf(hid * in1), db1=Buf(hid))

    def args(self):
        return [b.t for b in self.inputs] + [self.out[k].t for k in self.NAMES] + list(self.shape)

    def plain(self):
        call("nnhipLinearReLULinearBackward", *self.args())
        return self

    def host(self):
        return {k: self.out[k].host() for k in self.NAMES}

    def intact(self):
        return (all(b.intact() for b in self.inputs) and all(b.intact() for b in self.out.values())
                and all(np.array_equal(b.host(), np.asarray(a).reshape(-1), equal_nan=True) for b, a in zip(self.inputs, self.d)))

    def check(self, tag):
        ref = F.mlp_backward64(*self.d)
        bound, got = F.mlp_bounds(*self.d, ref), self.host()
        assert self.intact(), tag
        r = max(check(f"{tag} {k}", got[k], ref[k], bound[k]) for k in self.NAMES)
        print()
        return r


def mlp_id(c):
    fits, nw, u, tail, n = F.mlp_route(*c)
    return "x".join(map(str, c)) + f"-nw{nw}u{u}" + ("-tail" if tail else "")


@pytest.mark.parametrize("c", F.MLP_CASES, ids=mlp_id)
def test_mlp_backward_every_instance(hip, c):
    """Rows on both sides of every instance boundary, each with a geometry of whole tiles and ragged ones.  Run to run bit-identical; no
    launch through the GEMM dispatcher (the entry has no general path to fall back to)."""
    assert fn("nnhipLinearReLULinearBackwardFits")(*c, 0) == 1 and F.mlp_route(*c)[0]
    n0 = counts()
    m = Mlp(c, F.mlp_inputs(*c)).plain()
    m.check("mlp " + mlp_id(c))
    assert np.array_equal(counts(), n0)
    same_bits(Mlp(c, F.mlp_inputs(*c)).plain().host(), m.host(), "second run")


@pytest.mark.parametrize("where", ["W2_H", "dO_inf", "dO_nan"])
@pytest.mark.parametrize("c", [(37, 17, 17, 7), (100, 90, 50, 15), (128, 15, 50, 1), (200, 17, 17, 7)], ids=mlp_id)
def test_mlp_backward_special_values(hip, c, where):
    """NaN and +-inf in W2 and H (a few hidden units: the others stay finite and bounded), and in dO (every hidden unit sees them):
    NaN exactly where float64 has it, infinities equal.  A NaN in H closes the mask, as in the reference's `grad * (f_x > 0)`; an
    infinite dO W2 under a closed mask is NaN there (inf * 0), so hidden units whose H is 0 in the row of an infinite dO are NaN too."""
    rows, in1, hid, out2 = c
    X1, H, W2, dO = F.mlp_inputs(*c, seed=1)
    if where == "W2_H":
        W2[0, 1], W2[out2 - 1, 3], W2[0, hid - 1] = np.inf, -np.inf, np.nan
        H[0, 5], H[rows - 1, 6], H[rows // 2, 7] = np.nan, np.inf, np.nan
        H[:, 3] = np.abs(H[:, 3]) + 1.0                          # unit 3: an open mask in every row -- dZ is +-inf, nothing closes over it
    else:
        dO[0, 0] = np.inf if where == "dO_inf" else np.nan
        H[0, :4] = [0.0, -0.0, 1.0, 2.0]                         # closed and open masks under the infinite / NaN row
    m = Mlp(c, (X1, H, W2, dO)).plain()
    ref = F.mlp_backward64(X1, H, W2, dO)
    if where == "W2_H":
        assert np.isfinite(ref["dW1"]).any() and np.isnan(ref["dW1"]).any() and np.isinf(ref["dW2"]).any()
    else:
        assert np.isnan(ref["db1"][:2]).all() and (where == "dO_nan" or np.isinf(ref["db1"][2:4]).all())
    m.check(f"mlp special {where} " + mlp_id(c))


def test_mlp_backward_empty_batch(hip):
    """rows == 0: the four gradients are zero-filled, the inputs may be null."""
    in1, hid, out2 = 17, 33, 7
    out = dict(dW2=Buf(out2 * hid), db2=Buf(out2), dW1=Buf(hid * in1), db1=Buf(hid))
    call("nnhipLinearReLULinearBackward", None, None, None, None, *[out[k].t for k in Mlp.NAMES], 0, in1, hid, out2)
    for k, b in out.items():
        assert b.intact() and np.array_equal(b.host(), np.zeros(b.hi - b.lo, np.float32)), k


@pytest.mark.parametrize("c", F.MLP_FITS_GRID, ids=lambda c: "x".join(map(str, c)))
def test_mlp_backward_fits_agrees_with_the_entry(hip, c):
    """Both sides of rows 256 | 257, out2 16 | 17, of gemm_small_wanted's tile limits for the dW2 and the dW1 GEMM, and of the rows <= 64
    relaxation: Fits, the restated rule and the entry agree; a refusal is NNHIP_EINVAL with the documented text and writes nothing."""
    want = F.mlp_route(*c)[0]
    assert fn("nnhipLinearReLULinearBackwardFits")(*c, 0) == int(want)
    m = Mlp(c, F.mlp_inputs(*c))
    if want:
        m.plain().check("mlp fits " + "x".join(map(str, c)))
    else:
        refused(EINVAL, "outside the small-problem range (rows <= 256, out2 <= 16)", "nnhipLinearReLULinearBackward", *m.args())
        assert all_nan(*m.out.values()) and m.intact()


def test_mlp_backward_refusals(hip):
    c = (37, 17, 17, 7)
    m = Mlp(c, F.mlp_inputs(*c))
    a = m.args()
    for i in range(4, 8):
        refused(EINVAL, "null output", "nnhipLinearReLULinearBackward", *a[:i], None, *a[i + 1:])
    for i in range(4):
        refused(EINVAL, "null input", "nnhipLinearReLULinearBackward", *a[:i], None, *a[i + 1:])
    for i in (0, 3, 4, 7):
        refused(EALIGN, "misaligned pointer", "nnhipLinearReLULinearBackward", *a[:i], a[i].data_ptr() + 2, *a[i + 1:])
    for bad in ((-1, 17, 17, 7), (37, 0, 17, 7), (37, 17, 0, 7), (37, 17, 17, 0)):
        refused(EINVAL, "bad sizes", "nnhipLinearReLULinearBackward", *a[:8], *bad)
    assert all_nan(*m.out.values()) and m.intact()
    assert fn("nnhipLinearReLULinearBackwardFits")(0, 17, 17, 7, 0) == 0


# ==================================================================================================== MLP backward with Adam inside
def table(tensors):
    return cast((c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]), POINTER(c_void_p))


class Handle:
    """An optimizer handle; device stepping starts at `t0` steps done."""

    def __init__(self, axes, t0=None, lr=F.ADAM_LR):
        from neunet_hip._lib import call_hip_function
        self.mode, self.wd, self.step, self.scale, div = axes
        self.lr = lr
        self.h = fn("nnhipCreateFusedOptimizer")()
        assert self.h
        self.div = None
        if div is not None:
            self.div = torch.full((1,), div, dtype=torch.float32, device="cuda")
            call_hip_function("nnhipFusedOptimizerSetGradDivisor", self.h, self.div)
        if t0 is not None:
            call("nnhipFusedOptimizerSetStep", self.h, t0)
            call("nnhipFusedOptimizerSetHyper", self.h, self.lr, self.wd, self.scale)

    def hyper(self, step):
        return (self.lr, F.ADAM_BETAS[0], F.ADAM_BETAS[1], F.ADAM_EPS, self.wd, step, self.mode, self.scale)

    def close(self):
        fn("nnhipDestroyFusedOptimizer")(self.h)


class AdamMlp(Mlp):
    """Mlp plus {p, m, v} x {W2, b2, W1, b1}; p of W2 IS the W2 operand."""

    def __init__(self, shape, seed=0):
        super().__init__(shape, F.mlp_inputs(*shape, seed=seed))
        p, m, v = F.adam_state(*shape, seed=seed)
        self.state0 = ([self.d[2]] + p[1:], m, v)
        self.p = [self.inputs[2]] + [Buf(a) for a in p[1:]]
        self.m, self.v = [Buf(a) for a in m], [Buf(a) for a in v]
        self.pmv = table([b.t for i in range(4) for b in (self.p[i], self.m[i], self.v[i])])
        self.sizes = cast((c_int64 * 4)(*[b.hi - b.lo for b in self.p]), POINTER(c_int64))

    def fused(self, handle, step):
        assert fn("nnhipLinearReLULinearBackwardFits")(*self.shape, 1) == 1 and F.mlp_route(*self.shape, with_adam=True)[0]
        call("nnhipLinearReLULinearBackwardAdam", *self.args(), handle.h, self.pmv, *handle.hyper(step))
        return self

    def two_launches(self, handle, step):
        """The decomposition: the plain entry, then the multi-tensor Adam step on its gradients."""
        self.plain()
        call("nnhipFusedAdamWMultiTensorStep", handle.h, 4, table([b.t for b in self.p]), table([self.out[k].t for k in self.NAMES]),
             table([b.t for b in self.m]), table([b.t for b in self.v]), self.sizes, *handle.hyper(step))
        return self

    def host(self):
        out = super().host()
        for i, name in enumerate(("W2", "b2", "W1", "b1")):
            out.update({"p_" + name: self.p[i].host(), "m_" + name: self.m[i].host(), "v_" + name: self.v[i].host()})
        return out

    def intact(self):
        X1, H, _, dO = self.inputs
        ok = all(b.intact() for b in (X1, H, dO) + tuple(self.out.values()) + tuple(self.p) + tuple(self.m) + tuple(self.v))
        return ok and all(np.array_equal(b.host(), np.asarray(a).reshape(-1)) for b, a in ((X1, self.d[0]), (H, self.d[1]), (dO, self.d[3])))


def adam_pair(shape, axes, launches=1, seed=0):
    """`launches` consecutive launches of the fused entry and of its decomposition on equal operands, each with a handle of its own."""
    _, wd, step, _, _ = axes
    t0 = 4 if step == 0 else None
    hf, hr = Handle(axes, t0), Handle(axes, t0)
    try:
        f, r = AdamMlp(shape, seed), AdamMlp(shape, seed)
        for i in range(launches):
            f.fused(hf, step + i if step else 0)
            r.two_launches(hr, step + i if step else 0)
        torch.cuda.synchronize()
        return f, r, f.host(), r.host()
    finally:
        hf.close()
        hr.close()


@pytest.mark.parametrize("axes", F.ADAM_AXES, ids=lambda a: f"mode{a[0]}-wd{a[1]}-step{a[2]}-scale{a[3]}-div{a[4]}")
@pytest.mark.parametrize("shape", F.MLP_ADAM_SHAPES, ids=lambda s: "x".join(map(str, s)) + f"-n{F.mlp_route(*s)[4]}")
def test_adam_inside_equals_backward_then_step(hip, shape, axes):
    """Gradients: the plain entry's bits.  p, m, v: nnhipFusedAdamWMultiTensorStep's bits on those gradients -- both decay modes, with
    and without weight decay, host stepping at steps 1 and 7, device stepping for 3 launches in a row (the stepper block commits, the next
    launch reads it), grad_scale with and without a device divisor.  n = 2, 27, 28, 29, 56, 57 check-in blocks around the 28 words of the
    arrival board; everything ragged at n = 27."""
    mode, wd, step, scale, div = axes
    launches = 3 if step == 0 else 1
    f, r, got, want = adam_pair(shape, axes, launches)
    assert f.intact() and r.intact()
    same_bits(got, want, f"{shape} {axes}")
    for k in got:
        if k[:2] in ("p_", "m_", "v_"):
            assert not np.array_equal(got[k], np.asarray(f.state0["pmv".index(k[0])][("W2", "b2", "W1", "b1").index(k[2:])]).reshape(-1)), k + " did not move"
    if step:                                                     # anchored: one host-stepped launch against adam_ref.step64
        worst = [0.0, 0.0, 0.0]
        for i, name in enumerate(("W2", "b2", "W1", "b1")):
            p, m, v = (np.asarray(f.state0[k][i], np.float64).copy() for k in range(3))
            g = got["d" + name].astype(np.float64).reshape(p.shape)
            adam_ref.step64(mode, p, g, m, v, step, F.ADAM_LR, F.ADAM_BETAS, F.ADAM_EPS, wd, scale / (div or 1.0))
            for k, (key, x) in enumerate((("p_", p), ("m_", m), ("v_", v))):
                worst[k] = max(worst[k], adam_ref.worst_ratio(got[key + name], x.reshape(-1), adam_ref.ATOL[k]))
                np.testing.assert_allclose(got[key + name], x.reshape(-1), rtol=adam_ref.RTOL, atol=adam_ref.ATOL[k], err_msg=key + name)
        print(f"[adam {shape} {axes}] vs step64: worst ratio p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")
    if launches == 1:                                            # (a later launch differentiates through the updated W2)
        r.check(f"adam {shape} gradients")


@pytest.mark.parametrize("device", [False, True], ids=["host-stepped", "device-stepped"])
def test_adam_back_to_back_launches_of_different_grids(hip, device):
    """n = 57, 2, 28, 57 on one stream with no synchronisation in between: the closer of each launch clears the other bank for the next
    one, whatever its size.  Each launch equals its decomposition."""
    axes = (1, 1e-2, 0 if device else 3, 1.0, None)
    hf, hr = Handle(axes, 9 if device else None), Handle(axes, 9 if device else None)
    try:
        fs = [AdamMlp(F.MLP_ADAM_SHAPES[i], seed=k) for k, i in enumerate(F.MLP_ADAM_SEQUENCE)]
        rs = [AdamMlp(F.MLP_ADAM_SHAPES[i], seed=k) for k, i in enumerate(F.MLP_ADAM_SEQUENCE)]
        torch.cuda.synchronize()
        for k, f in enumerate(fs):
            f.fused(hf, 0 if device else 3 + k)
        for k, r in enumerate(rs):
            r.two_launches(hr, 0 if device else 3 + k)
        torch.cuda.synchronize()
        for k, (f, r) in enumerate(zip(fs, rs)):
            assert f.intact() and r.intact()
            same_bits(f.host(), r.host(), f"launch {k} {f.shape}")
        assert not np.array_equal(fs[0].host()["p_W1"], fs[3].host()["p_W1"])        # (another seed, another step)
    finally:
        hf.close()
        hr.close()


def test_adam_graph_replay_equals_eager(hip):
    """One capture of a device-stepped ragged launch, replayed 3 times (an odd count: the bank parity differs from capture to capture)
    against 3 eager launches."""
    shape, axes = F.MLP_ADAM_SHAPES[1], (1, 1e-2, 0, 1.0, None)
    he, hg = Handle(axes, 2), Handle(axes, 2)
    try:
        e, g = AdamMlp(shape), AdamMlp(shape)
        for _ in range(3):
            e.fused(he, 0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g.fused(hg, 0)
        torch.cuda.synchronize()
        assert np.array_equal(g.p[2].host(), np.asarray(g.state0[0][2]).reshape(-1))  # captured, not run
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        assert e.intact() and g.intact()
        same_bits(g.host(), e.host(), "3 replays")
        del graph
    finally:
        he.close()
        hg.close()


def test_adam_refusals(hip):
    shape, axes = (37, 120, 40, 7), (1, 1e-2, 1, 1.0, None)
    name = "nnhipLinearReLULinearBackwardAdam"
    h = Handle(axes)
    fresh = fn("nnhipCreateFusedOptimizer")()
    try:
        m = AdamMlp(shape)
        before = m.host()
        a, hy = m.args(), h.hyper(1)
        other = Buf(shape[3] * shape[2])
        wrong = table([other.t] + [b.t for i in range(4) for b in (m.p[i], m.m[i], m.v[i])][1:])
        refused(EINVAL, "pmv[0] must be W2", name, *a, h.h, wrong, *hy)
        holed = cast((c_void_p * 12)(*[None if i == 7 else m.pmv[i] for i in range(12)]), POINTER(c_void_p))
        refused(EINVAL, "null / misaligned optimizer tensor", name, *a, h.h, holed, *hy)
        refused(EINVAL, "decay_mode must be 0 or 1", name, *a, h.h, m.pmv, *hy[:6], 2, hy[7])
        refused(EINVAL, "bad sizes", name, *a[:8], 0, *shape[1:], h.h, m.pmv, *hy)
        refused(EINVAL, "step == 0 needs nnhipFusedOptimizerSetStep and SetHyper first", name, *a, fresh, m.pmv, *hy[:5], 0, *hy[6:])
        big = (64, 16, 16384, 1)                                 # 1025 pollers: beyond half of any chip's resident blocks
        assert fn("nnhipLinearReLULinearBackwardFits")(*big, 0) == 1 and fn("nnhipLinearReLULinearBackwardFits")(*big, 1) == 0
        # a sticky device error: the entry answers NNHIP_EDEVICE and launches nothing
        call("nnhipRaiseDeviceErrorForTest", 1)
        torch.cuda.synchronize()
        try:
            assert fn("nnhipDeviceError")() == EDEVICE
            refused(EDEVICE, "device error", name, *a, h.h, m.pmv, *hy)
        finally:
            fn("nnhipClearDeviceError")()
        assert fn("nnhipDeviceError")() == 0
        torch.cuda.synchronize()
        same_bits(m.host(), before, "a refused call wrote")
        assert all_nan(*m.out.values()) and m.intact()
    finally:
        h.close()
        fn("nnhipDestroyFusedOptimizer")(fresh)


# ==================================================================================================== Linear + CrossEntropy
LABEL_TYPES = {2: (np.int16, torch.int16), 4: (np.int32, torch.int32), 8: (np.int64, torch.int64)}


class LinCe:
    """The inputs of a case on the device, once; run() makes one call into fresh fenced outputs."""

    def __init__(self, c, seed=0):
        self.c = self.rows, self.K, self.classes, ox, ow = c
        self.X, self.W, self.b, self.cw, self.y = F.lince_inputs(self.rows, self.K, self.classes, seed)
        self.x, self.w, self.bb, self.cwd = Buf(self.X, ox), Buf(self.W, ow), Buf(self.b), Buf(self.cw)
        self.labels = {nb: torch.from_numpy(self.y.astype(t[0])).cuda() for nb, t in LABEL_TYPES.items()}
        self.ign = F.lince_ignore(self.classes)

    def outputs(self):
        r, c = self.rows, self.classes
        return dict(logits=Buf(r * c), dlogits=Buf(r * c), loss_rows=Buf(r), lse=Buf(r), loss=Buf(1))

    def launch(self, out, count, red, weighted, ign, lbytes=4, labels=None):
        call("nnhipLinearCrossEntropyLoss", self.x.t, self.w.t, self.bb.t, out["logits"].t, out["dlogits"].t, out["loss_rows"].t, out["lse"].t,
             self.labels[lbytes] if labels is None else labels, lbytes, self.cwd.t if weighted else None, ign, self.rows, self.K, self.classes,
             red.encode(), out["loss"].t, None if count is None else count[1:2])

    def run(self, red, weighted, ign, lbytes=4, with_count=True, labels=None):
        out = self.outputs()
        count = torch.full((3,), SENTINEL, device="cuda", dtype=torch.int32) if with_count else None
        self.launch(out, count, red, weighted, ign, lbytes, labels)
        got = {k: b.host() for k, b in out.items()}
        got["count"] = None if count is None else count.cpu().numpy()
        assert all(b.intact() for b in out.values()) and self.inputs_intact()
        return got

    def inputs_intact(self):
        return (all(b.intact() for b in (self.x, self.w, self.bb, self.cwd)) and np.array_equal(self.x.host(), self.X.reshape(-1))
                and np.array_equal(self.w.host(), self.W.reshape(-1)))

    def separate_logits(self):
        z = Buf(self.rows * self.classes)
        n0 = counts()
        call("nnhipLinearModuleForward", self.x.t, self.w.t, self.bb.t, z.t, self.rows, self.K, self.classes)
        assert np.array_equal(counts() - n0, [0, 0, 1, 0]) and z.intact()           # the small family: the tile code the fused kernel promises
        return z.host()

    def check(self, tag, got, z32, red, weighted, ign, y=None):
        """logits: the separate entry's bits; the loss outputs against float64 on those float32 logits."""
        rows, classes = self.rows, self.classes
        assert np.array_equal(got["logits"], z32), tag + ": logits differ from nnhipLinearModuleForward's"
        loss_rows, lse, loss, dl, n = cross_entropy(z32.reshape(rows, classes), self.y if y is None else y, self.cw if weighted else None, ign, red)
        shares = dict(loss_rows=np.max(np.abs(got["loss_rows"] - loss_rows) / close_bound(loss_rows, 1e-5, 1e-5)),
                      lse=np.max(np.abs(got["lse"] - lse) / close_bound(lse, 1e-5, 1e-5)),
                      dlogits=np.max(np.abs(got["dlogits"].reshape(rows, classes) - dl) / scaled_bound(dl)))
        if red != "n" and np.isnan(loss):                                       # 'mean' over no live row (0 / 0 in float64): the entry answers 0
            assert n == 0 and got["loss"][0] == 0, tag
        elif red != "n":
            shares["loss"] = float(abs(got["loss"][0] - loss) / close_bound(loss, 1e-5, 1e-5))
        print(f"[{tag} {red}{' weighted' if weighted else ''} ignore {ign}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
        assert all(v <= 1.0 for v in shares.values()), (tag, shares)
        if red == "n":
            assert np.isnan(got["loss"][0]), tag + ": 'n' wrote loss_out"
        if got["count"] is not None:
            assert got["count"][0] == SENTINEL and got["count"][2] == SENTINEL
            assert got["count"][1] == (n if red == "m" else SENTINEL), tag + f": count_out {got['count'][1]}, {n} live rows"
        inert = np.all(dl == 0, axis=1)
        assert np.all(got["dlogits"].reshape(rows, classes)[inert] == 0) and np.all(got["loss_rows"][inert] == 0), tag + ": an inert row is not zero"
        return max(shares.values())


@pytest.mark.parametrize("c", F.LINCE_CASES, ids=F.lince_id)
def test_linear_ce_every_instance(hip, c):
    """Every <VEC, NW> instance with one k-group per wave and with several; class counts that leave the second 16-column tile ragged;
    1, 2, 3, 16 and 17 blocks.  Three reductions with and without class weights, an in-range ignore_index and -100; labels of -1 and
    `classes` are inert; int16 / int32 / int64 labels; count_out null and non-null."""
    run = LinCe(c)
    rows, K, classes = c[:3]
    z64, mag = F.logits64(run.X, run.W, run.b)
    z32 = run.separate_logits()
    r = check("linear-ce " + F.lince_id(c) + " logits", z32, z64, dot_bound_of(mag, z64))
    print()
    assert {-1, classes, -100} <= set(run.y.tolist()) or rows < 5
    worst = r
    for red, weighted, inrange in F.LINCE_RUNS:
        ign = run.ign if inrange else -100
        got = run.run(red, weighted, ign)
        worst = max(worst, run.check(F.lince_id(c), got, z32, red, weighted, ign))
    # the label types agree (same values, other loads), with and without count_out
    base = run.run("m", True, -100)
    for lbytes in (2, 8):
        got = run.run("m", True, -100, lbytes, with_count=lbytes == 8)
        run.check(F.lince_id(c) + f" int{8 * lbytes}", got, z32, "m", True, -100)
        same_bits({k: got[k] for k in ("dlogits", "loss_rows", "lse", "loss")}, {k: base[k] for k in ("dlogits", "loss_rows", "lse", "loss")},
                  f"int{8 * lbytes} labels")
    print(f"[linear-ce {F.lince_id(c)}] worst error / bound {worst:.3f}")


def test_linear_ce_every_label_ignored_under_mean(hip):
    """Every label ignored under 'mean': loss 0, gradient 0, loss rows 0, count 0 -- on one block, the exchange path's two and the
    ticket path; the same from nnhipCrossEntropyLossEx on the logits (the entry this one promises to equal).  ce_epilogue used to divide
    the sum of no losses by the count of no rows: NaN on an MI355X at 1 x 1 x 1, 32 x 64 x 10, 33 x 65 x 31 and 256 x 132 x 15."""
    for c in ((1, 1, 1, 0, 0), (32, 64, 10, 0, 0), (33, 65, 31, 0, 0), (256, 132, 15, 0, 0)):
        run = LinCe(c)
        lab = torch.from_numpy(np.full(run.rows, run.ign, np.int32)).cuda()
        for weighted in (False, True):
            got = run.run("m", weighted, run.ign, labels=lab)
            print(f"[linear-ce all ignored {F.lince_id(c)}] loss {got['loss'][0]}, count {got['count'][1]}, largest |dlogits| {np.abs(got['dlogits']).max()}")
            assert not got["dlogits"].any() and not got["loss_rows"].any() and got["count"][1] == 0
            assert got["loss"][0] == 0, f"{F.lince_id(c)}: loss {got['loss'][0]}"
        z = run.separate_logits()
        assert np.array_equal(got["logits"], z)
        zb, dl, lr, lse, loss = Buf(z), Buf(z.size), Buf(run.rows), Buf(run.rows), Buf(1)
        call("nnhipCrossEntropyLossEx", zb.t, dl.t, lr.t, lse.t, lab, 4, None, run.classes, run.ign, run.rows, run.classes, b"m", loss.t, None)
        assert loss.host()[0] == 0 and not dl.host().any() and all(x.intact() for x in (zb, dl, lr, lse, loss))


def test_linear_ce_back_to_back(hip):
    """2, 1, 16, 2 blocks, each call twice, no synchronisation in between: the exchange word of the two-block path and the ticket of the
    general one are left clean by every launch."""
    runs = [LinCe((rows, 64, 10, 0, 0), seed=i) for i, rows in enumerate(F.LINCE_SEQUENCE)]
    outs = [[r.outputs(), r.outputs()] for r in runs]
    cnts = [[torch.full((3,), SENTINEL, device="cuda", dtype=torch.int32) for _ in range(2)] for _ in runs]
    torch.cuda.synchronize()
    for r, o, c in zip(runs, outs, cnts):
        for k in range(2):
            r.launch(o[k], c[k], "m", True, -100)
    torch.cuda.synchronize()
    for r, o, c in zip(runs, outs, cnts):
        z32 = r.separate_logits()
        for k in range(2):
            got = {name: b.host() for name, b in o[k].items()}
            got["count"] = c[k].cpu().numpy()
            assert all(b.intact() for b in o[k].values())
            r.check(f"linear-ce sequence rows {r.rows} call {k}", got, z32, "m", True, -100)
        same_bits({n: b.host() for n, b in o[0].items()}, {n: b.host() for n, b in o[1].items()}, "second call")


def test_linear_ce_refusals(hip):
    name = "nnhipLinearCrossEntropyLoss"
    run = LinCe((33, 64, 17, 0, 0))
    out = run.outputs()
    lab = run.labels[4]

    def args(rows=33, K=64, classes=17, red=b"m", lbytes=4, loss="loss", over=None):
        a = [run.x.t, run.w.t, run.bb.t, out["logits"].t, out["dlogits"].t, out["loss_rows"].t, out["lse"].t, lab, lbytes, None, -100, rows, K,
             classes, red, None if loss is None else out[loss].t, None]
        for i, v in (over or {}).items():
            a[i] = v
        return a

    limits = "needs 1 <= rows <= 256, 1 <= classes <= 32, 1 <= in_features <= 2048"
    for kw in (dict(rows=0), dict(rows=257), dict(classes=0), dict(classes=33), dict(K=0), dict(K=2049)):
        refused(EINVAL, limits, name, *args(**kw))
    refused(EINVAL, "reduction must be 'n', 'm' or 's'", name, *args(red=b"x"))
    refused(EINVAL, "labels must be int16, int32 or int64", name, *args(lbytes=3))
    refused(EINVAL, "'m'/'s' need loss_out", name, *args(loss=None))
    refused(EINVAL, "'m'/'s' need loss_out", name, *args(red=b"s", loss=None))
    refused(EINVAL, "null or aliased pointer", name, *args(over={4: out["logits"].t}))
    for i in (0, 1, 3, 4, 5, 6, 7):
        refused(EINVAL, "null or aliased pointer", name, *args(over={i: None}))
    for i in (0, 1, 2, 3, 4):
        refused(EALIGN, "misaligned pointer", name, *args(over={i: args()[i].data_ptr() + 2}))
    torch.cuda.synchronize()
    assert all_nan(*out.values()) and run.inputs_intact()
    assert status(name, *args(red=b"n", loss=None)) == 0                         # 'n' needs no loss_out; b may be null
    assert status(name, *args(over={2: None})) == 0


# ==================================================================================================== BatchNorm -> Linear -> Sigmoid -> MSE
class BnHead:
    KEYS = ("Y", "mean", "inv", "rm", "rv", "pred", "dz", "loss")

    def __init__(self, c, offset_channel=False):
        self.c = self.B, self.C, self.HW, self.N, self.nstat, self.affine, self.running, self.bias = c
        self.d = d = F.bn_inputs(c, offset_channel)
        self.inp = {k: (None if d[k] is None else Buf(d[k])) for k in ("X", "stats", "g", "be", "W", "b", "T")}

    def outputs(self):
        B, C, HW, N = self.c[:4]
        out = dict(Y=Buf(B * C * HW), mean=Buf(C), inv=Buf(C), pred=Buf(B * N), dz=Buf(B * N), loss=Buf(1))
        if self.running:
            out["rm"], out["rv"] = Buf(np.full(C, F.BN_RM0, np.float32)), Buf(np.full(C, F.BN_RV0, np.float32))
        return out

    def args(self, out, over=None):
        t = lambda b: None if b is None else b.t                                # noqa: E731
        i = self.inp
        a = [t(i["X"]), t(i["stats"]), self.nstat, self.d["count"], t(i["g"]), t(i["be"]), out["Y"].t, out["mean"].t, out["inv"].t,
             t(out.get("rm")), t(out.get("rv")), self.B, self.C, self.HW, F.BN_EPS, F.BN_MOMENTUM, t(i["W"]), t(i["b"]), self.N, t(i["T"]),
             out["pred"].t, out["dz"].t, out["loss"].t]
        for k, v in (over or {}).items():
            a[k] = v
        return a

    def launch(self, out):
        call("nnhipBatchNorm2dLinearSigmoidMSE", *self.args(out))

    def intact(self, out):
        return (all(b.intact() for b in out.values()) and all(b is None or b.intact() for b in self.inp.values())
                and np.array_equal(self.inp["X"].host(), self.d["X"].reshape(-1)))

    def check(self, tag, out, y_bound=None):
        ref = F.bnhead64(self.d)
        bound = F.bnhead_bounds(self.d, ref, y_bound)
        assert self.intact(out), tag
        rs = {}
        for k in self.KEYS:
            if k not in out:
                continue
            got, want, b = out[k].host(), np.asarray(ref[k], np.float64).reshape(-1), np.broadcast_to(bound[k], np.shape(ref[k])).reshape(-1)
            rs[k] = check(f"{tag} {k}", got, want, b)
        print()
        return rs


@pytest.mark.parametrize("c", F.BN_CASES, ids=F.bn_id)
def test_bn_head_every_path(hip, c):
    """1, 2, 3..19 and 256 blocks; a float4 of the A operand inside one channel, across one boundary and (HW = 1) across three; large
    non-power-of-two HW; 1, 31..33, 256, 257 and 1024 statistics pairs; affine, running statistics and the Linear bias on and off.
    Called twice: the ticket is left clean, the second call's bits are the first's."""
    assert fn("nnhipBatchNorm2dLinearSigmoidMSEFits")(*c[:4]) == 1 and F.bnhead_route(*c[:5])[0]
    run = BnHead(c)
    outs = [run.outputs(), run.outputs()]
    for o in outs:
        run.launch(o)
    run.check("bn-head " + F.bn_id(c), outs[0])
    same_bits({k: b.host() for k, b in outs[0].items()}, {k: b.host() for k, b in outs[1].items()}, "second call")


def test_bn_head_offset_channel(hip):
    """A channel with mean 100 and standard deviation 0.01: Y within 4 x the float32 two-pass reference's own error (measured on the
    CPU, below 1 % of the rms), pred and dz with that carried through; the statistics of every channel at the usual bounds (the Chan
    merge of the float32 (mean, M2) pairs keeps the offset channel's save_inv to 3e-7 relative on an MI355X)."""
    dy, rms = F.bn_offset_allowance()
    assert 4 * dy < 0.01 * rms
    run = BnHead(F.BN_OFFSET_CASE, offset_channel=True)
    out = run.outputs()
    run.launch(out)
    rs = run.check("bn-head offset channel", out, y_bound=4 * dy)
    ref = F.bnhead64(run.d)
    print(f"[bn-head offset channel] Y error / (4 x float32 two-pass) {rs['Y']:.3f}; save_inv of the offset channel: relative error "
          f"{abs(out['inv'].host()[1] / ref['inv'][1] - 1):.2e}")


def test_bn_head_refusals(hip):
    name, fits = "nnhipBatchNorm2dLinearSigmoidMSE", fn("nnhipBatchNorm2dLinearSigmoidMSEFits")
    limits = "needs C <= 16, N <= 16, C*HW a multiple of 4 and <= 2048, B <= 4096"
    run = BnHead((32, 4, 5, 16, 32, True, True, True))
    out = run.outputs()
    a = run.args(out)
    # (B, C, HW, N) on both sides of each limit; the buffers above are never touched by a refused call
    for ok, bad in (((32, 16, 4, 16), (32, 17, 4, 16)), ((32, 4, 5, 16), (32, 4, 5, 17)), ((32, 16, 128, 16), (32, 4, 513, 16)),
                    ((32, 4, 5, 16), (32, 5, 5, 16)), ((4096, 4, 5, 16), (4097, 4, 5, 16))):
        assert fits(*ok) == 1 and fits(*bad) == 0 and F.bnhead_route(*ok, 1)[0] and not F.bnhead_route(*bad, 1)[0]
        B, C, HW, N = bad
        refused(EINVAL, limits, name, *run.args(out, {11: B, 12: C, 13: HW, 18: N}))
    assert fits(32, 4, 513, 16) == 0 and 4 * 513 == 2052
    refused(EINVAL, "the statistics pairs must cover B*HW values per channel", name, *run.args(out, {2: 31}))
    refused(EINVAL, "the statistics pairs must cover B*HW values per channel", name, *run.args(out, {3: run.d["count"] + 1}))
    refused(EINVAL, "go in pairs", name, *run.args(out, {4: None}))
    refused(EINVAL, "go in pairs", name, *run.args(out, {5: None}))
    refused(EINVAL, "go in pairs", name, *run.args(out, {9: None}))
    refused(EINVAL, "go in pairs", name, *run.args(out, {10: None}))
    for i in (0, 1, 6, 7, 8, 16, 19, 20, 21, 22):
        refused(EINVAL, "null pointer", name, *run.args(out, {i: None}))
    for i in (0, 16, 6):
        refused(EALIGN, "X, W, Y must be 16-byte aligned", name, *run.args(out, {i: a[i].data_ptr() + 4}))
    torch.cuda.synchronize()
    for k, b in out.items():
        assert b.intact() and (k in ("rm", "rv") or bool(torch.isnan(b.t).all())), k
    assert np.array_equal(out["rm"].host(), np.full(4, F.BN_RM0, np.float32))


# ==================================================================================================== two streams
def test_adam_alternating_streams(hip, two_streams):
    """The three entries share one set of library words (arrival board, ticket, exchange word) behind one StreamGuard (runtime.hip): the same
    call issued alternately on two streams leaves the single-stream bits."""
    shape, axes = F.MLP_ADAM_SHAPES[1], (1, 1e-2, 5, 1.0, None)
    h = Handle(axes)
    try:
        want = AdamMlp(shape).fused(h, 5)
        runs = [AdamMlp(shape) for _ in range(4)]
        torch.cuda.synchronize()
        for k, r in enumerate(runs):
            with torch.cuda.stream(two_streams[k % 2]):
                r.fused(h, 5)
        torch.cuda.synchronize()
        for k, r in enumerate(runs):
            assert r.intact()
            same_bits(r.host(), want.host(), f"launch {k} on stream {k % 2}")
    finally:
        h.close()


def test_linear_ce_alternating_streams(hip, two_streams):
    run = LinCe((32, 64, 10, 0, 0))                                              # two blocks: the exchange word
    want = run.run("m", True, -100)
    outs = [run.outputs() for _ in range(4)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        with torch.cuda.stream(two_streams[k % 2]):
            run.launch(o, None, "m", True, -100)
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert all(b.intact() for b in o.values())
        same_bits({n: b.host() for n, b in o.items()}, {n: want[n] for n in o}, f"launch {k} on stream {k % 2}")


def test_linear_ce_unreduced_call_between_reduced_ones(hip, two_streams):
    """Stream A reduced, stream B unreduced ('n': no loss output, no shared word), stream B reduced, stream A reduced, twice over
    with no host synchronisation.  The unreduced call must not count as a user of the shared words: it used to re-record the guard's
    event on B without becoming the last stream, and the reduced call behind it on B then waited for its own stream instead of A."""
    run = LinCe((32, 64, 10, 0, 0))                                              # two blocks: the exchange word
    want = {"m": run.run("m", True, -100), "n": run.run("n", True, -100)}
    a, b = two_streams
    seq = [(a, "m"), (b, "n"), (b, "m"), (a, "m")] * 2
    outs = [run.outputs() for _ in seq]
    torch.cuda.synchronize()
    for (st, red), o in zip(seq, outs):
        with torch.cuda.stream(st):
            run.launch(o, None, red, True, -100)
    torch.cuda.synchronize()
    for k, ((st, red), o) in enumerate(zip(seq, outs)):
        assert all(buf.intact() for buf in o.values())
        same_bits({n: buf.host() for n, buf in o.items()}, {n: want[red][n] for n in o}, f"launch {k} ('{red}' on stream {'AB'[st is b]})")


def test_bn_head_alternating_streams(hip, two_streams):
    run = BnHead((33, 2, 6, 16, 33, False, False, False))                        # three blocks: the ticket
    want = run.outputs()
    run.launch(want)
    outs = [run.outputs() for _ in range(4)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        with torch.cuda.stream(two_streams[k % 2]):
            run.launch(o)
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert run.intact(o)
        same_bits({n: b.host() for n, b in o.items()}, {n: b.host() for n, b in want.items()}, f"launch {k} on stream {k % 2}")
