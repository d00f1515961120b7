"""CPU: gradient clipping by global norm (ABI 226; csrc/grad_norm.hip) -- the float64 restatement of tests/gradclip_ref.py against
torch.nn.utils.clip_grad_norm_, the float32 emulation of the kernel's summation order against the derived bound, the two new exports
and their ctypes signatures against the header's prototypes, the refusals that precede the first device call, and the host-side
switches (`max_grad_norm`, `grad_norm_type`, nn.utils) on optimizers built without a device."""
import ctypes
import re

import numpy as np
import pytest

import gradclip_ref as R
from test_abi import HEADER, lib  # noqa: F401 -- the fixture that loads (and if need be builds) the library

EINVAL, EALIGN = -1, -2
OPTIMIZERS = ["Adam", "AdamW", "SGD", "Momentum", "RMSprop", "Adagrad", "Adadelta", "Adamax", "NAdam"]


@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
@pytest.mark.parametrize("where", ["clips", "passes", "zeros"])
def test_restatement_equals_torch(norm_type, where):
    import torch
    rng = np.random.default_rng(7)
    grads = [rng.standard_normal(n) for n in (2049, 5, 128)]
    if where == "zeros":
        grads = [np.zeros_like(g) for g in grads]
    nt = R.NORM_L2 if norm_type == 2.0 else R.NORM_INF
    n0 = R.norm64(grads, nt)
    max_norm = {"clips": 0.37 * n0, "passes": 2.5 * n0, "zeros": 1.0}[where]
    ps = [torch.zeros(g.shape, dtype=torch.float64, requires_grad=True) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = torch.from_numpy(g.copy())
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=norm_type))
    norm, divisor, flag = R.words64(grads, nt, max_norm)
    assert flag == 0.0
    assert abs(norm - total) <= 1e-12 * max(total, 1e-300)
    assert (divisor > 1.0) == (where == "clips")
    for p, g in zip(ps, grads):
        np.testing.assert_allclose(g / divisor, p.grad.numpy(), rtol=1e-12, atol=0)


def test_restatement_scale_and_divisor_are_the_update_kernels_factor():
    g = [np.array([3.0, -4.0], np.float32)]
    assert R.norm64(g, R.NORM_L2, 0.5, 4.0) == 5.0 * 0.125 and R.norm64(g, R.NORM_INF, 0.5, 4.0) == 4.0 * 0.125
    assert R.divisor64(0.625, 10.0, 4.0) == 4.0 and R.divisor64(0.625, 0.25, 4.0) == pytest.approx(4.0 * (0.625 + 1e-6) / 0.25, rel=1e-15)
    assert np.isnan(R.norm64([np.array([1.0, np.nan], np.float32)], R.NORM_INF)) and np.isnan(R.divisor64(float("nan"), 1.0))
    assert R.words64([np.array([np.inf], np.float32)], R.NORM_L2, 1.0)[2] == 1.0


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_emulation_stays_inside_the_derived_bound(name):
    _, sizes, _ = R.case(name)
    blocks, chunk = R.plan(sizes)
    assert len(blocks) == sum(-(-n // chunk) for n in sizes) and R.depth(chunk) == {2048: 14, 16384: 28}[chunk]
    for gs, d_in in ((1.0, None), (0.5, 4.0)):
        grads = R.make_grads(name, 0)
        ref = R.norm64(grads, R.NORM_L2, gs, d_in)
        got = float(R.emulate_l2(grads, gs, d_in))
        err = abs(got - ref) / ref
        print(f"{name}: emulation vs float64 {err / R.EPS:.2f} x 2^-24, bound {R.l2_rel_bound(sizes) / R.EPS:.1f} x 2^-24")
        assert err <= R.l2_rel_bound(sizes)
        assert float(R.inf_norm32(grads, gs, d_in)) == R.norm64(grads, R.NORM_INF, gs, d_in)      # exact


def test_case_table_reaches_what_it_names():
    assert R.plan(R.case("blocks64")[1]) == ([(i, 0) for i in range(64)], 2048)
    blocks, chunk = R.plan(R.case("big_tail")[1])
    assert chunk == 16384 and len(blocks) == 257 and (2 ** 22 + 5) - 256 * chunk == 5
    assert R.plan(R.case("chunk_edges")[1])[0] == [(0, 0), (1, 0), (2, 0), (2, 1)]
    assert R.plan(R.case("zero_inside")[1])[0] == [(0, 0), (2, 0)]
    assert len(R.plan(R.case("misaligned")[1])[0]) == 3 and R.case("misaligned")[2] % 4 != 0


def test_version_is_226(lib):
    from neunet_hip import _lib
    assert _lib.load_hip_function("nnhipVersion")() >= 226


C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "float": ctypes.c_float,
           "const float* const*": ctypes.POINTER(ctypes.c_void_p), "float* const*": ctypes.POINTER(ctypes.c_void_p),
           "const int64_t*": ctypes.POINTER(ctypes.c_int64), "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
           "nnhipStream_t": ctypes.c_void_p}


@pytest.mark.parametrize("name", ["nnhipGradNormMultiTensor", "nnhipScaleMultiTensor"])
def test_ctypes_signature_matches_the_header(lib, name):
    from neunet_hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared in the header"
    want = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\*", "*", " ".join(arg.split()).rsplit(" ", 1)[0]).replace("*const", "* const")
        want.append(C_TYPES[ctype])
    restype, argtypes = _lib._SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == want
    assert hasattr(lib, name) and _lib.load_hip_function(name).argtypes == want
    assert re.search(r"NNHIP_NORM_L2\s*=\s*0\s*,\s*NNHIP_NORM_INF\s*=\s*1", text)


def test_refusals_that_need_no_device(lib):
    """Every check here precedes the first device call: the pointers are never dereferenced."""
    from neunet_hip import _lib
    norm, scale = _lib.load_hip_function("nnhipGradNormMultiTensor"), _lib.load_hip_function("nnhipScaleMultiTensor")
    opt = _lib.load_hip_function("nnhipCreateFusedOptimizer")()
    D = 0x1000
    g, sizes = (ctypes.c_void_p * 2)(D, D + 64), (ctypes.c_int64 * 2)(4, 4)
    gp, sp = ctypes.cast(g, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(sizes, ctypes.POINTER(ctypes.c_int64))

    def refused(rc, code, text):
        assert rc == code and text in _lib.last_error(), (rc, _lib.last_error())

    try:
        refused(norm(None, 2, gp, sp, 0, 1.0, None, 1, 1.0, D, None), EINVAL, "null optimizer handle")
        refused(norm(opt, 2, gp, sp, 0, 1.0, None, 1, 1.0, None, None), EINVAL, "null words")
        refused(norm(opt, 2, gp, sp, 0, 1.0, None, 1, 1.0, D + 2, None), EALIGN, "misaligned")
        refused(norm(opt, 2, gp, sp, 0, 1.0, D + 1, 1, 1.0, D, None), EALIGN, "misaligned")
        refused(norm(opt, 2, gp, sp, 2, 1.0, None, 1, 1.0, D, None), EINVAL, "norm_type")
        refused(norm(opt, 2, gp, sp, -1, 1.0, None, 1, 1.0, D, None), EINVAL, "norm_type")
        for bad in (0.0, -1.0, float("nan")):
            refused(norm(opt, 2, gp, sp, 0, bad, None, 1, 1.0, D, None), EINVAL, "max_norm")
        refused(norm(opt, 2, gp, sp, 0, 1.0, None, -1, 1.0, D, None), EINVAL, "step")
        refused(norm(opt, 2, gp, sp, 0, 1.0, None, 0, 1.0, D, None), EINVAL, "SetStep")      # step == 0 on an unprepared handle
        refused(norm(opt, -1, gp, sp, 0, 1.0, None, 1, 1.0, D, None), EINVAL, "n_tensors")
        refused(norm(opt, 2, None, sp, 0, 1.0, None, 1, 1.0, D, None), EINVAL, "null table")
        sizes[1] = -4
        refused(norm(opt, 2, gp, sp, 0, 1.0, None, 1, 1.0, D, None), EINVAL, "negative size")
        refused(scale(opt, 2, gp, sp, D, None), EINVAL, "negative size")
        sizes[1], g[1] = 4, None
        refused(norm(opt, 2, gp, sp, 0, 1.0, None, 1, 1.0, D, None), EINVAL, "null tensor pointer")
        refused(scale(opt, 2, gp, sp, D, None), EINVAL, "null tensor pointer")
        g[1] = D + 66
        refused(norm(opt, 2, gp, sp, 0, 1.0, None, 1, 1.0, D, None), EALIGN, "misaligned tensor")
        refused(scale(opt, 2, gp, sp, D, None), EALIGN, "misaligned tensor")
        g[1] = D + 64
        refused(scale(None, 2, gp, sp, D, None), EINVAL, "null optimizer handle")
        refused(scale(opt, 2, gp, sp, None, None), EINVAL, "null divisor")
        refused(scale(opt, 2, gp, sp, D + 3, None), EALIGN, "misaligned divisor")
        sizes[0] = sizes[1] = 0
        assert scale(opt, 2, gp, sp, D, None) == 0 and scale(opt, 0, None, None, D, None) == 0      # nothing to do: no launch
    finally:
        _lib.load_hip_function("nnhipDestroyFusedOptimizer")(opt)


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_switches_on_an_optimizer_without_parameters(lib, name):
    from neunet_hip import optim
    opt = getattr(optim, name)([])
    assert opt.max_grad_norm is None and opt.grad_norm_type == 2.0 and opt.last_grad_norm is None and opt.last_grad_nonfinite is None
    fuses = opt.can_fuse_into_backward()
    assert fuses is (name in ("Adam", "AdamW"))
    for bad in (0.0, -1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="max_norm"):
            opt.max_grad_norm = bad
    for bad in (1.0, 3, 0, -2.0, float("nan"), "fro", None):
        with pytest.raises(ValueError, match="norm_type"):
            opt.grad_norm_type = bad
    assert opt.max_grad_norm is None and opt.grad_norm_type == 2.0          # a refused assignment changes nothing
    opt.grad_norm_type = float("inf")
    opt.max_grad_norm = 1
    assert opt.max_grad_norm == 1.0 and opt.grad_norm_type == float("inf")
    assert opt.can_fuse_into_backward() is False and opt.pending_update_args([], 1) is None
    opt.max_grad_norm = None
    assert opt.can_fuse_into_backward() is fuses
    opt.step()                                                               # no parameters: nothing is launched, armed or not


def test_nn_utils_refuses_cpu_tensors():
    import neunet_hip
    from neunet_hip.nn import utils
    t = neunet_hip.Tensor(np.ones(3, np.float32), device="cpu")
    t.grad = np.ones(3, np.float32)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        utils.clip_grad_norm_([t], 1.0)
    with pytest.raises(NotImplementedError, match="no CPU path"):
        utils.get_grad_norm([t])
    with pytest.raises(ValueError, match="norm_type"):
        utils.clip_grad_norm_([], 1.0, norm_type=1.0)
    with pytest.raises(ValueError, match="max_norm"):
        utils.clip_grad_norm_([], 0.0)
