"""CPU-only: the C ABI of the weight-streaming Linear forward (nnhipLinearGemvForward, nnhipSetLinearGemv / nnhipGetLinearGemv; ABI
214) -- every argument check happens before any device call -- the host package's switch, the example's --linear option, and the
float32 emulation of the kernel's summation order that the GPU tests' error bound (c = 4 in assert_dot_close) rests on."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_abi import lib  # noqa: F401  (fixture: builds the library if it is missing, then loads it)

EINVAL, EALIGN = -1, -2
DUMMY = 0x1000                      # a non-null, 16-byte aligned pointer value nothing dereferences: every check precedes the device


def gemv(*args):
    from neunet_hip import _lib
    return _lib.load_hip_function("nnhipLinearGemvForward")(*args)


def test_abi_214_symbols_bind(lib):  # noqa: F811
    from neunet_hip import _lib
    assert _lib.load_hip_function("nnhipVersion")() >= 214
    for name in ("nnhipLinearGemvForward", "nnhipSetLinearGemv", "nnhipGetLinearGemv"):
        assert hasattr(lib, name), name
        _lib.load_hip_function(name)
    assert "nnhipGetLinearGemv" in _lib._NO_STATUS and "nnhipSetLinearGemv" not in _lib._NO_STATUS
    assert _lib.load_hip_function("nnhipGemmLaunchCount")(4) >= 0           # the kernel's family exists
    assert _lib.load_hip_function("nnhipGemmLaunchCount")(5) == -1


def test_status_codes_need_no_device(lib):  # noqa: F811
    from neunet_hip import _lib
    D = DUMMY
    launched = _lib.load_hip_function("nnhipGemmLaunchCount")(4)
    assert gemv(D, D, D, D, D, 9, 16, 16, None) == EINVAL                   # rows > NNHIP_LINEAR_GEMV_MAX_ROWS
    assert "nnhipLinearGemvForward" in _lib.last_error()
    for rows, n_in, n_out in ((-1, 16, 16), (1, -16, 16), (1, 16, -16)):
        assert gemv(D, D, D, D, D, rows, n_in, n_out, None) == EINVAL
        assert "nnhipLinearGemvForward" in _lib.last_error() and "negative" in _lib.last_error()
    for null in range(3):                                                   # X, W, O
        p = [D, D, None, None, D]
        p[(0, 1, 4)[null]] = None
        assert gemv(*p, 1, 16, 16, None) == EINVAL
        assert "nnhipLinearGemvForward" in _lib.last_error() and "null" in _lib.last_error()
    for odd in range(5):                                                    # X, W, b, addend, O: 4-byte alignment each
        p = [D, D, D, D, D]
        p[odd] = D + 2
        assert gemv(*p, 1, 16, 16, None) == EALIGN
        assert "nnhipLinearGemvForward" in _lib.last_error() and "misaligned" in _lib.last_error()
    # nothing to do: 0 and no launch, whatever the pointers are
    assert gemv(None, None, None, None, None, 0, 16, 16, None) == 0
    assert gemv(D, D, None, None, D, 1, 16, 0, None) == 0
    assert _lib.load_hip_function("nnhipGemmLaunchCount")(4) == launched


def test_switch_defaults_off_and_rejects_other_values(lib):  # noqa: F811
    from neunet_hip import _lib
    get, set_ = _lib.load_hip_function("nnhipGetLinearGemv"), _lib.load_hip_function("nnhipSetLinearGemv")
    assert get() == 0
    assert set_(2) == EINVAL and get() == 0
    assert "nnhipSetLinearGemv" in _lib.last_error()
    assert set_(-1) == EINVAL and get() == 0
    try:
        assert set_(1) == 0 and get() == 1
        assert set_(2) == EINVAL and get() == 1                             # a refused value leaves the switch where it was
    finally:
        assert set_(0) == 0
    assert get() == 0


def test_context_manager_restores_the_previous_value(lib):  # noqa: F811
    import neunet_hip
    assert neunet_hip.get_linear_gemv() is False
    with neunet_hip.linear_gemv():
        assert neunet_hip.get_linear_gemv() is True
        with neunet_hip.linear_gemv(False):
            assert neunet_hip.get_linear_gemv() is False
        assert neunet_hip.get_linear_gemv() is True
    assert neunet_hip.get_linear_gemv() is False
    with pytest.raises(RuntimeError, match="boom"):
        with neunet_hip.linear_gemv(True):
            assert neunet_hip.get_linear_gemv() is True
            raise RuntimeError("boom")
    assert neunet_hip.get_linear_gemv() is False
    neunet_hip.set_linear_gemv(True)
    try:
        with pytest.raises(RuntimeError, match="boom"):
            with neunet_hip.linear_gemv(False):
                raise RuntimeError("boom")
        assert neunet_hip.get_linear_gemv() is True                         # "previous", not "off"
    finally:
        neunet_hip.set_linear_gemv(False)


def test_example_linear_option(lib):  # noqa: F811
    import inspect
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import gpt2_infer as G
    assert inspect.signature(G.generate).parameters["linear"].default == "gemm"
    with pytest.raises(ValueError, match="bogus"):
        G.generate(None, np.zeros((1, 4), np.int32), 2, mode="cached", linear="bogus")
    ap = G.build_parser()
    assert ap.parse_args(["--random"]).linear == "gemm"
    assert ap.parse_args(["--random", "--linear", "gemv"]).linear == "gemv"
    with pytest.raises(SystemExit):
        ap.parse_args(["--random", "--linear", "bogus"])


# ------------------------------------------------------------------------------------------- the error bound
# The kernel's order of additions for one output (csrc/linear_gemv.hip), restated in float32 NumPy WITHOUT fused multiply-adds (each
# product rounded, then each add: the kernel's fmaf chain rounds once where this rounds twice, so this is the pessimistic twin):
# lane t of 256 folds the float4 groups t, t + 256, ... sequentially; then the 256 chain ends are merged.  Two merges are checked: the
# one the kernel uses (lane q of eight adds the ends q, q + 8, ... in order, then a three-level tree over the eight) and a pairwise
# tree per 64 lanes with the four partials added in order.  Either stays within 1 unit of 2^-24 sum|x||w| of float64 -- measured:
# at most 0.90 units, at (3, 7) where a term is the whole sum -- which is why the GPU tests ask for c = 4 where the tiled GEMM's
# k-ordered chain needs c = 32.  A dropped or doubled k element costs a whole term: orders of magnitude more than 4 units.
F32 = np.float32


def lane_chain_ends(x, W):
    K, N = x.shape[0], W.shape[0]
    J = (((K + 3) // 4) + 255) // 256
    prod = np.zeros((N, J * 1024), F32)
    prod[:, :K] = (W * x[None, :]).astype(F32)
    prod = prod.reshape(N, J, 256, 4)
    acc = np.zeros((N, 256), F32)
    for j in range(J):
        for e in range(4):
            acc = (acc + prod[:, j, :, e]).astype(F32)
    return acc


def merge_kernel(acc):
    a = acc.reshape(-1, 32, 8)                                              # chain end 8 j + q
    s = a[:, 0, :].copy()
    for j in range(1, 32):
        s = (s + a[:, j, :]).astype(F32)
    s = (s[:, 0::2] + s[:, 1::2]).astype(F32)
    s = (s[:, 0::2] + s[:, 1::2]).astype(F32)
    return (s[:, 0] + s[:, 1]).astype(F32)


def merge_tree64(acc):
    a, n = acc.reshape(-1, 4, 64), 64
    while n > 1:
        a = (a[:, :, 0:n:2] + a[:, :, 1:n:2]).astype(F32)
        n //= 2
    a = a[:, :, 0]
    return (((a[:, 0] + a[:, 1]).astype(F32) + a[:, 2]).astype(F32) + a[:, 3]).astype(F32)


@pytest.mark.parametrize("dist", ["uniform", "normal"])
@pytest.mark.parametrize("n_in,n_out", [(768, 3000), (3072, 3000), (3, 7)])
def test_lane_striped_sum_stays_within_one_unit(n_in, n_out, dist):
    rng = np.random.default_rng(n_in + n_out)
    draw = (lambda *s: rng.uniform(-1, 1, s)) if dist == "uniform" else (lambda *s: rng.standard_normal(s))
    x, W = draw(n_in).astype(F32), draw(n_out, n_in).astype(F32)
    ref = W.astype(np.float64) @ x.astype(np.float64)
    unit = 2.0 ** -24 * (np.abs(W).astype(np.float64) @ np.abs(x).astype(np.float64))
    ends = lane_chain_ends(x, W)
    for name, merge in (("kernel", merge_kernel), ("tree64", merge_tree64)):
        worst = float(np.max(np.abs(merge(ends).astype(np.float64) - ref) / unit))
        assert worst <= 1.0, f"{name} merge: {worst:.2f} units at in = {n_in}, {dist}"
    # the bound notices one missing term
    broken = merge_kernel(lane_chain_ends(np.concatenate([x[:-1], [F32(0)]]).astype(F32), W))
    assert float(np.max(np.abs(broken.astype(np.float64) - ref) / unit)) > 4.0 * 100
