"""The arithmetic core of the Tensor tape (neunet/autograd.py:96-531, 588-640, 810-893) on the device.

Three layers, top to bottom:
  * tape nodes: binary / unary / reduce / transpose / matmul build the output Tensor and its grad_fn (the reference's op names, its
    `args` convention -- None when no operand needs a gradient -- and its gradient formulas);
  * canonicalisation: pure functions of shapes -- broadcast shapes -> collapsed (extent, stride) groups, axis / keepdims -> collapsed
    kept / reduced groups -- and the tier choice (`route_binary`, `route_reduce`, `route_copy`).  They restate what
    csrc/tensor_ops.hip decides on its own from the raw shapes it is handed, so they can be tested without a GPU
    (tests/test_tape_ops.py) and the GPU tests can aim a case at a tier;
  * the C entries nnhipBroadcastBinary*, nnhipReduceAxes*, nnhipStridedCopy (csrc/tensor_ops.hip) and nnhipGemmF32 for matmul.

Device float32 only; a CPU tensor raises NotImplementedError (no CPU fallback).  Comparisons and logical ops, where, flip,
__getitem__ / __setitem__ and the integer / bool tensors they need live in tensor_index.py (csrc/tensor_index.hip).
"""
from __future__ import annotations

import ctypes
import numbers

import numpy as np

from . import _lib

MAX_RANK = 8        # NNHIP_TENSOR_MAX_RANK
MAX_GROUPS = 6      # axis groups after collapsing (csrc/tensor_ops.hip: TO_MAXG)
BIN_KINDS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "power": 4, "maximum": 5, "minimum": 6}        # NNHIP_BIN_*
RED_KINDS = {"sum": 0, "mean": 1, "var": 2, "max": 3, "min": 4}                                      # NNHIP_RED_*
ACT_EXP, ACT_SQRT, ACT_SIN, ACT_COS, ACT_ABS = 8, 9, 10, 11, 12                                      # NNHIP_ACT_*
# tier boundaries of the reduction kernels (csrc/tensor_ops.hip: RED_*)
RED_WAVE_MAX_R, RED_FILL_BLOCKS, RED_ROW_SPLIT_MIN_R, RED_ROW_SEG, RED_COL_SPLIT_MIN_R, RED_COL_SEG, RED_MAX_S = 1024, 512, 8192, 4096, 256, 64, 256
RED_GEN_SPLIT_MIN_R, RED_GEN_SEG = 4096, 2048


# ---- canonicalisation: pure functions of shapes ------------------------------------------------------------------------------------
def contiguous_strides(shape):
    out, acc = [], 1
    for e in reversed(tuple(shape)):
        out.append(acc)
        acc *= e
    return tuple(reversed(out))


def broadcast_shape(sa, sb):
    """NumPy's rule; ValueError when the shapes do not broadcast."""
    sa, sb = tuple(sa), tuple(sb)
    n = max(len(sa), len(sb))
    pa, pb = (1,) * (n - len(sa)) + sa, (1,) * (n - len(sb)) + sb
    out = []
    for x, y in zip(pa, pb):
        if x != y and x != 1 and y != 1:
            raise ValueError(f"operands could not be broadcast together with shapes {sa} {sb}")
        out.append(y if x == 1 else x)
    return tuple(out)


def broadcast_strides(shape, out_shape):
    """Element strides of a CONTIGUOUS operand of `shape` viewed as `out_shape`: 0 along the axes it is broadcast over."""
    shape, out_shape = tuple(shape), tuple(out_shape)
    pad = len(out_shape) - len(shape)
    cs = (0,) * pad + contiguous_strides(shape)
    ps = (1,) * pad + shape
    return tuple(0 if (p == 1 and o != 1) else s for p, o, s in zip(ps, out_shape, cs))


def collapse(shape, strides_list, flags=None):
    """Drop axes of extent 1, merge adjacent axes that every operand walks contiguously (and that share a flag).
    -> (extents, [strides per operand], flags), each a list over the groups; one group of extent 1 for a one-element shape.
    ValueError past MAX_GROUPS.  (csrc/tensor_ops.hip: collapse)"""
    ext, st, fl = [], [[] for _ in strides_list], []
    for i, e in enumerate(shape):
        if e == 1:
            continue
        f = bool(flags[i]) if flags is not None else False
        merge = bool(ext) and fl[-1] == f and all(s[-1] == src[i] * e for s, src in zip(st, strides_list))
        if merge:
            ext[-1] *= e
            for s, src in zip(st, strides_list):
                s[-1] = src[i]
        else:
            ext.append(e)
            fl.append(f)
            for s, src in zip(st, strides_list):
                s.append(src[i])
    if len(ext) > MAX_GROUPS:
        raise ValueError(f"more than {MAX_GROUPS} axis groups remain after collapsing shape {tuple(shape)}")
    if not ext:
        ext, fl = [1], [False]
        st = [[0] for _ in strides_list]
    return ext, st, fl


def check_rank(shape):
    if len(shape) > MAX_RANK:
        raise ValueError(f"rank {len(shape)} is over the limit of {MAX_RANK}")


def canonical_broadcast(sa, sb):
    """Shapes of two contiguous operands -> (out_shape, extents, strides_a, strides_b) over the collapsed groups."""
    out_shape = broadcast_shape(sa, sb)
    check_rank(out_shape)
    ext, (ta, tb), _ = collapse(out_shape, [broadcast_strides(sa, out_shape), broadcast_strides(sb, out_shape)])
    return out_shape, ext, ta, tb


def normalize_axes(ndim, axis):
    if axis is None:
        return tuple(range(ndim))
    axes = (axis,) if isinstance(axis, numbers.Integral) else tuple(axis)
    out = []
    for a in axes:
        a = int(a)
        if not -ndim <= a < ndim:
            raise ValueError(f"axis {a} is out of bounds for a tensor of rank {ndim}")
        a %= ndim
        if a in out:
            raise ValueError("duplicate value in 'axis'")
        out.append(a)
    return tuple(out)


def canonical_reduce(shape, axis, keepdims=False):
    """-> dict: flags (per raw axis), out_shape (as NumPy gives it), kept_shape (keepdims form), n (reduced count),
    extents / strides / red (collapsed groups of a contiguous input)."""
    shape = tuple(shape)
    check_rank(shape)
    axes = normalize_axes(len(shape), axis)
    flags = [i in axes for i in range(len(shape))]
    kept_shape = tuple(1 if f else e for e, f in zip(shape, flags))
    out_shape = kept_shape if keepdims else tuple(e for e, f in zip(shape, flags) if not f)
    n = int(np.prod([e for e, f in zip(shape, flags) if f], dtype=np.int64)) if axes else 1
    ext, (st,), red = collapse(shape, [contiguous_strides(shape)], flags)
    return {"flags": flags, "out_shape": out_shape, "kept_shape": kept_shape, "n": n, "extents": ext, "strides": st, "red": red}


def _full(ext, st):
    want = 1
    for e, s in zip(reversed(ext), reversed(st)):
        if s != want:
            return False
        want *= e
    return True


def route_ew(ext, strides_list, aligned=True):
    """The elementwise kernel of csrc/tensor_ops.hip for operands that are neither all-full nor scalar: 'vec2d' or 'general'."""
    vec = aligned and len(ext) <= 2 and ext[-1] % 4 == 0
    for st in strides_list:
        vec = vec and st[-1] in (0, 1) and (st[-1] == 0 or len(ext) == 1 or st[0] % 4 == 0)
    return "vec2d" if vec else "general"


def route_binary(sa, sb, aligned=True, scalar=None):
    """Tier of nnhipBroadcastBinaryForward: 'same' | 'scalar' | 'inner' | 'outer' | 'vec2d' | 'general'.  `scalar`: 'a' or 'b' when
    that operand is a Python scalar (its shape argument is ignored).  inner / outer are the two named faces of the vec2d kernel:
    the small operand spans the innermost group ([N,F] o [F]) or is constant along it ([N,F] o [N,1])."""
    if scalar is not None:
        return "scalar"
    _, ext, ta, tb = canonical_broadcast(sa, sb)
    n = int(np.prod(ext))
    fa, fb = _full(ext, ta) or n == 1, _full(ext, tb) or n == 1
    if fa and fb:
        return "same"
    if (fa and not any(tb)) or (fb and not any(ta)):
        return "scalar"
    tier = route_ew(ext, [ta, tb], aligned)
    if tier == "vec2d" and len(ext) == 2 and (fa or fb):
        small = tb if fa else ta
        if small[0] == 0 and small[1] == 1:
            return "inner"
        if small[1] == 0:
            return "outer"
    return tier


def route_reduce(ext, red):
    """Tier of the reduction kernels for collapsed groups: (name, S) with S the number of segments the reduced extent is split into.
    'row-wave' | 'row-block' | 'col' | 'general'."""
    pat = "".join("R" if r else "K" for r in red)
    if pat not in ("R", "K", "KR", "RK", "KRK"):
        nout = int(np.prod([e for e, r in zip(ext, red) if not r]))
        nred = int(np.prod([e for e, r in zip(ext, red) if r]))
        cdiv = lambda a, b: -(-a // b)
        S = 1
        if nout < RED_FILL_BLOCKS and nred >= RED_GEN_SPLIT_MIN_R:
            S = min(cdiv(nred, RED_GEN_SEG), cdiv(2 * RED_FILL_BLOCKS, nout), RED_MAX_S)
            S = cdiv(nred, cdiv(nred, S))
        return "general", S
    ko = ext[0] if pat in ("KR", "KRK") else 1
    r = ext[pat.index("R")] if "R" in pat else 1
    ki = ext[-1] if pat in ("K", "RK", "KRK") else 1
    cdiv = lambda a, b: -(-a // b)
    S = 1
    if ki == 1:
        if r <= RED_WAVE_MAX_R:
            return "row-wave", 1
        if ko < RED_FILL_BLOCKS and r >= RED_ROW_SPLIT_MIN_R:
            S = min(cdiv(r, RED_ROW_SEG), cdiv(2 * RED_FILL_BLOCKS, ko), RED_MAX_S)
            S = cdiv(r, cdiv(r, S))
        return "row-block", S
    nbx = cdiv(ki, 64)
    if ko * nbx < RED_FILL_BLOCKS and r >= RED_COL_SPLIT_MIN_R:
        S = min(cdiv(r, RED_COL_SEG), cdiv(2 * RED_FILL_BLOCKS, ko * nbx), RED_MAX_S)
        S = cdiv(r, cdiv(r, S))
    return "col", S


def route_copy(shape, strides_in, aligned=True):
    """Tier of nnhipStridedCopy: 'tile' (the 2-D transpose through LDS) | 'vec2d' | 'general'."""
    ext, (st,), _ = collapse(shape, [strides_in])
    if len(ext) in (2, 3) and st[-2] == 1 and st[-1] != 1:
        return "tile"
    return route_ew(ext, [st], aligned)


# ---- calls --------------------------------------------------------------------------------------------------------------------------
def _i64(values):
    return (ctypes.c_int64 * max(len(values), 1))(*[int(v) for v in values])


def _i32(values):
    return (ctypes.c_int32 * max(len(values), 1))(*[int(v) for v in values])


def _torch():
    import torch
    return torch


def require_device_f32(t, what):
    if t.device != "cuda":
        raise NotImplementedError(f"Tensor.{what} runs on device tensors only (no CPU fallback); move the tensor with .to('cuda')")
    if t.dtype != np.float32:
        raise NotImplementedError(f"Tensor.{what}: float32 only, got {t.dtype}")


def _contig(a):
    return a if a.is_contiguous() else a.contiguous()


def is_scalar(t):
    return isinstance(t, (numbers.Number, np.number, np.bool_)) or (isinstance(t, np.ndarray) and t.ndim == 0)


def binary_forward(kind, a, b, scalar=0.0):
    """a, b: contiguous device arrays, or None for the by-value `scalar` (one of them at most)."""
    torch = _torch()
    sa = tuple(a.shape) if a is not None else ()
    sb = tuple(b.shape) if b is not None else ()
    out_shape = broadcast_shape(sa, sb)
    check_rank(out_shape)
    out = torch.empty(out_shape, dtype=torch.float32, device="cuda")
    _lib.call_hip_function("nnhipBroadcastBinaryForward", kind, out, a, b, float(scalar), len(out_shape), _i64(out_shape),
                           _i64(broadcast_strides(sa, out_shape)), _i64(broadcast_strides(sb, out_shape)), _lib.get_current_stream_ptr())
    return out


def binary_backward(kind, grad, a, b, scalar, need_a, need_b):
    """-> (dA, dB) in the operands' own shapes (None where not needed): ONE nnhipBroadcastBinaryBackward call."""
    torch = _torch()
    sa = tuple(a.shape) if a is not None else ()
    sb = tuple(b.shape) if b is not None else ()
    out_shape = tuple(grad.shape)
    dA = torch.empty(sa, dtype=torch.float32, device="cuda") if need_a else None
    dB = torch.empty(sb, dtype=torch.float32, device="cuda") if need_b else None
    _lib.call_hip_function("nnhipBroadcastBinaryBackward", kind, dA, dB, _contig(grad), a, b, float(scalar), len(out_shape), _i64(out_shape),
                           _i64(broadcast_strides(sa, out_shape)), _i64(broadcast_strides(sb, out_shape)), _lib.get_current_stream_ptr())
    return dA, dB


def binary(x, t, op, reflected=False):
    """x.op(t) (or t.op(x) when reflected, t then being a scalar) on the tape."""
    from .autograd import Tensor
    require_device_f32(x, op)
    kind = BIN_KINDS[op]
    if isinstance(t, Tensor):
        if t.device != x.device:
            raise ValueError("Tensors must be on the same device")
        require_device_f32(t, op)
    elif is_scalar(t):
        t = float(t)
    else:   # array-likes become constants, as the reference's ensure_tensor makes them (requires_grad=False)
        t = Tensor(np.asarray(t, dtype=np.float32), requires_grad=False, device="cuda")
    A, B = (t, x) if reflected else (x, t)
    ad = _contig(A.data) if isinstance(A, Tensor) else None
    bd = _contig(B.data) if isinstance(B, Tensor) else None
    sc = A if ad is None else (B if bd is None else 0.0)
    rg = any(isinstance(o, Tensor) and o.requires_grad for o in (A, B))
    out = Tensor._wrap(binary_forward(kind, ad, bd, sc), (A, B) if rg else None, op, "cuda", requires_grad=rg)

    def grad_fn(a, b, grad):
        need_a = isinstance(a, Tensor) and a.requires_grad
        need_b = isinstance(b, Tensor) and b.requires_grad
        if not (need_a or need_b):
            return
        dA, dB = binary_backward(kind, grad, ad, bd, sc, need_a, need_b)
        if need_a:
            a.apply_grad(dA)
        if need_b:
            b.apply_grad(dB)

    out.grad_fn = grad_fn
    return out


def unary(x, kind, op):
    from .nn.experimental.activations import hip_activation
    require_device_f32(x, op)
    return hip_activation(x, kind, op)


def tanh(x):
    """neunet/autograd.py:391: nnhipTanhForward; the backward reads the OUTPUT (nnhipTanhBackward: grad (1 - f^2))."""
    from .autograd import Tensor
    require_device_f32(x, "tanh")
    torch = _torch()
    xd = _contig(x.data)
    f = torch.empty_like(xd)
    _lib.call_hip_function("nnhipTanhForward", f, xd, xd.numel(), _lib.get_current_stream_ptr())
    out = Tensor._wrap(f, (x,), "tanh", "cuda", requires_grad=x.requires_grad)

    def grad_fn(t, grad):
        if not t.requires_grad:
            return
        g = torch.empty_like(f)
        _lib.call_hip_function("nnhipTanhBackward", g, _contig(grad), f, f.numel(), _lib.get_current_stream_ptr())
        t.apply_grad(g)

    out.grad_fn = grad_fn
    return out


def neg(x):
    """neunet/autograd.py:810: -x, backward -grad: the scalar tier of mul."""
    from .autograd import Tensor
    require_device_f32(x, "neg")
    xd = _contig(x.data)
    out = Tensor._wrap(binary_forward(BIN_KINDS["mul"], xd, None, -1.0), (x,), "neg", "cuda", requires_grad=x.requires_grad)

    def grad_fn(t, grad):
        if t.requires_grad:
            t.apply_grad(binary_forward(BIN_KINDS["mul"], _contig(grad), None, -1.0))

    out.grad_fn = grad_fn
    return out


def pos(x):
    from .autograd import Tensor
    require_device_f32(x, "pos")
    out = Tensor._wrap(x.data, (x,), "pos", "cuda", requires_grad=x.requires_grad)

    def grad_fn(t, grad):
        if t.requires_grad:
            t.apply_grad(grad)

    out.grad_fn = grad_fn
    return out


def reduce(x, op, axis=None, keepdims=False):
    from .autograd import Tensor
    require_device_f32(x, op)
    torch = _torch()
    kind = RED_KINDS[op]
    xd = _contig(x.data)
    shape = tuple(xd.shape)
    c = canonical_reduce(shape, axis, keepdims)
    if c["n"] == 0 and int(np.prod(c["out_shape"], dtype=np.int64)) > 0:
        raise ValueError(f"Tensor.{op}: reduction over zero elements")
    out = torch.empty(c["out_shape"], dtype=torch.float32, device="cuda")
    # var keeps the mean its forward computed, in keepdims shape, for the backward
    mean = torch.empty(c["kept_shape"], dtype=torch.float32, device="cuda") if op == "var" and x.requires_grad else None
    flags = _i32(c["flags"])
    _lib.call_hip_function("nnhipReduceAxesForward", kind, out, mean, xd, len(shape), _i64(shape), _i64(contiguous_strides(shape)), flags,
                           _lib.get_current_stream_ptr())
    res = Tensor._wrap(out, (x, axis), op, "cuda", requires_grad=x.requires_grad)
    saved = mean if op == "var" else (out if op in ("max", "min") else None)

    def grad_fn(t, axis_, grad):
        if not t.requires_grad:
            return
        dX = torch.empty(shape, dtype=torch.float32, device="cuda")
        need_x = op in ("var", "max", "min")
        _lib.call_hip_function("nnhipReduceAxesBackward", kind, dX, _contig(grad), xd if need_x else None, saved if need_x else None,
                               len(shape), _i64(shape), flags, _lib.get_current_stream_ptr())
        t.apply_grad(dX)

    res.grad_fn = grad_fn
    return res


def strided_copy(src, shape, strides, scale=1.0):
    torch = _torch()
    check_rank(shape)
    out = torch.empty(tuple(shape), dtype=torch.float32, device="cuda")
    _lib.call_hip_function("nnhipStridedCopy", out, _lib.StridedView(src) if not src.is_contiguous() else src, float(scale), len(shape),
                           _i64(shape), _i64(strides), _lib.get_current_stream_ptr())
    return out


def permute(xd, axes):
    """A contiguous copy of the contiguous device array `xd` with its axes permuted."""
    shape, st = tuple(xd.shape), contiguous_strides(xd.shape)
    return strided_copy(xd, [shape[a] for a in axes], [st[a] for a in axes])


def transpose(x, axes, op="transpose", extra=None):
    from .autograd import Tensor
    require_device_f32(x, op)
    nd = x.ndim
    axes = tuple(range(nd))[::-1] if not axes else tuple(int(a) % nd if -nd <= int(a) < nd else int(a) for a in axes)
    if sorted(axes) != list(range(nd)):
        raise ValueError(f"axes {axes} do not match a tensor of rank {nd}")
    out = Tensor._wrap(permute(_contig(x.data), axes), (x,) + (tuple(extra) if extra is not None else (axes,)), op, "cuda",
                       requires_grad=x.requires_grad)
    inverse = tuple(int(i) for i in np.argsort(axes))

    def grad_fn(t, *rest, grad):
        if t.requires_grad:
            t.apply_grad(permute(_contig(grad), inverse))

    out.grad_fn = grad_fn
    return out


def swapaxes(x, axis1, axis2):
    nd = x.ndim
    axes = list(range(nd))
    a1, a2 = int(axis1) % nd, int(axis2) % nd
    axes[a1], axes[a2] = axes[a2], axes[a1]
    return transpose(x, axes, "swapaxes", (axis1, axis2))


def _gemm(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, batch=1, sA=0, sB=0, sC=0):
    if M * N * batch == 0:
        return
    if K == 0:
        C.zero_()
        return
    _lib.call_hip_function("nnhipGemmF32", A, B, C, None, M, N, K, lda, ldb, ldc, int(a_kmajor), int(b_kmajor), batch, sA, sB, sC,
                           _lib.get_current_stream_ptr())


def matmul(x, t):
    """neunet/autograd.py:192-230 on nnhipGemmF32: matrix x matrix with equal leading batch dimensions or a shared 2-D right operand,
    and the 1-D vector cases (against a 2-D matrix).  Transposed operands of the backward are layout flags, not copies; the gradient
    of a shared right operand is one GEMM over the flattened (batch * M) dimension."""
    from .autograd import Tensor
    torch = _torch()
    require_device_f32(x, "matmul")
    if not isinstance(t, Tensor):
        t = Tensor(np.asarray(t, dtype=np.float32), requires_grad=False, device="cuda")
    if t.device != x.device:
        raise ValueError("Tensors must be on the same device")
    require_device_f32(t, "matmul")
    a, b = _contig(x.data), _contig(t.data)
    if a.ndim == 0 or b.ndim == 0:
        raise ValueError("matmul: operands must have at least one dimension")
    va, vb = a.ndim == 1, b.ndim == 1
    if (va or vb) and max(a.ndim, b.ndim) > 2:
        raise NotImplementedError("matmul: a vector operand is supported against a 2-D matrix (or a vector) only")
    a2 = a.reshape(1, -1) if va else a
    b2 = b.reshape(-1, 1) if vb else b
    M, K, N = a2.shape[-2], a2.shape[-1], b2.shape[-1]
    if b2.shape[-2] != K:
        raise ValueError(f"matmul: shapes {tuple(a.shape)} and {tuple(b.shape)} are not aligned")
    shared = b2.ndim == 2
    if not shared and tuple(a2.shape[:-2]) != tuple(b2.shape[:-2]):
        raise NotImplementedError(f"matmul: batch dimensions {tuple(a2.shape[:-2])} and {tuple(b2.shape[:-2])} differ; only equal batch "
                                  f"dimensions or a shared 2-D right operand are supported")
    batch = int(np.prod(a2.shape[:-2], dtype=np.int64))
    c2 = torch.empty(tuple(a2.shape[:-1]) + (N,), dtype=torch.float32, device="cuda")
    if shared:
        _gemm(a2, b2, c2, batch * M, N, K, K, N, N, 1, 0)
    else:
        _gemm(a2, b2, c2, M, N, K, K, N, N, 1, 0, batch, M * K, K * N, M * N)
    out_shape = tuple(c2.shape[:-2]) + (() if va else (M,)) + (() if vb else (N,))
    rg = x.requires_grad or t.requires_grad
    out = Tensor._wrap(c2.reshape(out_shape), (x, t) if rg else None, "matmul", "cuda", requires_grad=rg)

    def grad_fn(p, q, grad):
        g2 = _contig(grad).reshape(c2.shape)
        if p.requires_grad:        # dA = g B^T
            dA = torch.empty_like(a2)
            if shared:
                _gemm(g2, b2, dA, batch * M, K, N, N, N, K, 1, 1)
            else:
                _gemm(g2, b2, dA, M, K, N, N, N, K, 1, 1, batch, M * N, K * N, M * K)
            p.apply_grad(dA.reshape(a.shape))
        if q.requires_grad:        # dB = A^T g
            dB = torch.empty_like(b2)
            if shared:
                _gemm(a2, g2, dB, K, N, batch * M, K, N, N, 0, 0)
            else:
                _gemm(a2, g2, dB, K, N, M, K, N, N, 0, 0, batch, M * K, M * N, K * N)
            q.apply_grad(dB.reshape(b.shape))

    out.grad_fn = grad_fn
    return out
