"""The rest of the Tensor tape (neunet/autograd.py:642-808, 895-923) on the device: comparisons and logical ops, where, flip,
__getitem__ / __setitem__ (basic keys, integer arrays on adjacent axes, boolean-mask assignment), on float32, int32, int64 and bool.

Layers, as in tensor_ops.py:
  * tape nodes: compare / logical / where / getitem / setitem / flip build the output Tensor and its grad_fn with the reference's op
    names and `args` convention.  A CPU tensor runs the same op in NumPy, gradients included (masks and ids being prepared on the host);
  * canonicalisation, pure functions of shapes that tests can check against NumPy without a GPU: `canonical_index` (ints, slices of any
    step, None, Ellipsis -> offset, shape, signed strides), `canonical_lattice` (the same key as start / step / count per axis, for the
    backward) and `canonical_advanced` (integer arrays on adjacent axes -> [outer, D1..Dk, inner] and the broadcast index arrays);
  * the C entries of csrc/tensor_index.hip (ABI 224).

An index array that lives on the HOST (a list, an ndarray, a CPU Tensor) is range-checked here (IndexError).  A DEVICE index Tensor is
not: the check would be a host read in the middle of a step (see neunet_hip.argmax).  An element of it outside its axis reads as 0 in
__getitem__ and is skipped by the backward and by __setitem__ -- nnhipEmbeddingForward's rule.
Repeated indices: the reference ASSIGNS in its backward (`_grad[index] = grad`), so the last occurrence in C order wins, as in NumPy.
Boolean-mask __getitem__ has a data-dependent shape and is not provided: use where (or a mask __setitem__).
"""
from __future__ import annotations

import ctypes
import numbers
import operator

import numpy as np

from . import _lib
from .tensor_ops import (_contig, _i64, broadcast_shape, broadcast_strides, check_rank, collapse, contiguous_strides, normalize_axes)

DT_F32, DT_I32, DT_I64, DT_U8 = 0, 1, 2, 3                                             # NNHIP_DT_*
_NP_DT = {np.dtype(np.float32): DT_F32, np.dtype(np.int32): DT_I32, np.dtype(np.int64): DT_I64, np.dtype(np.bool_): DT_U8,
          np.dtype(np.uint8): DT_U8}
CMP_KINDS = {"equal": 0, "not_equal": 1, "greater": 2, "greater_equal": 3, "less": 4, "less_equal": 5}      # NNHIP_CMP_*
LOGICAL_KINDS = {"logical_and": 0, "logical_or": 1, "logical_not": 2}                                      # NNHIP_LOGICAL_*
MAX_INDEX_ARRAYS = 4                                                                                        # NNHIP_INDEX_MAX_ARRAYS
# NNHIP_TIER_* of csrc/tensor_index.hip
TIER_VEC4, TIER_GENERAL, TIER_SLICE_BWD_VEC, TIER_SLICE_BWD_SCALAR, TIER_ROW_VEC, TIER_ROW, TIER_ELEMENT = 20, 21, 22, 23, 24, 25, 26
GATHER_ROW_MIN_INNER = 16


def _torch():
    import torch
    return torch


def _T():
    from .autograd import Tensor
    return Tensor


def _stream():
    return _lib.get_current_stream_ptr()


def _dt(np_dtype, what):
    try:
        return _NP_DT[np.dtype(np_dtype)]
    except KeyError:
        raise NotImplementedError(f"Tensor.{what}: float32, int32, int64 and bool tensors only, got {np.dtype(np_dtype)}") from None


def _is_py_scalar(t):
    return isinstance(t, (bool, numbers.Number)) and not isinstance(t, np.generic)


def _scalar_args(v):
    """A Python scalar -> (double, int64, is_int) as the C entries take it."""
    if isinstance(v, (bool, numbers.Integral)):
        v = int(v)
        if not -(1 << 63) <= v < (1 << 63):
            raise NotImplementedError("an integer scalar outside int64")
        return float(v), v, 1
    if isinstance(v, numbers.Real):
        return float(v), 0, 0
    raise NotImplementedError(f"a scalar of type {type(v).__name__}")


# ---- canonicalisation of keys: pure functions ---------------------------------------------------------------------------------------------
def _is_index_array(k):
    return isinstance(k, (list, np.ndarray)) or isinstance(k, _T())


def _expand_key(ndim, key):
    """tuple key with its Ellipsis replaced by full slices; IndexError as NumPy raises it."""
    key = key if isinstance(key, tuple) else (key,)
    n_ell = sum(1 for k in key if k is Ellipsis)
    if n_ell > 1:
        raise IndexError("an index can only have a single ellipsis ('...')")
    used = sum(1 for k in key if k is not None and k is not Ellipsis)
    if used > ndim:
        raise IndexError(f"too many indices for array: array is {ndim}-dimensional, but {used} were indexed")
    if n_ell == 0:
        key = key + (Ellipsis,)
    out = []
    for k in key:
        if k is Ellipsis:
            out.extend([slice(None)] * (ndim - used))
        else:
            out.append(k)
    return out


def _parse_basic(shape, key):
    """-> entries in key order: ("new",) | ("int", axis, index) | ("slice", axis, start, step, count)."""
    shape = tuple(int(e) for e in shape)
    entries, axis = [], 0
    for k in _expand_key(len(shape), key):
        if k is None:
            entries.append(("new",))
            continue
        ext = shape[axis]
        if isinstance(k, slice):
            start, stop, step = k.indices(ext)
            count = len(range(start, stop, step))
            entries.append(("slice", axis, start if count else 0, step, count))
        elif isinstance(k, (bool, np.bool_)):
            raise NotImplementedError("a boolean scalar as an index")
        else:
            try:
                i = operator.index(k)
            except TypeError:
                raise IndexError("only integers, slices (`:`), ellipsis (`...`), None and integer arrays are valid indices") from None
            if not -ext <= i < ext:
                raise IndexError(f"index {i} is out of bounds for axis {axis} with size {ext}")
            entries.append(("int", axis, i % ext))
        axis += 1
    return entries


def canonical_index(shape, key):
    """A basic key (ints, slices of any step, None, Ellipsis and their tuples) on a contiguous array of `shape`
    -> (offset, out_shape, strides) in elements: out[c] = flat[offset + sum(c_i * strides_i)].  Strides are signed and never 0
    (a None axis has extent 1 and stride 1).  IndexError exactly where NumPy raises it."""
    cs = contiguous_strides(shape)
    offset, out_shape, strides = 0, [], []
    for e in _parse_basic(shape, key):
        if e[0] == "new":
            out_shape.append(1)
            strides.append(1)
        elif e[0] == "int":
            offset += e[2] * cs[e[1]]
        else:
            _, axis, start, step, count = e
            offset += start * cs[axis]
            out_shape.append(count)
            strides.append(step * cs[axis])
    return offset, tuple(out_shape), tuple(strides)


def canonical_lattice(shape, key):
    """The same key as (start, step, count) per axis of `shape` (an int takes count 1): what nnhipSliceBackward walks."""
    start, step, count = [0] * len(shape), [1] * len(shape), [0] * len(shape)
    for e in _parse_basic(shape, key):
        if e[0] == "int":
            start[e[1]], count[e[1]] = e[2], 1
        elif e[0] == "slice":
            _, axis, s, st, c = e
            start[axis], step[axis], count[axis] = s, st, c
    return start, step, count


def classify_key(key):
    """'basic' | 'advanced' (integer arrays) | 'mask' (one boolean array as the whole key)."""
    Tensor = _T()
    items = key if isinstance(key, tuple) else (key,)

    def is_bool(k):
        if isinstance(k, Tensor):
            return k.dtype == np.bool_
        if isinstance(k, np.ndarray):
            return k.dtype == np.bool_
        if isinstance(k, list):
            return np.asarray(k).dtype == np.bool_
        return False

    if any(is_bool(k) for k in items):
        if len(items) != 1:
            raise NotImplementedError("a boolean mask combined with other indices")
        return "mask"
    return "advanced" if any(_is_index_array(k) for k in items) else "basic"


def canonical_advanced(shape, key):
    """Integer index arrays (and ints next to them) on ADJACENT axes, full slices before and after
    -> dict(axis, k, outer, dims, inner, arrays, bshape, out_shape, full).  `arrays`: the k index operands as given (host arrays as int64
    ndarrays, range-checked; device Tensors untouched); `bshape`: what they broadcast to; `full`: False when a slice around them is not
    `:` (the caller then slices first).  NotImplementedError for index arrays separated by a slice, for None in such a key."""
    Tensor = _T()
    shape = tuple(int(e) for e in shape)
    items = _expand_key(len(shape), key)
    if any(k is None for k in items):
        raise NotImplementedError("None (newaxis) together with index arrays")
    is_adv = [_is_index_array(k) for k in items]
    first = is_adv.index(True)
    last = len(items) - 1 - is_adv[::-1].index(True)
    # ints next to the arrays are 0-d index arrays (NumPy); an int elsewhere would move the result axes to the front
    while first > 0 and not isinstance(items[first - 1], slice):
        first -= 1
    while last + 1 < len(items) and not isinstance(items[last + 1], slice):
        last += 1
    for i, k in enumerate(items):
        inside = first <= i <= last
        if inside and isinstance(k, slice):
            raise NotImplementedError("index arrays separated by a slice")
        if not inside and not isinstance(k, slice):
            raise NotImplementedError("an integer index separated from the index arrays by a slice")
    k = last - first + 1
    if k > MAX_INDEX_ARRAYS:
        raise NotImplementedError(f"more than {MAX_INDEX_ARRAYS} index arrays")
    arrays, shapes = [], []
    for j in range(first, last + 1):
        it, ext = items[j], shape[j]
        if isinstance(it, Tensor) and it.device == "cuda":
            if it.dtype not in (np.int32, np.int64):
                raise IndexError("arrays used as indices must be of integer (or boolean) type")
            arrays.append(it)
            shapes.append(tuple(it.shape))
            continue
        a = np.asarray(it.data if isinstance(it, Tensor) else it)
        if a.size == 0 and a.dtype == np.float64:
            a = a.astype(np.int64)              # [] is an empty integer index in NumPy
        if a.dtype.kind not in "iu":
            raise IndexError("arrays used as indices must be of integer (or boolean) type")
        a = a.astype(np.int64)
        bad = a[(a < -ext) | (a >= ext)]
        if bad.size:
            raise IndexError(f"index {int(bad.flat[0])} is out of bounds for axis {j} with size {ext}")
        arrays.append(a)
        shapes.append(a.shape)
    bshape = ()
    for s in shapes:
        try:
            bshape = broadcast_shape(bshape, s)
        except ValueError:
            raise IndexError(f"shape mismatch: indexing arrays could not be broadcast together with shapes {' '.join(map(str, shapes))}") from None
    full = all(it == slice(None) or it.indices(shape[i]) == (0, shape[i], 1) for i, it in enumerate(items) if isinstance(it, slice))
    return {"axis": first, "k": k, "outer": int(np.prod(shape[:first], dtype=np.int64)), "dims": shape[first:last + 1],
            "inner": int(np.prod(shape[last + 1:], dtype=np.int64)), "arrays": arrays, "bshape": bshape,
            "out_shape": shape[:first] + bshape + shape[last + 1:], "full": full,
            "slices": tuple(items[:first]) + (slice(None),) * k + tuple(items[last + 1:])}


def route_gather(inner):
    """Tier of nnhipIndexGather / nnhipIndexAssign by the inner extent: 'row' | 'element' | 'general'."""
    return "row" if inner >= GATHER_ROW_MIN_INNER else ("element" if inner == 1 else "general")


# ---- calls --------------------------------------------------------------------------------------------------------------------------
def slice_forward(src, offset, shape, strides):
    """A contiguous copy of src[offset + c . strides] over `shape` (src: a contiguous device array of any supported dtype)."""
    torch = _torch()
    check_rank(shape)
    collapse(shape, [strides])                        # ValueError past 6 groups, before any launch
    out = torch.empty(tuple(shape), dtype=src.dtype, device="cuda")
    from .autograd import _T2NP
    _lib.call_hip_function("nnhipSliceForward", out, src, int(offset), _dt(_T2NP[src.dtype], "getitem"), len(shape), _i64(shape), _i64(strides),
                           _stream())
    return out


def _broadcast_to(src, shape):
    """`src` (contiguous device array) materialised at `shape` (NumPy broadcasting, leading 1s of src dropped as assignment allows)."""
    s = tuple(src.shape)
    while len(s) > len(shape) and s[0] == 1:
        s = s[1:]
    if s == tuple(shape):
        return src.reshape(shape)
    if broadcast_shape(s, shape) != tuple(shape):
        raise ValueError(f"could not broadcast input array from shape {tuple(src.shape)} into shape {tuple(shape)}")
    return slice_forward(src, 0, shape, broadcast_strides(s, shape))


def _operand(x, t, what):
    """The other operand of x's binary op: ('tensor', Tensor) | ('scalar', python scalar) | None (not comparable)."""
    Tensor = _T()
    if isinstance(t, Tensor):
        if t.device != x.device:
            raise ValueError("Tensors must be on the same device")
        return "tensor", t
    if _is_py_scalar(t):
        return "scalar", t
    if isinstance(t, np.generic):
        # a NumPy scalar is no weak Python scalar (NumPy 2): it takes part in the promotion.  Where that promotion ends in the type the
        # by-value scalar is compared in anyway (int64 / double for an integer tensor, float32 for a float32 tensor), it travels by value
        xk = np.dtype(x.dtype).kind
        if (xk in "iub" and t.dtype.kind in "iubf") or (xk == "f" and np.result_type(x.dtype, t.dtype) == np.dtype(x.dtype)):
            return "scalar", t.item()
    if isinstance(t, (np.generic, np.ndarray)):
        return "tensor", Tensor(np.asarray(t), requires_grad=False, dtype=np.asarray(t).dtype, device=x.device)
    if isinstance(t, (list, tuple)):
        try:
            arr = np.asarray(t, dtype=x.dtype)
        except (TypeError, ValueError):
            return None
        return "tensor", Tensor(arr, requires_grad=False, dtype=x.dtype, device=x.device)
    return None


_NP_CMP = {"equal": np.equal, "not_equal": np.not_equal, "greater": np.greater, "greater_equal": np.greater_equal, "less": np.less,
           "less_equal": np.less_equal}
_NP_LOGICAL = {"logical_and": np.logical_and, "logical_or": np.logical_or}


def _bool_result(data, op, device):
    Tensor = _T()
    if device == "cpu":
        return Tensor(np.asarray(data, dtype=np.bool_), None, op, requires_grad=False, dtype=np.bool_, device="cpu")
    return Tensor._wrap(data, None, op, "cuda", requires_grad=False)


def compare(x, t, op):
    """x (op) t -> a bool Tensor off the tape.  NotImplemented for an operand that is neither a Tensor, a number nor an array-like."""
    other = _operand(x, t, op)
    if other is None:
        return NotImplemented
    kind, t = other
    if x.device == "cpu":
        return _bool_result(_NP_CMP[op](x.data, t.data if kind == "tensor" else t), op, "cpu")
    torch = _torch()
    dt = _dt(x.dtype, op)
    a, sa = _contig(x.data), tuple(x.shape)
    if kind == "tensor":
        if _dt(t.dtype, op) != dt:
            raise NotImplementedError(f"Tensor.{op}: operands of different dtypes ({x.dtype} and {t.dtype}); convert one of them")
        b, sb, sc = _contig(t.data), tuple(t.shape), (0.0, 0, 0)
    else:
        b, sb, sc = None, (), _scalar_args(t)
    out_shape = broadcast_shape(sa, sb)
    check_rank(out_shape)
    out = torch.empty(out_shape, dtype=torch.bool, device="cuda")
    _lib.call_hip_function("nnhipCompare", CMP_KINDS[op], out, a, b, sc[0], sc[1], sc[2], dt, len(out_shape), _i64(out_shape),
                           _i64(broadcast_strides(sa, out_shape)), _i64(broadcast_strides(sb, out_shape)), _stream())
    return _bool_result(out, op, "cuda")


def logical(x, t, op):
    Tensor = _T()
    unary = op == "logical_not"
    if not unary:
        other = _operand(x, t, op)
        if other is None:
            return NotImplemented
        kind, t = other
        if kind == "scalar":
            t = Tensor(np.asarray(bool(t)), requires_grad=False, dtype=np.bool_, device=x.device)
    if x.device == "cpu":
        return _bool_result(np.logical_not(x.data) if unary else _NP_LOGICAL[op](x.data, t.data), op, "cpu")
    torch = _torch()
    a, sa, dta = _contig(x.data), tuple(x.shape), _dt(x.dtype, op)
    b, sb, dtb = (None, (), dta) if unary else (_contig(t.data), tuple(t.shape), _dt(t.dtype, op))
    out_shape = broadcast_shape(sa, sb)
    check_rank(out_shape)
    out = torch.empty(out_shape, dtype=torch.bool, device="cuda")
    _lib.call_hip_function("nnhipLogical", LOGICAL_KINDS[op], out, a, b, dta, dtb, len(out_shape), _i64(out_shape),
                           _i64(broadcast_strides(sa, out_shape)), _i64(broadcast_strides(sb, out_shape)), _stream())
    return _bool_result(out, op, "cuda")


def _f32_operand(t, device, what):
    """where's value operands: a float32 Tensor, or a Python scalar by value."""
    Tensor = _T()
    if isinstance(t, Tensor):
        if t.device != device:
            raise ValueError("Tensors must be on the same device")
        if t.dtype != np.float32:
            raise NotImplementedError(f"where: float32 operands only, got {t.dtype}")
        return t
    if _is_py_scalar(t) or isinstance(t, np.generic):
        return float(t)
    return Tensor(np.asarray(t, dtype=np.float32), requires_grad=False, device=device)


def where(cond, a, b):
    """np.where(cond, a, b) -> float32 on the tape; a and b: float32 Tensors or scalars (by value), cond: bool / uint8 / int32 / float32."""
    Tensor = _T()
    if not isinstance(cond, Tensor):
        dev = next((o.device for o in (a, b) if isinstance(o, Tensor)), "cpu")
        cond = Tensor(np.asarray(cond), requires_grad=False, dtype=np.asarray(cond).dtype, device=dev)
    device = cond.device
    a, b = _f32_operand(a, device, "where"), _f32_operand(b, device, "where")
    ta, tb = isinstance(a, Tensor), isinstance(b, Tensor)
    rg = (ta and a.requires_grad) or (tb and b.requires_grad)
    args = (a, cond, b) if rg else None
    sa, sb, sc = (tuple(a.shape) if ta else ()), (tuple(b.shape) if tb else ()), tuple(cond.shape)
    out_shape = broadcast_shape(broadcast_shape(sa, sb), sc)
    if device == "cpu":
        data = np.where(cond.data, a.data if ta else np.float32(a), b.data if tb else np.float32(b)).astype(np.float32)
        out = Tensor(data, args, "where", requires_grad=rg, device="cpu")

        def grad_fn_cpu(p, c, q, grad):
            zero = np.zeros_like(grad)
            if isinstance(p, Tensor) and p.requires_grad:
                p.apply_grad(np.where(c.data, grad, zero))
            if isinstance(q, Tensor) and q.requires_grad:
                q.apply_grad(np.where(c.data, zero, grad))

        out.grad_fn = grad_fn_cpu
        return out
    torch = _torch()
    cdt = _dt(cond.dtype, "where")
    if cdt == DT_I64:
        raise NotImplementedError("where: the condition is a bool, uint8, int32 or float32 tensor")
    check_rank(out_shape)
    cd = _contig(cond.data)
    ad, bd = (_contig(a.data) if ta else None), (_contig(b.data) if tb else None)
    rank, shp = len(out_shape), _i64(out_shape)
    st_c, st_a, st_b = (_i64(broadcast_strides(s, out_shape)) for s in (sc, sa, sb))
    data = torch.empty(out_shape, dtype=torch.float32, device="cuda")
    _lib.call_hip_function("nnhipWhereForward", data, cd, cdt, ad, bd, 0.0 if ta else a, 0.0 if tb else b, rank, shp, st_c, st_a, st_b, _stream())
    out = Tensor._wrap(data, args, "where", "cuda", requires_grad=rg)

    def grad_fn(p, c, q, grad):
        need_a = isinstance(p, Tensor) and p.requires_grad
        need_b = isinstance(q, Tensor) and q.requires_grad
        if not (need_a or need_b):
            return
        dA = torch.empty(sa, dtype=torch.float32, device="cuda") if need_a else None
        dB = torch.empty(sb, dtype=torch.float32, device="cuda") if need_b else None
        _lib.call_hip_function("nnhipWhereBackward", dA, dB, _contig(grad), cd, cdt, rank, shp, st_c, st_a, st_b, _stream())
        if need_a:
            p.apply_grad(dA)
        if need_b:
            q.apply_grad(dB)

    out.grad_fn = grad_fn
    return out


def _np_key(key):
    """The key with Tensors replaced by their host arrays (CPU tensors only)."""
    Tensor = _T()
    if isinstance(key, tuple):
        return tuple(_np_key(k) for k in key)
    if isinstance(key, Tensor):
        if key.device != "cpu":
            raise ValueError("a device index Tensor cannot index a CPU tensor")
        return key.data
    return key


def _index_pointers(c, what):
    """canonical_advanced's arrays on the device, broadcast to c['bshape'], one dtype -> (keepalive list, void*[k], NNHIP_DT_*, M)."""
    Tensor = _T()
    torch = _torch()
    dev = [a for a in c["arrays"] if isinstance(a, Tensor)]
    dts = {a.dtype for a in dev}
    if len(dts) > 1:
        raise NotImplementedError(f"{what}: device index tensors of different integer types")
    np_dt = np.dtype(dts.pop()) if dts else np.dtype(np.int64)
    bshape = c["bshape"]
    keep = []
    for a in c["arrays"]:
        if isinstance(a, Tensor):
            d = _contig(a.data)
            if tuple(d.shape) != bshape:
                d = slice_forward(d, 0, bshape, broadcast_strides(tuple(d.shape), bshape))
        else:
            d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, bshape)).astype(np_dt)).to("cuda")
        keep.append(d)
    ptrs = (ctypes.c_void_p * max(len(keep), 1))(*[d.data_ptr() for d in keep])
    return keep, ptrs, _NP_DT[np_dt], int(np.prod(bshape, dtype=np.int64))


def _gather(xd, c, np_dtype):
    torch = _torch()
    keep, ptrs, idt, M = _index_pointers(c, "getitem")
    out = torch.empty(c["out_shape"], dtype=xd.dtype, device="cuda")
    _lib.call_hip_function("nnhipIndexGather", out, xd, _dt(np_dtype, "getitem"), ptrs, idt, c["k"], _i64(c["dims"]), c["outer"], M, c["inner"],
                           _stream())
    return out, (keep, ptrs, idt, M)


def _index_assign(dst, src, scalar, c, idx, np_dtype, zero_fill):
    keep, ptrs, idt, M = idx
    sc = _scalar_args(scalar) if src is None else (0.0, 0, 0)
    _lib.call_hip_function("nnhipIndexAssign", dst, src, sc[0], sc[1], sc[2], _dt(np_dtype, "setitem"), int(zero_fill), ptrs, idt, c["k"],
                           _i64(c["dims"]), c["outer"], M, c["inner"], _stream())


def getitem(x, key):
    """x[key] (neunet/autograd.py:895-916): a contiguous copy; the backward assigns the gradient into zeros."""
    Tensor = _T()
    if x.device == "cpu":
        nk = _np_key(key)
        out = Tensor(x.data[nk], (x, key), "getitem", requires_grad=x.requires_grad, dtype=x.dtype, device="cpu")

        def grad_fn_cpu(t, index, grad):
            if t.requires_grad:
                g = np.zeros_like(t.data)
                g[nk] = grad
                t.apply_grad(g)

        out.grad_fn = grad_fn_cpu
        return out
    torch = _torch()
    kind = classify_key(key)
    if kind == "mask":
        raise NotImplementedError("Tensor.__getitem__ with a boolean mask has a data-dependent shape and is not provided; "
                                  "select with where(mask, x, other) or assign with x[mask] = value")
    dtype = x.dtype
    _dt(dtype, "getitem")
    rg = x.requires_grad and dtype == np.float32
    xd = _contig(x.data)
    shape = tuple(xd.shape)
    if kind == "basic":
        offset, out_shape, strides = canonical_index(shape, key)
        out = Tensor._wrap(slice_forward(xd, offset, out_shape, strides), (x, key), "getitem", "cuda", requires_grad=rg)
        start, step, count = canonical_lattice(shape, key)

        def grad_fn(t, index, grad):
            if not t.requires_grad:
                return
            dX = torch.empty(shape, dtype=torch.float32, device="cuda")
            _lib.call_hip_function("nnhipSliceBackward", dX, _contig(grad), len(shape), _i64(shape), _i64(start), _i64(step), _i64(count), _stream())
            t.apply_grad(dX)

        out.grad_fn = grad_fn
        return out
    c = canonical_advanced(shape, key)
    if not c["full"]:       # slices with bounds or steps around the arrays: slice first (a tape node of its own), then gather
        return getitem(getitem(x, c["slices"]), (slice(None),) * c["axis"] + tuple(a for a in c["arrays"]))
    data, idx = _gather(xd, c, dtype)
    out = Tensor._wrap(data, (x, key), "getitem", "cuda", requires_grad=rg)

    def grad_fn_adv(t, index, grad):
        if not t.requires_grad:
            return
        dX = torch.empty(shape, dtype=torch.float32, device="cuda")
        _index_assign(dX, _contig(grad), None, c, idx, np.float32, True)
        t.apply_grad(dX)

    out.grad_fn = grad_fn_adv
    return out


def setitem(x, key, value):
    """x[key] = value in place (neunet/autograd.py:919-923); refuses a tensor that requires a gradient, as the reference does."""
    Tensor = _T()
    if x.requires_grad:
        raise RuntimeError("Cannot assign values to a tensor with requires_grad=True")
    if x.device == "cpu":
        x.data[_np_key(key)] = value.data if isinstance(value, Tensor) else value
        return
    dtype = x.dtype
    dt = _dt(dtype, "setitem")
    if isinstance(value, Tensor):
        if value.device != "cuda":
            raise ValueError("Tensors must be on the same device")
        if _dt(value.dtype, "setitem") != dt:
            raise NotImplementedError(f"Tensor.__setitem__: a value of dtype {value.dtype} into a {dtype} tensor; convert it first")
        vd, scalar = _contig(value.data), None
    elif _is_py_scalar(value):
        vd, scalar = None, value
    else:
        vd, scalar = _torch().from_numpy(np.ascontiguousarray(np.asarray(value, dtype=dtype))).to("cuda"), None
    if not x.data.is_contiguous():
        x.data = x.data.contiguous()
    xd = x.data
    shape = tuple(xd.shape)
    kind = classify_key(key)
    if kind == "basic":
        offset, region, strides = canonical_index(shape, key)
        check_rank(region)
        st_in = None
        if vd is not None:
            vs = tuple(vd.shape)
            while len(vs) > len(region) and vs[0] == 1:
                vs = vs[1:]
            if len(vs) > len(region) or broadcast_shape(vs, region) != region:
                raise ValueError(f"could not broadcast input array from shape {tuple(vd.shape)} into shape {region}")
            st_in = broadcast_strides(vs, region)
        collapse(region, [strides] + ([st_in] if st_in is not None else []))
        sc = _scalar_args(scalar) if vd is None else (0.0, 0, 0)
        _lib.call_hip_function("nnhipStridedAssign", xd, int(offset), _i64(strides), vd, _i64(st_in) if st_in is not None else None, sc[0], sc[1],
                               sc[2], dt, len(region), _i64(region), _stream())
        return
    if kind == "mask":
        mask = key[0] if isinstance(key, tuple) else key
        if not isinstance(mask, Tensor):
            mask = Tensor(np.asarray(mask, dtype=np.bool_), requires_grad=False, dtype=np.bool_, device="cuda")
        if mask.device != "cuda":
            raise ValueError("Tensors must be on the same device")
        ms = tuple(mask.shape)
        if ms != shape[:len(ms)]:
            raise IndexError(f"boolean index did not match the indexed tensor: mask shape {ms}, tensor shape {shape}")
        rest = shape[len(ms):]
        if vd is not None:
            try:
                vd = _broadcast_to(vd, rest)
            except ValueError:
                raise NotImplementedError("Tensor.__setitem__ with a boolean mask takes a scalar or a value that broadcasts to the "
                                          f"unmasked axes {rest}; a value shaped by the number of selected elements is not provided") from None
        sc = _scalar_args(scalar) if vd is None else (0.0, 0, 0)
        _lib.call_hip_function("nnhipMaskedAssign", xd, _contig(mask.data), vd, sc[0], sc[1], sc[2], dt, int(np.prod(ms, dtype=np.int64)),
                               int(np.prod(rest, dtype=np.int64)), _stream())
        return
    c = canonical_advanced(shape, key)
    if not c["full"]:
        raise NotImplementedError("Tensor.__setitem__ with index arrays takes full slices (`:`) around them")
    idx = _index_pointers(c, "setitem")
    src = _broadcast_to(vd, c["out_shape"]) if vd is not None else None
    _index_assign(xd, src, scalar, c, idx, dtype, False)


def flip(x, axis=None):
    """np.flip (neunet/autograd.py:642-659): a strided copy with negative strides, and the same copy on the way back."""
    Tensor = _T()
    axes = normalize_axes(x.ndim, axis)
    if x.device == "cpu":
        out = Tensor(np.flip(x.data, axes), (x, axis), "flip", requires_grad=x.requires_grad, dtype=x.dtype, device="cpu")

        def grad_fn_cpu(t, axis_, grad):
            if t.requires_grad:
                t.apply_grad(np.flip(grad, axes))

        out.grad_fn = grad_fn_cpu
        return out
    _dt(x.dtype, "flip")
    xd = _contig(x.data)
    shape = tuple(xd.shape)
    cs = contiguous_strides(shape)
    strides = [-s if i in axes else s for i, s in enumerate(cs)]
    offset = sum((shape[i] - 1) * cs[i] for i in axes) if all(shape) else 0
    rg = x.requires_grad and x.dtype == np.float32
    out = Tensor._wrap(slice_forward(xd, offset, shape, strides), (x, axis), "flip", "cuda", requires_grad=rg)

    def grad_fn(t, axis_, grad):
        if t.requires_grad:
            t.apply_grad(slice_forward(_contig(grad), offset, shape, strides))

    out.grad_fn = grad_fn
    return out
