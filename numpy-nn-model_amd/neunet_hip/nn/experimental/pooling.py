"""The shape layers of neunet/nn/layers that had no counterpart here: HIPAvgPool2d (avgpool2d.py), HIPZeroPad2d (zeropad2d.py) and
HIPFlatten (flatten.py) -- the reference's constructor arguments and forward results.  AvgPool2d has kernels of its own
(csrc/avgpool.hip); ZeroPad2d is the library's slice pair run the other way round (a zero pad IS the backward of a crop:
nnhipSliceBackward writes an array on a lattice of a larger tensor and 0 elsewhere, one launch); Flatten is Tensor.reshape."""
import ctypes

import numpy as np

from ..._lib import Pool2dDesc
from ...autograd import Tensor
from ..modules import Module
from .utils import call_hip_function, contiguous, get_current_stream_ptr, require_device_f32


def _ints(v, what, lengths):
    """An int or a tuple / list of ints of one of `lengths` -> a tuple of that length (an int fills the shortest)."""
    if isinstance(v, str):
        raise ValueError(f"{what}: string values are not supported (the reference's '{v}' branch cannot run either), got {v!r}")
    if isinstance(v, (tuple, list)):
        t = tuple(v)
        if len(t) not in lengths:
            raise ValueError(f"{what} must be an int or a tuple of {' or '.join(map(str, lengths))} ints, got {v!r}")
    else:
        t = (v,) * lengths[0]
    for e in t:
        if isinstance(e, bool) or not isinstance(e, (int, np.integer)):
            raise ValueError(f"{what} must hold ints, got {v!r}")
    return tuple(int(e) for e in t)


def _padding4(padding, what):
    """int | (vertical, horizontal) | (up, down, left, right) -> (up, down, left, right), none negative."""
    p = _ints(padding, what, (2, 4))
    p = (p[0], p[0], p[1], p[1]) if len(p) == 2 else p
    if min(p) < 0:
        raise ValueError(f"{what} must not be negative, got {padding!r}")
    return p


# ----------------------------------------------------------------------------------------------- AvgPool2d
class HIPAvgPool2d(Module):
    """neunet/nn/layers/avgpool2d.py: AvgPool2d(kernel_size, stride=None, padding=0) on a (B, C, H, W) device float32 tensor.
    The zero padding counts in the mean (always divided by kh * kw), Ho = (H + up + down - kh) // sh + 1, stride None / 0 means
    kernel_size, no dilation, padding >= kernel accepted (windows wholly in the padding give 0).
    Deviations from the reference: the gradient is correct for unequal (vertical != horizontal) and 4-tuple padding, where the
    reference's grad_fn raises (it sizes its buffer from padding[0], padding[1] of the 4-tuple); the tape node is labelled
    "avgpool2d" (the reference says "maxpool2d"); a string padding raises ValueError at construction (the reference's "same" / "valid"
    branches read an attribute that does not exist)."""

    def __init__(self, kernel_size, stride=None, padding=0):
        super().__init__()
        self.kernel_size = _ints(kernel_size, "kernel_size", (2,))
        self.stride = _ints(stride, "stride", (2,)) if stride else self.kernel_size
        self.padding = _padding4(padding, "padding")            # (up, down, left, right) from the start, as HIPMaxPool2d
        if min(self.kernel_size) < 1 or min(self.stride) < 1:
            raise ValueError(f"kernel_size and stride must be >= 1, got {kernel_size!r}, {stride!r}")

    def forward(self, X: Tensor) -> Tensor:
        if not isinstance(X, Tensor):
            raise TypeError("Input must be a tensor")
        require_device_f32(X)
        if X.ndim != 4:
            raise ValueError("AvgPool2d expects a (B, C, H, W) input")
        B, C, H, W = X.shape
        kh, kw = self.kernel_size
        sh, sw = self.stride
        pu, pd, pl, pr = self.padding
        Ho = (H + pu + pd - kh) // sh + 1                        # avgpool2d.py:118-123
        Wo = (W + pl + pr - kw) // sw + 1
        if Ho < 1 or Wo < 1:
            raise ValueError(f"AvgPool2d: a {kh} x {kw} window does not fit the padded {H + pu + pd} x {W + pl + pr} input")
        desc = Pool2dDesc(B, C, H, W, kh, kw, sh, sw, pu, pd, pl, pr, 1, 1)
        O = X.xp.empty((B, C, Ho, Wo), dtype=np.float32)
        call_hip_function("nnhipAvgPool2dForward", O, contiguous(X.data), ctypes.byref(desc), get_current_stream_ptr())
        rg = X.requires_grad
        out = Tensor._wrap(O, (X, desc) if rg else None, "avgpool2d", "cuda", requires_grad=rg)

        def grad_fn(t, d, grad):
            grad_X = t.xp.empty((d.B, d.C, d.H, d.W), dtype=np.float32)
            call_hip_function("nnhipAvgPool2dBackward", grad_X, contiguous(grad), ctypes.byref(d), get_current_stream_ptr())
            t.apply_grad(grad_X)

        if rg:
            out.grad_fn = grad_fn
        return out


# ----------------------------------------------------------------------------------------------- ZeroPad2d
class HIPZeroPad2d(Module):
    """neunet/nn/layers/zeropad2d.py: ZeroPad2d(padding), padding an int, (vertical, horizontal) or (up, down, left, right), on a 3-D
    or 4-D device float32 tensor.  Forward: ONE nnhipSliceBackward launch that writes X at (up, left) of the padded tensor and 0
    everywhere else; backward: ONE nnhipSliceForward launch, the crop.  A non-contiguous input is made contiguous first.
    Deviation from the reference: the backward works (the reference assigns `_backward` instead of `grad_fn`, so any backward()
    through its ZeroPad2d raises TypeError)."""

    def __init__(self, padding):
        super().__init__()
        self.padding = _padding4(padding, "padding")

    def forward(self, X: Tensor) -> Tensor:
        from ...tensor_index import slice_forward
        from ...tensor_ops import _i64, contiguous_strides
        if not isinstance(X, Tensor):
            raise TypeError("Input must be a tensor")
        if X.ndim != 3 and X.ndim != 4:
            raise ValueError("X must be 3D or 4D tensor")
        require_device_f32(X)
        pu, pd, pl, pr = self.padding
        shape = tuple(X.shape)
        lead, (H, W) = shape[:-2], shape[-2:]
        padded = lead + (H + pu + pd, W + pl + pr)
        start = (0,) * len(lead) + (pu, pl)
        O = X.xp.empty(padded, dtype=np.float32)
        call_hip_function("nnhipSliceBackward", O, contiguous(X.data), len(padded), _i64(padded), _i64(start), _i64((1,) * len(padded)),
                          _i64(shape), get_current_stream_ptr())
        rg = X.requires_grad
        out = Tensor._wrap(O, (X, self.padding) if rg else None, "zeropad2d", "cuda", requires_grad=rg)
        offset, strides = pu * padded[-1] + pl, contiguous_strides(padded)

        def grad_fn(t, padding, grad):
            t.apply_grad(slice_forward(contiguous(grad), offset, shape, strides))

        if rg:
            out.grad_fn = grad_fn
        return out


# ------------------------------------------------------------------------------------------------- Flatten
class HIPFlatten(Module):
    """neunet/nn/layers/flatten.py: Flatten(start_dim=1, end_dim=-1) = X.reshape(shape[:start] + (prod(shape[start:end + 1]),) +
    shape[end + 1:]), negative dims counted from the end; CPU and device tensors alike.  It goes through X.reshape, so an output that
    is still pending (HIPBatchNorm2d's deferred launch) stays pending.  start > end after normalisation, or a dim outside the
    tensor's rank, raises ValueError (the reference would reshape to a wrong element count and fail inside NumPy)."""

    def __init__(self, start_dim: int = 1, end_dim: int = -1):
        super().__init__()
        self.start_dim = int(start_dim)
        self.end_dim = int(end_dim)

    def forward(self, X: Tensor) -> Tensor:
        if not isinstance(X, Tensor):
            raise TypeError("Input must be a tensor")
        shape, nd = tuple(X.shape), X.ndim
        start = nd + self.start_dim if self.start_dim < 0 else self.start_dim
        end = nd + self.end_dim if self.end_dim < 0 else self.end_dim
        if not (0 <= start < nd and 0 <= end < nd):
            raise ValueError(f"Flatten({self.start_dim}, {self.end_dim}): dim out of range for a tensor of rank {nd}")
        if start > end:
            raise ValueError(f"Flatten({self.start_dim}, {self.end_dim}): start_dim is behind end_dim on a tensor of rank {nd}")
        new_shape = shape[:start] + (int(np.prod(shape[start:end + 1], dtype=np.int64)),) + shape[end + 1:]
        return X.reshape(*new_shape)
