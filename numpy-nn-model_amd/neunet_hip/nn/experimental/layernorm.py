"""HIPLayerNorm -- nn.LayerNorm on the row kernels of csrc/rowops.hip (ABI 212, net-new: the reference has no CUDA LayerNorm).
CPU semantics: neunet/nn/layers/layernorm.py:115-147 (fwd), :48-93 (bwd).

A multi-axis normalized_shape is one row of prod(normalized_shape) columns.  The forward saves mean and rstd (one float per row
each); the reference saves X_centered, a whole extra tensor -- the backward recomputes xhat from X.  Parameter gradients are the
full sums over every leading axis: the reference sums over axis 0 only and lets apply_grad's reverse broadcast finish
(layernorm.py:87-88 + autograd.py:948-962), which is the same number."""
from typing import Union

import numpy as np

from ...autograd import Tensor
from ..modules import Module
from ..parameter import Parameter
from .linear import _finish_param, _grad_out
from .utils import call_hip_function, contiguous, get_current_stream_ptr, require_device_f32


def layernorm_forward(X, weight, bias, O, mean, rstd, n_cols: int, eps: float):
    if X.shape != O.shape:
        raise ValueError("Input and output shapes must match")
    n_rows = X.numel() // n_cols if n_cols else 0
    call_hip_function("nnhipLayerNormForward", contiguous(X), weight, bias, O, mean, rstd, n_rows, n_cols, float(eps),
                      get_current_stream_ptr())
    return O, mean, rstd


def layernorm_backward(X, weight, grad_O, grad_X, grad_weight, grad_bias, mean, rstd, n_cols: int, grad_X_addend=None):
    """grad_X_addend (extension): grad_X = layernorm gradient + addend in the same pass (nnhipLayerNormBackwardEx)."""
    if X.shape != grad_O.shape or grad_X.shape != X.shape:
        raise ValueError("Input, output and gradient shapes must match")
    n_rows = X.numel() // n_cols if n_cols else 0
    if grad_X_addend is None:
        call_hip_function("nnhipLayerNormBackward", contiguous(grad_O), contiguous(X), weight, mean, rstd, grad_X, grad_weight,
                          grad_bias, n_rows, n_cols, get_current_stream_ptr())
    else:
        call_hip_function("nnhipLayerNormBackwardEx", contiguous(grad_O), contiguous(X), weight, mean, rstd, grad_X_addend, grad_X,
                          grad_weight, grad_bias, n_rows, n_cols, get_current_stream_ptr())
    return grad_X, grad_weight, grad_bias


class _HIPLayerNormTensor(Tensor):
    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(X: Tensor, weight, bias, mean, rstd, n_cols, grad):
            grad_X = X.xp.empty_like(X.data, dtype=np.float32)
            grad_weight = _grad_out(weight, weight.data) if weight is not None else None
            grad_bias = _grad_out(bias, bias.data) if bias is not None else None
            held = X.foldable_grad() if X.requires_grad else None   # e.g. the residual branch's gradient (pre-norm blocks)
            layernorm_backward(X.data, weight.data if weight is not None else None, grad, grad_X, grad_weight, grad_bias,
                               mean, rstd, n_cols, grad_X_addend=held)
            if held is not None:
                X.grad = grad_X
            else:
                X.apply_grad(grad_X)
            if weight is not None:
                _finish_param(weight, grad_weight)
            if bias is not None:
                _finish_param(bias, grad_bias)

        self.grad_fn = grad_fn


class HIPLayerNorm(Module):
    """nn.LayerNorm(normalized_shape, eps=1e-5, elementwise_affine=True): parameters `weight` (ones) and `bias` (zeros) of shape
    normalized_shape, as the reference class (layernorm.py:98-113)."""

    def __init__(self, normalized_shape: Union[int, tuple], eps: float = 1e-5, elementwise_affine: bool = True, device="cuda"):
        super().__init__()
        self.normalized_shape = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
        self.eps = eps
        self.elementwise_affine = elementwise_affine
        if elementwise_affine:
            self.weight: Union[Parameter, None] = Parameter(Tensor(np.ones(self.normalized_shape), dtype=np.float32))
            self.bias: Union[Parameter, None] = Parameter(Tensor(np.zeros(self.normalized_shape), dtype=np.float32))
        else:
            self.weight = None
            self.bias = None
        self.to(device)

    def forward(self, X: Tensor) -> Tensor:
        if not isinstance(X, Tensor):
            raise TypeError("Input must be a tensor")
        require_device_f32(X)
        k = len(self.normalized_shape)
        if tuple(X.shape[-k:]) != self.normalized_shape:
            raise ValueError(f"Expected trailing dims {self.normalized_shape}, got {tuple(X.shape[-k:])}")
        n_cols = int(np.prod(self.normalized_shape))
        lead = tuple(X.shape[:-k])
        mean = X.xp.empty(lead + (1,), dtype=np.float32)
        rstd = X.xp.empty(lead + (1,), dtype=np.float32)
        O = X.xp.empty_like(X.data)
        layernorm_forward(X.data, self.weight.data if self.weight is not None else None,
                          self.bias.data if self.bias is not None else None, O, mean, rstd, n_cols, self.eps)
        return _HIPLayerNormTensor(O, (X, self.weight, self.bias, mean, rstd, n_cols), "layernorm", device=self.device)
