"""HIPBatchNorm1d -- neunet/nn/layers/batchnorm1d.py:46-109 on the column-strip kernels of csrc/batchnorm1d.hip
(nnhipBatchNorm1dForward / nnhipBatchNorm1dBackward): one launch per direction, whatever the batch size."""
from typing import Union

import numpy as np

from ...autograd import Tensor
from ..modules import Module
from ..parameter import Parameter
from .linear import _finish_param, _grad_out
from .utils import call_hip_function, contiguous, get_current_stream_ptr, require_device_f32


class _HIPBatchNorm1dTensor(Tensor):
    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(X: Tensor, weight, bias, xd, save_mean, save_inv, affine, grad):
            N, F = xd.shape
            grad_X = X.xp.empty_like(xd)
            gw = _grad_out(weight, weight.data) if affine else None
            gb = _grad_out(bias, bias.data) if affine else None
            call_hip_function("nnhipBatchNorm1dBackward", contiguous(grad), xd, weight.data if affine else None, save_mean, save_inv,
                              grad_X, gw, gb, N, F, get_current_stream_ptr())
            X.apply_grad(grad_X)
            if affine:
                _finish_param(weight, gw)
                _finish_param(bias, gb)

        self.grad_fn = grad_fn


class HIPBatchNorm1d(Module):
    """neunet/nn/layers/batchnorm1d.py:46-109, same constructor.  weight / bias / running statistics keep the reference's (1, F)
    shape; running_mean / running_var are Parameters with requires_grad=False (in state_dict, not in parameters()).  Training:
    batch mean and biased variance over axis 0, running = momentum * running + (1 - momentum) * stat (the reference's convention,
    not torch's); eval: the running statistics.  The backward is the reference's one formula in both modes.

    The input must be 2-D, [N, F] with F == num_features: anything else raises ValueError.  (The reference layer accepts a 3-D
    [N, C, L] input without complaint, but its axis-0 mean then has shape (1, C, L) and the running-statistics update broadcasts
    (1, C) against it -- the layer corrupts its own running statistics; that is not a behaviour to reproduce.)

    The forward launches when it is called: no deferral."""

    def __init__(self, num_features: int, eps: float = 1e-5, momentum: float = 0.1, affine: bool = True, device="cuda"):
        super().__init__()
        self.num_features, self.eps, self.momentum, self.affine = num_features, eps, momentum, affine
        self.running_mean = Parameter(Tensor(np.zeros((1, num_features)), dtype=np.float32), requires_grad=False)
        self.running_var = Parameter(Tensor(np.ones((1, num_features)), dtype=np.float32), requires_grad=False)
        self.weight: Union[Tensor, None] = Parameter(Tensor(np.ones((1, num_features)), dtype=np.float32)) if affine else None
        self.bias: Union[Tensor, None] = Parameter(Tensor(np.zeros((1, num_features)), dtype=np.float32)) if affine else None
        self.training = True
        self.to(device)

    def forward(self, X: Tensor) -> Tensor:
        if not isinstance(X, Tensor):
            raise TypeError("Input must be a tensor")
        if X.device != self.device:
            raise ValueError("Tensors must be on the same device")
        if X.ndim != 2 or X.shape[1] != self.num_features:
            raise ValueError(f"BatchNorm1d expects a 2-D (N, F) input with F == num_features = {self.num_features} (got {tuple(X.shape)})")
        N, F = X.shape
        if N < 1:
            raise ValueError("BatchNorm1d needs at least one row")
        require_device_f32(X)
        xd = contiguous(X.data)
        O = X.xp.empty_like(xd)
        save_mean = X.xp.empty((F,), dtype=np.float32)
        save_inv = X.xp.empty((F,), dtype=np.float32)
        w = self.weight.data if self.affine else None
        b = self.bias.data if self.affine else None
        call_hip_function("nnhipBatchNorm1dForward", xd, w, b, O, save_mean, save_inv, self.running_mean.data, self.running_var.data,
                          N, F, float(self.eps), float(self.momentum), int(bool(self.training)), get_current_stream_ptr())
        return _HIPBatchNorm1dTensor(O, (X, self.weight, self.bias, xd, save_mean, save_inv, self.affine), "batchnorm", device=self.device)

    def train(self, mode=True):
        self.training = mode

    def eval(self):
        self.training = False
