"""HIPConvTranspose2d -- ConvTranspose2d on the stride-phase MFMA kernel (net-new: the reference has no CUDA one).
CPU semantics: neunet/nn/layers/convtranspose2d.py:123-384 (constructor :139-188, geometry in build :190-291, forward
:293-384, backward :16-120).  The weight is [out_channels, in_channels, kh, kw] and is correlated, NOT flipped, with the
zero-stuffed input -- i.e. torch's conv_transpose2d with W.flip(2, 3).transpose(0, 1).  Unlike the reference, weight.data is
never mutated (it dilates the weight in forward and un-dilates it in grad_fn, convtranspose2d.py:303,113)."""
import ctypes
from typing import Union

import numpy as np

from ..._lib import ConvTranspose2dDesc
from ...autograd import Tensor
from ..modules import Module
from ..parameter import Parameter
from .conv2d import _pair, resolve_padding
from .linear import _finish_param, _grad_out
from .utils import call_hip_function, get_current_stream_ptr, require_device_f32

ROUTES = {"auto": 0, "phase": 1, "gather": 2}


def conv_transpose2d_desc(x_shape, w_shape, stride, padding4, dilation, output_padding):
    B, Cin, H, W = x_shape
    Cout, Cin_w, kh, kw = w_shape
    if Cin != Cin_w:
        raise ValueError(f"input has {Cin} channels, weight expects {Cin_w}")
    d = ConvTranspose2dDesc(B, Cin, H, W, Cout, kh, kw, stride[0], stride[1], dilation[0], dilation[1], *padding4, *output_padding)
    Ho = (H - 1) * stride[0] - (padding4[0] + padding4[1]) + dilation[0] * (kh - 1) + output_padding[0] + 1  # convtranspose2d.py:249-262
    Wo = (W - 1) * stride[1] - (padding4[2] + padding4[3]) + dilation[1] * (kw - 1) + output_padding[1] + 1
    return d, (Ho, Wo)


def hip_conv_transpose2d_forward(X, W, bias, O, desc):
    return call_hip_function("nnhipConvTranspose2dForward", X, W, bias, O, ctypes.byref(desc), get_current_stream_ptr())


def hip_conv_transpose2d_backward(X, W, grad_O, grad_X, grad_W, grad_b, desc):
    return call_hip_function("nnhipConvTranspose2dBackward", X, W, grad_O, grad_X, grad_W, grad_b, ctypes.byref(desc),
                             get_current_stream_ptr())


def conv_transpose2d_plan(desc):
    """nnhipConvTranspose2dPlan (host only): (route that `auto` resolves to, taps per stride phase, output pixels per image and
    phase); phases are row-major in ((y + pu) mod sh, (x + pl) mod sw).  Routes: 1 phase, 2 gather, 3 the Conv2d entries."""
    n = int(desc.sh * desc.sw)
    route = ctypes.c_int32(0)
    taps, pixels = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
    got = call_hip_function("nnhipConvTranspose2dPlan", ctypes.byref(desc), ctypes.byref(route), taps, pixels, n)
    if got != n:
        from ..._lib import NeunetHipError, last_error
        raise NeunetHipError(f"nnhipConvTranspose2dPlan failed with status {got}: {last_error()}")
    return route.value, list(taps), list(pixels)


class _HIPConvTranspose2dTensor(Tensor):
    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(X: Tensor, weight: Tensor, bias, desc, grad):
            grad = grad if grad.is_contiguous() else grad.contiguous()
            grad_X = X.xp.empty_like(X.data, dtype=np.float32) if X.requires_grad else None
            grad_W = _grad_out(weight, weight.data)
            grad_b = _grad_out(bias, bias.data) if bias is not None else None
            hip_conv_transpose2d_backward(X.data, weight.data, grad, grad_X, grad_W, grad_b, desc)
            if grad_X is not None:
                X.apply_grad(grad_X)
            _finish_param(weight, grad_W)
            if bias is not None:
                _finish_param(bias, grad_b)

        self.grad_fn = grad_fn


class HIPConvTranspose2d(Module):
    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=(1, 1), padding=(0, 0), dilation=(1, 1),
                 output_padding=(0, 0), bias: bool = True, device="cuda"):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride, self.dilation, self.output_padding = _pair(stride), _pair(dilation), _pair(output_padding)
        self.padding = resolve_padding(padding)
        stdv = 1.0 / np.sqrt(in_channels * self.kernel_size[0] * self.kernel_size[1])  # convtranspose2d.py:165-185
        self.weight = Parameter(Tensor(
            np.random.uniform(-stdv, stdv, (out_channels, in_channels, *self.kernel_size)), dtype=np.float32))
        self.bias: Union[Tensor, None] = Parameter(Tensor(np.zeros(out_channels), dtype=np.float32)) if bias else None
        self.to(device)

    def forward(self, X: Tensor) -> Tensor:
        if not isinstance(X, Tensor):
            raise TypeError("Input must be a tensor")
        if X.device != self.device:
            raise ValueError("Tensors must be on the same device")
        require_device_f32(X)
        if X.ndim != 4:
            raise ValueError("ConvTranspose2d expects a (B, C, H, W) input")
        if not X.data.is_contiguous():
            raise ValueError("HIPConvTranspose2d needs a C-contiguous NCHW input")
        desc, (Ho, Wo) = conv_transpose2d_desc(X.shape, self.weight.shape, self.stride, self.padding, self.dilation,
                                                self.output_padding)
        if Ho <= 0 or Wo <= 0:
            raise ValueError(f"ConvTranspose2d output would be empty ({Ho} x {Wo})")
        O = X.xp.empty((X.shape[0], self.out_channels, Ho, Wo), dtype=np.float32)
        hip_conv_transpose2d_forward(X.data, self.weight.data, self.bias.data if self.bias is not None else None, O, desc)
        return _HIPConvTranspose2dTensor(O, (X, self.weight, self.bias, desc), "conv_transpose2d", self.device)
