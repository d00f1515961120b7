"""HIP activations: drop-ins for CUDASwish (experimental/activations/swish/swish.py:92-120),
CUDAFusedSwishAndMul (.../fused_swish_and_mul/fused_swish_and_mul.py:154-179), CUDASoftmax
(.../softmax/softmax.py:139-169), plus HIPReLU (CPU reference: neunet/nn/activations.py:40-59), HIPTanh (:107-126), HIPSoftplus,
HIPSoftsign, HIPMish, HIPTanhExp, HIPELU, HIPSELU (:140-383) and HIPLogSoftmax (:462-492)."""
import weakref

import numpy as np

from ...autograd import Tensor
from ..modules import Module
from .linear import ACT_RELU, ACT_SWISH, _HIPLinearTensor
from .utils import call_hip_function, contiguous, get_current_stream_ptr, require_device_f32


def _is_device_array(a):
    return hasattr(a, "data_ptr") and a.is_cuda


def _check_arrays(*arrs):
    if not all(_is_device_array(a) for a in arrs):
        raise ValueError("All arguments must be device (torch cuda) arrays.")


# ------------------------------------------------------------------------------------------- ReLU
def hip_relu_forward(x, out):
    _check_arrays(x, out)
    call_hip_function("nnhipReLUForward", out, contiguous(x), x.numel(), get_current_stream_ptr())
    return out


def hip_relu_backward(grad_input, grad_output, f_x):
    _check_arrays(grad_input, grad_output, f_x)
    call_hip_function("nnhipReLUBackward", grad_input, contiguous(grad_output), contiguous(f_x),
                      f_x.numel(), get_current_stream_ptr())
    return grad_input


class _HIPReLUTensor(Tensor):
    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)
        self_ref = weakref.ref(self)

        def grad_fn(t: Tensor, f_x, grad):
            me = self_ref()
            if getattr(me, "_grad_is_dz", False):
                # the consumer (a HIPLinear) already applied [f > 0] in its dX epilogue (linear.py:_plan_fold)
                me._grad_is_dz = False
                t.apply_grad(grad)
                return
            grad_input = t.xp.empty_like(f_x)        # not t.data: t may be a Linear output that was never materialised
            hip_relu_backward(grad_input, grad, f_x)
            t.apply_grad(grad_input)

        self.grad_fn = grad_fn


class HIPReLU(Module):
    def __init__(self):
        super().__init__()

    def forward(self, x: Tensor):
        require_device_f32(x)
        if isinstance(x, _HIPLinearTensor) and x.pending():
            f_x = x.run_fused(ACT_RELU)              # relu in the Linear's GEMM epilogue: one launch instead of two
        else:
            f_x = x.xp.empty_like(x.data)
            hip_relu_forward(x.data, f_x)
        return _HIPReLUTensor(f_x, [x, f_x], "relu", device=x.device)


# ------------------------------------------------------------------------------------------ Swish
def hip_swish_forward(x, out, beta: float):
    """cuda_swish_forward (swish.py:40-63)."""
    _check_arrays(x, out)
    if x.shape != out.shape:
        raise ValueError("Input and output shapes must match")
    call_hip_function("nnhipSwishForward", out, contiguous(x), float(beta), x.numel(), get_current_stream_ptr())
    return out


def hip_swish_backward(grad_input, grad_output, x, beta: float):
    """cuda_swish_backward (swish.py:65-90)."""
    _check_arrays(grad_input, grad_output, x)
    if not (grad_input.shape == grad_output.shape == x.shape):
        raise ValueError("Shapes must match")
    call_hip_function("nnhipSwishBackward", grad_input, contiguous(grad_output), contiguous(x), float(beta),
                      x.numel(), get_current_stream_ptr())
    return grad_input


class _HIPSwishTensor(Tensor):
    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(x: Tensor, beta, grad):
            grad_input = x.xp.empty_like(x.data)
            hip_swish_backward(grad_input, grad, x.data, beta)
            x.apply_grad(grad_input)

        self.grad_fn = grad_fn


class HIPSwish(Module):
    def __init__(self, beta: float = 1.0):
        super().__init__()
        self.beta = beta

    def forward(self, x: Tensor):
        require_device_f32(x)
        if isinstance(x, _HIPLinearTensor) and x.pending():
            # Swish(Linear(x)): one GEMM writes z (the Linear's own output, needed by the Swish backward) and swish(z)
            out = x.run_fused(ACT_SWISH, self.beta, save_preactivation=True)
        else:
            out = x.xp.empty_like(x.data)
            hip_swish_forward(x.data, out, self.beta)
        return _HIPSwishTensor(out, [x, self.beta], "swish", device=x.device)


# ------------------------------------------------------------------------------------------- GELU
def hip_gelu_forward(x, out):
    """GELU, tanh form (neunet/nn/activations.py:412-417) -> nnhipGELUForward."""
    _check_arrays(x, out)
    if x.shape != out.shape:
        raise ValueError("Input and output shapes must match")
    call_hip_function("nnhipGELUForward", out, contiguous(x), x.numel(), get_current_stream_ptr())
    return out


def hip_gelu_backward(grad_input, grad_output, x):
    """The exact derivative of the tanh form (the reference's, activations.py:396-401, rounds its constants to six digits)."""
    _check_arrays(grad_input, grad_output, x)
    if not (grad_input.shape == grad_output.shape == x.shape):
        raise ValueError("Shapes must match")
    call_hip_function("nnhipGELUBackward", grad_input, contiguous(grad_output), contiguous(x), x.numel(), get_current_stream_ptr())
    return grad_input


class _HIPGELUTensor(Tensor):
    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(x: Tensor, grad):
            grad_input = x.xp.empty_like(x.data)
            hip_gelu_backward(grad_input, grad, x.data)
            x.apply_grad(grad_input)

        self.grad_fn = grad_fn


class HIPGELU(Module):
    def __init__(self):
        super().__init__()

    def forward(self, x: Tensor):
        require_device_f32(x)
        out = x.xp.empty_like(x.data)
        hip_gelu_forward(x.data, out)
        return _HIPGELUTensor(out, [x], "gelu", device=x.device)


# ------------------------------------------------------------------------------------------- Tanh
class _HIPTanhTensor(Tensor):
    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(t: Tensor, f_x, grad):
            grad_input = t.xp.empty_like(f_x)        # not t.data: t may be a Linear output that was never materialised
            call_hip_function("nnhipTanhBackward", grad_input, contiguous(grad), f_x, f_x.numel(), get_current_stream_ptr())
            t.apply_grad(grad_input)

        self.grad_fn = grad_fn


class HIPTanh(Module):
    """neunet/nn/activations.py:107-126: f = tanh(x); the backward reads the saved output, dx = dy (1 - f^2)."""

    def __init__(self):
        super().__init__()

    def forward(self, x: Tensor):
        require_device_f32(x)
        xd = contiguous(x.data)
        f_x = x.xp.empty_like(xd)
        call_hip_function("nnhipTanhForward", f_x, xd, f_x.numel(), get_current_stream_ptr())
        return _HIPTanhTensor(f_x, [x, f_x], "tanh", device=x.device)


# -------------------------------------------------------------------------------- SwiGLU gate
def hip_fused_swish_and_mul(x, out, beta: float = 1.0, hidden_size=None):
    """cuda_fused_swish_and_mul (fused_swish_and_mul.py:44-89): x rows = [gate | up]."""
    _check_arrays(x, out)
    if x.ndim < 1:
        raise ValueError("Input must have at least 1 dimension.")
    if hidden_size is None:
        hidden_size = out.shape[-1]
    if hidden_size <= 0:
        raise ValueError("hidden_size must be > 0.")
    if x.shape[-1] != hidden_size * 2:
        raise ValueError("Input last dimension must be exactly 2 * hidden_size.")
    if tuple(out.shape) != tuple(x.shape[:-1]) + (hidden_size,):
        raise ValueError("Output shape must be input.shape[:-1] + (hidden_size,).")
    call_hip_function("nnhipFusedSwishAndMul", out, contiguous(x), float(beta), hidden_size, out.numel(),
                      get_current_stream_ptr())
    return out


def hip_fused_swish_and_mul_backward(grad_input, grad_output, x, beta: float = 1.0, hidden_size=None):
    """cuda_fused_swish_and_mul_backward (fused_swish_and_mul.py:92-135)."""
    _check_arrays(grad_input, grad_output, x)
    if hidden_size is None:
        hidden_size = grad_output.shape[-1]
    if hidden_size <= 0:
        raise ValueError("hidden_size must be > 0.")
    if x.shape[-1] != hidden_size * 2:
        raise ValueError("Input last dimension must be exactly 2 * hidden_size.")
    if tuple(grad_output.shape) != tuple(x.shape[:-1]) + (hidden_size,):
        raise ValueError("grad_output shape must be input.shape[:-1] + (hidden_size,).")
    if grad_input.shape != x.shape:
        raise ValueError("grad_input shape must match input shape.")
    call_hip_function("nnhipFusedSwishAndMulBackward", grad_input, contiguous(grad_output), contiguous(x),
                      float(beta), hidden_size, grad_output.numel(), get_current_stream_ptr())
    return grad_input


class _HIPFusedSwishAndMulTensor(Tensor):
    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(x: Tensor, beta: float, grad):
            grad_input = x.xp.empty_like(x.data)
            hip_fused_swish_and_mul_backward(grad_input, grad, x.data, beta=beta)
            x.apply_grad(grad_input)

        self.grad_fn = grad_fn


class HIPFusedSwishAndMul(Module):
    def __init__(self, beta: float = 1.0):
        super().__init__()
        self.beta = beta

    def forward(self, x: Tensor):
        require_device_f32(x)
        if x.ndim < 1:
            raise ValueError("Input must have at least 1 dimension.")
        if x.shape[-1] % 2 != 0:
            raise ValueError("Input last dimension must be divisible by 2.")
        hidden = x.shape[-1] // 2
        out = x.xp.empty(x.shape[:-1] + (hidden,), dtype=np.float32)
        hip_fused_swish_and_mul(x.data, out, beta=self.beta)
        return _HIPFusedSwishAndMulTensor(out, [x, self.beta], "fused_swish_and_mul", device=x.device)


# ---------------------------------------------------------------------------- Softmax, LogSoftmax
def _slices(a, dim):
    dim = dim % a.ndim
    slice_size = a.shape[dim]
    num_slices = a.numel() // slice_size if slice_size else 0
    stride = a.stride(dim)  # elements (softmax.py:83 divides byte strides by itemsize)
    return num_slices, slice_size, stride


def _slice_forward(entry, x, o, dim):
    """Both families' forward: arbitrary axis through (num_slices, slice_size, stride)."""
    _check_arrays(x, o)
    if x.shape != o.shape:
        raise ValueError("Input and output shapes must match")
    x = contiguous(x)
    n, s, st = _slices(x, dim)
    call_hip_function(entry, o, x, n, s, st, get_current_stream_ptr())
    return o


def _slice_backward(entry, what, grad_x, grad, f_x, dim):
    _check_arrays(grad_x, grad, f_x)
    if grad_x.shape != grad.shape or grad_x.shape != f_x.shape:
        raise ValueError(f"Input, output gradients and {what} shapes must match")
    grad, f_x = contiguous(grad), contiguous(f_x)
    n, s, st = _slices(f_x, dim)
    call_hip_function(entry, grad_x, grad, f_x, n, s, st, get_current_stream_ptr())
    return grad_x


def hip_softmax_forward(x, o, dim: int):
    """cuda_softmax_forward (softmax.py:52-94)."""
    return _slice_forward("nnhipSoftmaxForward", x, o, dim)


def hip_softmax_backward(grad_x, grad, f_x, dim: int):
    """cuda_softmax_backward (softmax.py:96-136)."""
    return _slice_backward("nnhipSoftmaxBackward", "softmax", grad_x, grad, f_x, dim)


def hip_logsoftmax_forward(x, o, dim: int):
    """neunet/nn/activations.py:485-488 -> nnhipLogSoftmaxForward."""
    return _slice_forward("nnhipLogSoftmaxForward", x, o, dim)


def hip_logsoftmax_backward(grad_x, grad, f_x, dim: int):
    """neunet/nn/activations.py:466-471: grad - exp(f_x) * grad.sum(axis) -> nnhipLogSoftmaxBackward."""
    return _slice_backward("nnhipLogSoftmaxBackward", "log-softmax", grad_x, grad, f_x, dim)


class _HIPSliceTensor(Tensor):
    """args = [input, output, axis].  `_backward_name`: the family's module-level helper, looked up when the gradient runs."""

    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)
        name = self._backward_name

        def grad_fn(t: Tensor, f_x, axis, grad):
            grad_x = t.xp.empty_like(f_x)
            globals()[name](grad_x, grad, f_x, axis)
            t.apply_grad(grad_x)

        self.grad_fn = grad_fn


class _HIPSoftmaxTensor(_HIPSliceTensor):
    _backward_name = "hip_softmax_backward"


class HIPSoftmax(Module):
    def __init__(self, axis: int = 1):
        super().__init__()
        self.axis = axis

    def forward(self, x: Tensor):
        require_device_f32(x)
        f_x = x.xp.empty_like(x.data)
        hip_softmax_forward(x.data, f_x, self.axis)
        return _HIPSoftmaxTensor(f_x, [x, f_x, self.axis], "softmax", device=x.device)


class _HIPLogSoftmaxTensor(_HIPSliceTensor):
    """HIPNLLLoss looks at this node's args to fold its backward into this node's (losses.py)."""

    _backward_name = "hip_logsoftmax_backward"


class HIPLogSoftmax(Module):
    """neunet/nn/activations.py:476-492: x - max - log(sum(exp(x - max))) along `axis`; the tensor saves its output."""

    def __init__(self, axis: int = 1):
        super().__init__()
        self.axis = axis

    def forward(self, x: Tensor):
        require_device_f32(x)
        f_x = x.xp.empty_like(x.data)
        hip_logsoftmax_forward(x.data, f_x, self.axis)
        return _HIPLogSoftmaxTensor(f_x, [x, f_x, self.axis], "log_softmax", device=x.device)


# ---------------------------------------------- Softplus, Softsign, Mish, TanhExp, ELU, SELU, log
ACT_SOFTPLUS, ACT_SOFTSIGN, ACT_MISH, ACT_TANHEXP, ACT_ELU, ACT_SELU, ACT_LOG = range(7)     # NNHIP_ACT_* (include/neunet_hip.h)


class _HIPActivationTensor(Tensor):
    """args = [input, kind, alpha]: the backward reads the saved INPUT (nnhipActivationBackward)."""

    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(t: Tensor, kind, alpha, grad):
            xd = contiguous(t.data)
            grad_input = t.xp.empty_like(xd)
            call_hip_function("nnhipActivationBackward", kind, grad_input, contiguous(grad), xd, float(alpha), xd.numel(),
                              get_current_stream_ptr())
            t.apply_grad(grad_input)

        self.grad_fn = grad_fn


def hip_activation(x: Tensor, kind: int, op: str, alpha: float = 0.0) -> Tensor:
    """One nnhipActivationForward launch on the tape (also Tensor.log, autograd.py)."""
    require_device_f32(x)
    xd = contiguous(x.data)
    f_x = x.xp.empty_like(xd)
    call_hip_function("nnhipActivationForward", kind, f_x, xd, float(alpha), f_x.numel(), get_current_stream_ptr())
    return _HIPActivationTensor(f_x, [x, kind, alpha], op, device=x.device)


class HIPSoftplus(Module):
    """neunet/nn/activations.py:140-160: log(1 + exp(x)), evaluated as max(x, 0) + log1p(exp(-|x|)) (finite above 88, relative
    accuracy below -17 where the reference's float32 expression is inf / exactly 0); dx = dy sigmoid(x)."""

    def __init__(self):
        super().__init__()

    def forward(self, x: Tensor):
        return hip_activation(x, ACT_SOFTPLUS, "softplus")


class HIPSoftsign(Module):
    """neunet/nn/activations.py:174-194: x / (1 + |x|); dx = dy / (1 + |x|)^2."""

    def __init__(self):
        super().__init__()

    def forward(self, x: Tensor):
        return hip_activation(x, ACT_SOFTSIGN, "softsign")


class HIPMish(Module):
    """neunet/nn/activations.py:250-279: x tanh(softplus(x)); the derivative in the form t + x sigmoid(x) (1 - t^2), which has no
    exp(3x) to overflow."""

    def __init__(self):
        super().__init__()

    def forward(self, x: Tensor):
        return hip_activation(x, ACT_MISH, "mish")


class HIPTanhExp(Module):
    """neunet/nn/activations.py:293-317: x tanh(exp(x)); dx = dy (t + x exp(x) (1 - t^2)), the second term dropped once 1 - t^2 is 0."""

    def __init__(self):
        super().__init__()

    def forward(self, x: Tensor):
        return hip_activation(x, ACT_TANHEXP, "tanh_exp")


class HIPELU(Module):
    """neunet/nn/activations.py:331-354, same constructor: x <= 0 ? alpha (exp(x) - 1) : x; the derivative at 0 is alpha."""

    def __init__(self, alpha=0.1):
        super().__init__()
        self.alpha = alpha

    def forward(self, x: Tensor):
        return hip_activation(x, ACT_ELU, "elu", self.alpha)


class HIPSELU(Module):
    """neunet/nn/activations.py:357-383: lambda (x > 0 ? x : alpha (exp(x) - 1)) with the reference's two constants (held by the
    kernel; the attributes are informational)."""

    def __init__(self):
        super().__init__()
        self.alpha = 1.6732632423543772848170429916717
        self.lmbda = 1.0507009873554804934193349852946

    def forward(self, x: Tensor):
        return hip_activation(x, ACT_SELU, "selu")


CUDASwish, CUDAFusedSwishAndMul, CUDASoftmax = HIPSwish, HIPFusedSwishAndMul, HIPSoftmax
