"""Host-side Tensor + tape: the dispatch hook of the drop-in boundary.

Restates the contract of neunet/autograd.py that the accelerated layers rely on -- and only that:
  * Tensor(data, args, op, requires_grad, dtype, device)           (autograd.py:7-26)
  * apply_grad: reverse-broadcast then assign / accumulate-by-allocation  (autograd.py:85-93, 948-962)
  * backward: seed ones, DFS topological sort over `args`, replay `grad_fn(*args, grad=v.grad)`
    in reverse                                                        (autograd.py:965-1002)
The arithmetic core of the reference Tensor -- the broadcasting binary ops and their operators, the unary maps, the axis
reductions, transpose / swapaxes / .T and matmul (autograd.py:96-531, 588-640, 810-893) -- runs on the device through
tensor_ops.py (csrc/tensor_ops.hip); comparisons and logical ops, where, flip, __getitem__ / __setitem__ (autograd.py:642-808,
895-923) run through tensor_index.py (csrc/tensor_index.hip) on float32, int32, int64 and bool tensors, and in NumPy on a CPU
tensor.  Boolean-mask __getitem__ (a data-dependent shape) and comparisons between tensors of different dtypes are not provided.

Device arrays: on device "cuda" `Tensor.data` is a torch.Tensor living in HBM (torch-ROCm plays the
role CuPy plays in the reference: allocation + streams only); on "cpu" it is a numpy.ndarray and the
Tensor is only a container -- the dense ops themselves run on "cuda" exclusively (no CPU fallback).
"""
from __future__ import annotations

from typing import Any, Callable, Literal

import numpy as np

from . import _lib

try:  # torch is plumbing: device memory, streams, process groups
    import torch
except Exception:  # pragma: no cover - torch is part of the image
    torch = None

_NP2T = {}
if torch is not None:
    _NP2T = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
             np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
             np.dtype(np.int16): torch.int16, np.dtype(np.bool_): torch.bool,
             np.dtype(np.uint8): torch.uint8}
_T2NP = {v: k for k, v in _NP2T.items()}


def _torch_dtype(dt):
    if dt is None:
        return torch.float32
    if torch is not None and isinstance(dt, torch.dtype):
        return dt
    return _NP2T[np.dtype(dt)]


class _DeviceXP:
    """The few array-module calls the accelerated layers make on `X.xp` (the reference uses cupy)."""
    float32 = np.float32
    int32 = np.int32

    @staticmethod
    def empty(shape, dtype=np.float32):
        return torch.empty(tuple(np.atleast_1d(shape).tolist()) if not isinstance(shape, tuple) else shape,
                           dtype=_torch_dtype(dtype), device="cuda")

    @staticmethod
    def zeros(shape, dtype=np.float32):
        return torch.zeros(shape, dtype=_torch_dtype(dtype), device="cuda")

    @staticmethod
    def empty_like(a, dtype=None):
        return torch.empty_like(a, dtype=_torch_dtype(dtype) if dtype is not None else None,
                                memory_format=torch.contiguous_format)

    @staticmethod
    def zeros_like(a, dtype=None):
        return torch.zeros_like(a, dtype=_torch_dtype(dtype) if dtype is not None else None,
                                memory_format=torch.contiguous_format)

    @staticmethod
    def ones_like(a, dtype=None):
        return torch.ones_like(a, dtype=_torch_dtype(dtype) if dtype is not None else None,
                               memory_format=torch.contiguous_format)

    @staticmethod
    def ascontiguousarray(a):
        return a.contiguous()


device_xp = _DeviceXP()


def _to_device_array(data, dtype):
    td = _torch_dtype(dtype)
    if isinstance(data, torch.Tensor):
        return data.to(device="cuda", dtype=td).contiguous().clone() if not data.is_cuda or data.dtype != td \
            else data.contiguous().clone()
    arr = np.ascontiguousarray(np.array(data, dtype=_T2NP[td]))
    return torch.from_numpy(arr).to("cuda")


# Parameter epoch: advanced by every in-place parameter update (optimizer.step(), a graph replay).  A deferred kernel output
# (experimental/linear.py: the lazily launched Linear GEMM) remembers the epoch it was created in; materialising it in a
# LATER epoch would silently compute with the updated weights, so that read raises instead.
_param_epoch = [0]


def param_epoch() -> int:
    return _param_epoch[0]


def bump_param_epoch() -> None:
    _param_epoch[0] += 1


def add_arrays(a, b):
    """apply_grad's `self.grad + grad` (autograd.py:93).  On device: one nnhipAdd launch."""
    if isinstance(a, np.ndarray):
        return a + b
    if a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape \
            and a.is_contiguous() and b.is_contiguous():
        out = torch.empty_like(a)
        _lib.call_hip_function("nnhipAdd", out, a, b, a.numel(), _lib.get_current_stream_ptr())
        return out
    return a + b


class Tensor:
    def __init__(self, data: Any, args=None, op=None, requires_grad: bool = True, dtype=None,
                 device: Literal["cpu", "cuda"] = "cpu", _nocopy: bool = False):
        if device not in ("cpu", "cuda"):
            raise ValueError("Device must be 'cpu' or 'cuda'")
        if isinstance(data, Tensor):
            data = data.data
        if _nocopy:
            # kernel outputs are wrapped, not copied (the reference's `xp.array(data)` in
            # Tensor.__init__ re-copies every op output, autograd.py:15-19)
            self.xp = np if device == "cpu" else device_xp
            self.data = data
        elif device == "cpu":
            self.xp = np
            if torch is not None and isinstance(data, torch.Tensor):
                data = data.detach().cpu().numpy()
            self.data = np.array(data, dtype=dtype if dtype else np.float32)
        else:
            self.xp = device_xp
            self.data = _to_device_array(data, dtype)
        self.grad = None
        self.op = op
        self.args = args
        self.requires_grad = requires_grad
        self.device = device
        self.grad_fn: Callable = lambda *a, **k: None

    # ---- gradient slot ------------------------------------------------------------------------------------------------
    # `grad` is a plain slot except while a backward kernel that produces it is still PENDING (experimental/linear.py:
    # _PendingMLPBackward -- the README MLP's one-launch backward waits for optimizer.step() so that the same launch can
    # apply Adam; whoever reads a gradient first makes the launch happen, so a reader never sees anything but the
    # finished gradient the reference's eager backward would have left, autograd.py:85-93).
    _pending = None

    @property
    def grad(self):
        pend = self._pending
        if pend is not None:
            pend.materialize()
        return self._grad

    @grad.setter
    def grad(self, value):
        pend = self._pending
        if pend is not None:
            pend.detach(self)       # the caller's value replaces what that backward pass would have left here
        self._grad = value

    # ---- wrapping an already-allocated device buffer without a copy (outputs of kernels) --------
    @classmethod
    def _wrap(cls, array, args, op, device, requires_grad=True):
        t = cls.__new__(cls)
        t.xp = np if device == "cpu" else device_xp
        t.data = array
        t.grad = None
        t.op = op
        t.args = args
        t.requires_grad = requires_grad
        t.device = device
        t.grad_fn = lambda *a, **k: None
        return t

    # ---- movement ---------------------------------------------------------------------------------
    def to(self, device):
        if device == self.device:
            return self
        if device not in ("cpu", "cuda"):
            raise ValueError("Device must be 'cpu' or 'cuda'")
        return Tensor(self.data, requires_grad=self.requires_grad, dtype=self.dtype, device=device)

    def cpu(self):
        return self.to("cpu")

    def cuda(self):
        return self.to("cuda")

    def numpy(self) -> np.ndarray:
        """Host copy of the data (the reference's numpy() refuses device tensors; ours copies)."""
        if self.device == "cpu":
            return self.data
        return self.data.detach().cpu().numpy()

    def detach(self):
        return Tensor._wrap(self.data, None, self.op, self.device, requires_grad=False)

    def item(self) -> float:
        return float(self.data.item())

    @property
    def shape(self):
        return tuple(self.data.shape)

    @property
    def dtype(self):
        if isinstance(self.data, np.ndarray):
            return self.data.dtype
        return _T2NP[self.data.dtype]

    @property
    def ndim(self):
        return self.data.ndim

    @property
    def size(self):
        return int(np.prod(self.shape)) if self.shape else 1

    # ---- tape ---------------------------------------------------------------------------------------
    def _reverse_broadcast(self, grad):
        """autograd.py:948-962."""
        gshape, sshape = tuple(grad.shape), tuple(self.shape)    # .shape, not .data.shape: a deferred Linear output stays deferred
        if gshape == sshape:
            return grad
        if len(sshape) == grad.ndim:
            axes = tuple(i for i, (a, b) in enumerate(zip(sshape, gshape)) if a != b)
            grad = grad.sum(axes, keepdims=True) if isinstance(grad, np.ndarray) else grad.sum(axes, keepdim=True)
        else:
            padded = (1,) * (grad.ndim - len(sshape)) + sshape
            axes = tuple(i for i, (a, b) in enumerate(zip(padded, gshape)) if a != b)
            grad = grad.sum(axis=axes) if isinstance(grad, np.ndarray) else grad.sum(axes)
        return grad.reshape(sshape)

    def apply_grad(self, grad):
        """autograd.py:85-93: first gradient is kept by reference, later ones accumulate by allocation."""
        if not self.requires_grad:
            return
        grad = self._reverse_broadcast(grad)
        if self.grad is None:
            self.grad = grad
        else:
            self.grad = add_arrays(self.grad, grad)

    def foldable_grad(self):
        """The gradient this tensor already holds, if a kernel can fold it into the next one it produces
        (out = new + held, written to a fresh buffer): same shape, contiguous.  None otherwise."""
        g = self.grad
        if g is None or isinstance(g, np.ndarray) or tuple(g.shape) != tuple(self.shape) or not g.is_contiguous():
            return None
        return g

    def backward(self, grad=None):
        """autograd.py:965-1002."""
        if not self.requires_grad:
            return
        self._seeded_with_ones = grad is None
        if grad is None and getattr(self, "_implicit_seed", False):
            # a loss tensor whose grad_fn already holds d(loss)/d(input) for a unit seed (fused CrossEntropy / MSE):
            # no ones tensor, no fill launch -- its grad_fn ignores `grad` when `_seeded_with_ones` is set
            grad = None
        elif grad is None:
            grad = self.xp.ones_like(self.data, dtype=self.dtype)
        elif self.device == "cpu":
            grad = np.array(grad, dtype=self.dtype)
        else:
            grad = _to_device_array(grad.data if isinstance(grad, Tensor) else grad, self.dtype)
        if grad is not None:
            self.apply_grad(grad)

        tape: list = []
        visited: set = set()
        # iterative post-order DFS (the reference recurses; deep graphs would hit the recursion limit)
        stack = [(self, False)]
        while stack:
            v, expanded = stack.pop()
            if expanded:
                tape.append(v)
                continue
            if id(v) in visited:
                continue
            visited.add(id(v))
            if v.args is None:
                continue
            stack.append((v, True))
            for child in reversed(list(v.args)):
                if isinstance(child, Tensor) and child.requires_grad and id(child) not in visited:
                    stack.append((child, False))
        # how many tape nodes consume each tensor: lets a grad_fn hand a *transformed* gradient to a sole-consumer
        # input (experimental/linear.py folds the Swish backward of a LinearSwish input into its dX GEMM)
        for v in tape:
            for child in v.args:
                if isinstance(child, Tensor):
                    child._consumers = 0
        for v in tape:
            for child in v.args:
                if isinstance(child, Tensor):
                    child._consumers += 1
        # small parameter-gradient GEMMs are queued by the library while the tape is walked and launched a layer's worth at a
        # time (_lib.py: deferred parameter gradients); everything is launched by the time backward() returns
        from ._lib import wgrad_begin, wgrad_end
        deferring = self.device != "cpu" and wgrad_begin()
        try:
            for v in reversed(tape):
                if getattr(v, "_bwd_done", False):      # a consumer's fused backward already produced this node's gradients
                    v._bwd_done = False                 # (experimental/linear.py: Linear2(relu(Linear1(x))) in one launch)
                    continue
                v.grad_fn(*v.args, grad=v.grad)
        finally:
            if deferring:
                wgrad_end()

    # ---- the few shape / scalar ops callers of the hot path need ----------------------------------------
    def reshape(self, *shape):
        shape = shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        out = Tensor._wrap(self.data.reshape(*shape) if not isinstance(self.data, np.ndarray)
                           else self.data.reshape(shape), (self,), "reshape", self.device, self.requires_grad)

        def grad_fn(t, grad):
            t.apply_grad(grad.reshape(t.shape))

        out.grad_fn = grad_fn
        return out

    def add(self, t) -> "Tensor":
        """out = self + t (neunet/autograd.py:96-116), both parents receive the gradient.  Same shape, contiguous, float32 is the residual
        add of the hot path: one nnhipAdd.  Anything else on the device broadcasts (tensor_ops.binary); the same-shape CPU add stays."""
        if isinstance(t, Tensor) and tuple(t.shape) == tuple(self.shape):
            if t.device != self.device:
                raise ValueError("Tensors must be on the same device")
            rg = self.requires_grad or t.requires_grad
            out = Tensor(add_arrays(self.data, t.data), (self, t) if rg else None, "add", requires_grad=rg,
                         device=self.device, _nocopy=True)

            def grad_fn(a, b, grad):
                if a.requires_grad:
                    a.apply_grad(grad)
                if b.requires_grad:
                    b.apply_grad(grad)

            out.grad_fn = grad_fn
            return out
        if isinstance(t, Tensor):
            if t.device != self.device:
                raise ValueError("Tensors must be on the same device")
            from .tensor_ops import broadcast_shape
            broadcast_shape(self.shape, t.shape)        # ValueError when the shapes do not broadcast, on either device
        return self._binary(t, "add")

    def _binary(self, t, op, reflected=False):
        from .tensor_ops import binary
        return binary(self, t, op, reflected)

    def sub(self, t) -> "Tensor":
        return self._binary(t, "sub")

    def mul(self, t) -> "Tensor":
        return self._binary(t, "mul")

    def div(self, t) -> "Tensor":
        return self._binary(t, "div")

    def power(self, t) -> "Tensor":
        return self._binary(t, "power")

    def maximum(self, t) -> "Tensor":
        """NaN from either side propagates (np.maximum); on a tie both operands receive the gradient (autograd.py:456-460)."""
        return self._binary(t, "maximum")

    def minimum(self, t) -> "Tensor":
        return self._binary(t, "minimum")

    __add__ = add
    __sub__ = sub
    __mul__ = mul
    __truediv__ = div
    __pow__ = power

    def __radd__(self, t):
        return self._binary(t, "add", reflected=True)

    def __rsub__(self, t):
        return self._binary(t, "sub", reflected=True)

    def __rmul__(self, t):
        return self._binary(t, "mul", reflected=True)

    def __rtruediv__(self, t):
        return self._binary(t, "div", reflected=True)

    def __rpow__(self, t):
        return self._binary(t, "power", reflected=True)

    def __neg__(self):
        from .tensor_ops import neg
        return neg(self)

    def __pos__(self):
        from .tensor_ops import pos
        return pos(self)

    def matmul(self, t) -> "Tensor":
        from .tensor_ops import matmul
        return matmul(self, t)

    __matmul__ = matmul

    def __rmatmul__(self, t):
        from .tensor_ops import matmul
        return matmul(Tensor(np.asarray(t, dtype=np.float32), requires_grad=False, device=self.device), self)

    __array_priority__ = 100
    __array_ufunc__ = None          # a NumPy scalar or array on the left defers to the reflected operators

    # ---- reductions (autograd.py:233-311, 490-531): axis None, an int or a tuple, negative axes, keepdims ------------------------
    def _reduce(self, op, args, kwargs):
        from .tensor_ops import reduce
        axis = kwargs.pop("axis", None) if not args else args[0]
        keepdims = kwargs.pop("keepdims", False) if len(args) < 2 else args[1]
        if kwargs or len(args) > 2:
            raise TypeError(f"Tensor.{op}: unsupported arguments {sorted(kwargs)}")
        return reduce(self, op, axis, keepdims)

    def sum(self, *args, **kwargs) -> "Tensor":
        return self._reduce("sum", args, kwargs)

    def mean(self, *args, **kwargs) -> "Tensor":
        return self._reduce("mean", args, kwargs)

    def var(self, *args, **kwargs) -> "Tensor":
        """Population variance (ddof 0); the backward reuses the mean the forward computed."""
        return self._reduce("var", args, kwargs)

    def max(self, axis=None, keepdims=False) -> "Tensor":
        """np.max: a NaN propagates; the backward is grad * (x == max) from the saved output, every tie receives the gradient."""
        return self._reduce("max", (axis, keepdims), {})

    def min(self, axis=None, keepdims=False) -> "Tensor":
        return self._reduce("min", (axis, keepdims), {})

    # ---- layout (autograd.py:605-640): contiguous results, the backward is the inverse permutation ---------------------------------
    def transpose(self, *axes) -> "Tensor":
        from .tensor_ops import transpose
        axes = axes[0] if len(axes) == 1 and not isinstance(axes[0], (int, np.integer)) else axes
        return transpose(self, tuple(axes) if axes is not None else ())

    def swapaxes(self, axis1: int, axis2: int) -> "Tensor":
        from .tensor_ops import swapaxes
        return swapaxes(self, axis1, axis2)

    @property
    def T(self) -> "Tensor":
        return self.transpose()

    # ---- unary maps (autograd.py:339-440, 588-602) -----------------------------------------------------------------------------------
    def exp(self) -> "Tensor":
        from .tensor_ops import ACT_EXP, unary
        return unary(self, ACT_EXP, "exp")

    def sqrt(self) -> "Tensor":
        from .tensor_ops import ACT_SQRT, unary
        return unary(self, ACT_SQRT, "sqrt")

    def sin(self) -> "Tensor":
        from .tensor_ops import ACT_SIN, unary
        return unary(self, ACT_SIN, "sin")

    def cos(self) -> "Tensor":
        from .tensor_ops import ACT_COS, unary
        return unary(self, ACT_COS, "cos")

    def abs(self) -> "Tensor":
        from .tensor_ops import ACT_ABS, unary
        return unary(self, ACT_ABS, "abs")

    def tanh(self) -> "Tensor":
        from .tensor_ops import tanh
        return tanh(self)

    def log(self) -> "Tensor":
        """Natural logarithm on the tape (neunet/autograd.py:357): out = log(self), literally (log(0) = -inf, a negative entry gives
        NaN); the backward is grad / self.  Device float32 only: one nnhipActivationForward launch (kind NNHIP_ACT_LOG)."""
        from .nn.experimental.activations import ACT_LOG, hip_activation
        return hip_activation(self, ACT_LOG, "log")

    # ---- comparisons and logical ops (autograd.py:686-808): bool tensors off the tape --------------------------------------------------
    # An operand that is neither a Tensor, a number nor an array-like gives NotImplemented, so `t == None` is False and `t in [None]`
    # works.  There is no __bool__, as in the reference: compare tensors by identity (`is`) in host code.
    def _compare(self, t, op):
        from .tensor_index import compare
        return compare(self, t, op)

    def _logical(self, t, op):
        from .tensor_index import logical
        return logical(self, t, op)

    def equal(self, t) -> "Tensor":
        return self._compare(t, "equal")

    def not_equal(self, t) -> "Tensor":
        return self._compare(t, "not_equal")

    def greater(self, t) -> "Tensor":
        return self._compare(t, "greater")

    def greater_equal(self, t) -> "Tensor":
        return self._compare(t, "greater_equal")

    def less(self, t) -> "Tensor":
        return self._compare(t, "less")

    def less_equal(self, t) -> "Tensor":
        return self._compare(t, "less_equal")

    def logical_and(self, t) -> "Tensor":
        return self._logical(t, "logical_and")

    def logical_or(self, t) -> "Tensor":
        return self._logical(t, "logical_or")

    def logical_not(self) -> "Tensor":
        return self._logical(None, "logical_not")

    __eq__ = equal
    __ne__ = not_equal
    __gt__ = greater
    __ge__ = greater_equal
    __lt__ = less
    __le__ = less_equal
    __and__ = logical_and
    __or__ = logical_or
    __invert__ = logical_not
    __hash__ = object.__hash__      # defining __eq__ would otherwise make Tensors unhashable (parameter sets, tape bookkeeping)

    # ---- where, flip, indexing (autograd.py:642-684, 895-923) --------------------------------------------------------------------------
    def where(self, condition, t) -> "Tensor":
        """np.where(condition, self, t): float32 out; the backward is a select (dSelf = condition ? g : 0), summed over broadcast axes."""
        from .tensor_index import where
        return where(condition, self, t)

    def flip(self, axis=None) -> "Tensor":
        from .tensor_index import flip
        return flip(self, axis)

    def __getitem__(self, index) -> "Tensor":
        """A contiguous copy (basic keys; integer arrays on adjacent axes).  The backward ASSIGNS into zeros as the reference does:
        for repeated indices the last occurrence in C order wins."""
        from .tensor_index import getitem
        return getitem(self, index)

    def __setitem__(self, key, value):
        from .tensor_index import setitem
        setitem(self, key, value)

    def contiguous(self) -> "Tensor":
        return self

    def __abs__(self) -> "Tensor":
        return self.abs()

    def __repr__(self):
        return f"Tensor(shape={self.shape}, dtype={self.dtype}, device={self.device}, op={self.op})"
