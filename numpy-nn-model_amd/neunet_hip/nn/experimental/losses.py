"""HIPCrossEntropyLoss -- drop-in for CUDACrossEntropyLoss
(neunet/nn/experimental/losses/cross_entropy_loss/cross_entropy.py:35-150).

One kernel computes per-row loss, log-sum-exp AND d(logits).  Differences from the reference's GPU
path, all on the side of the CPU semantics (neunet/nn/losses.py:59-126):
  * out-of-place by default: `logits` survive the forward (the reference kernel overwrites them,
    cross_entropy.py:69,94); `inplace=True` restores the reference's memory behaviour;
  * ignored rows are excluded from the 'mean' denominator on the DEVICE (nnhipCountNotEqual), so the
    forward never synchronises the host (the reference calls `.item()`, cross_entropy.py:72);
  * the 'mean' / 'sum' reduction also runs on the device (nnhipReduceLoss).

Also HIPBCELoss, HIPNLLLoss, HIPL1Loss and HIPKLDivLoss (neunet/nn/losses.py:25-56, 83-178): the CPU reference's constructors, loss and
gradient from one launch each.
"""
import weakref
from ...autograd import Tensor
from ..modules import Module
from .utils import call_hip_function, contiguous, get_current_stream_ptr, require_device_f32, times_upstream

_RED = {"none": b"n", "mean": b"m", "sum": b"s"}


def cross_entropy_forward_backward(logits, labels, reduction: str = "none", ignore_index: int = -100,
                                   inplace: bool = False, weight=None):
    """cross_entropy.py:35-103.  logits (rows, C) f32 device array, labels (rows,) int16/int32/int64 device array
    (the reference's CUDA path takes int32 only, cross_entropy.py:57; its CPU path all three, losses.py:100),
    weight: optional (C,) f32 device array of class weights (losses.py:93-118).
    Returns (loss, grad_logits): loss is a 0-d device array for 'mean'/'sum', (rows,) for 'none'.
    One launch whatever the reduction (nnhipCrossEntropyLossEx)."""
    import torch
    if logits.ndim != 2:
        raise ValueError("Logits must be 2D tensor")
    if labels.ndim != 1:
        raise ValueError("Labels must be 1D tensor")
    if labels.shape[0] != logits.shape[0]:
        raise ValueError("Logits and labels must have the same number of samples")
    if labels.dtype not in _LABEL_BYTES():
        raise TypeError("Labels must be of int16, int32 or int64 dtype")
    if logits.dtype != torch.float32:
        raise TypeError("Logits must be of float32 dtype")
    if reduction not in _RED:
        raise ValueError("Reduction must be 'none', 'mean', or 'sum'")
    rows, vocab = logits.shape
    if weight is not None:
        if tuple(weight.shape) != (vocab,):
            raise ValueError("Weight shape must be equal to number of classes")
        if weight.dtype != torch.float32:
            raise TypeError("Weight must be of float32 dtype")
        weight = contiguous(weight)
    logits, labels = contiguous(logits), contiguous(labels)
    loss_rows = torch.empty(rows, dtype=torch.float32, device=logits.device)
    lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    grad_logits = logits if inplace else torch.empty_like(logits)
    loss = count = None
    if reduction != "none":
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        count = torch.empty(1, dtype=torch.int32, device=logits.device) if reduction == "mean" else None
    call_hip_function("nnhipCrossEntropyLossEx", logits, None if inplace else grad_logits, loss_rows, lse, labels,
                      _LABEL_BYTES()[labels.dtype], weight, logits.stride(0), int(ignore_index), rows, vocab,
                      _RED[reduction], loss, count, get_current_stream_ptr())
    return (loss_rows if reduction == "none" else loss), grad_logits


def _LABEL_BYTES():
    import torch
    return {torch.int16: 2, torch.int32: 4, torch.int64: 8}


def _fused_linear_cross_entropy(y_pred, labels, reduction, ignore_index, weight):
    """If y_pred is the still-pending output of a small HIPLinear (a classifier head: <= 256 rows, <= 32 classes), run the
    GEMM and the loss as ONE launch (nnhipLinearCrossEntropyLoss) and hand the logits to the Linear's tensor.  Returns
    (loss, grad_logits) or None when the ordinary two-launch path has to run."""
    import torch
    ops = getattr(y_pred, "_operands", None)
    if ops is None or not getattr(y_pred, "pending", lambda: False)() or len(y_pred.shape) != 2:
        return None
    rows, classes = y_pred.shape
    xdata, w, b = ops
    in_features = w.shape[1]
    if not (1 <= rows <= 256 and 1 <= classes <= 32 and 1 <= in_features <= 2048):
        return None
    if labels.ndim != 1 or labels.shape[0] != rows or labels.dtype not in _LABEL_BYTES() or reduction not in _RED:
        return None                                    # let the ordinary path raise its errors
    if weight is not None and (tuple(weight.shape) != (classes,) or weight.dtype != torch.float32):
        return None
    labels = contiguous(labels)
    dev = xdata.device
    logits = torch.empty((rows, classes), dtype=torch.float32, device=dev)
    grad_logits = torch.empty_like(logits)
    loss_rows = torch.empty(rows, dtype=torch.float32, device=dev)
    lse = torch.empty(rows, dtype=torch.float32, device=dev)
    loss = count = None
    if reduction != "none":
        loss = torch.empty((), dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev) if reduction == "mean" else None
    call_hip_function("nnhipLinearCrossEntropyLoss", xdata, w, b, logits, grad_logits, loss_rows, lse, labels,
                      _LABEL_BYTES()[labels.dtype], None if weight is None else contiguous(weight), int(ignore_index), rows,
                      in_features, classes, _RED[reduction], loss, count, get_current_stream_ptr())
    y_pred.adopt(logits)
    return (loss_rows if reduction == "none" else loss), grad_logits


class _HIPCrossEntropyTensor(Tensor):
    _implicit_seed = True      # backward() with no argument needs no ones tensor: grad_fn below handles the unit seed

    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)
        out_ref = weakref.ref(self)   # no tensor -> grad_fn -> closure -> tensor cycle: activations die by refcount

        def grad_fn(y_pred: Tensor, grad_y_pred, grad):
            # cross_entropy.py:111-114: y_pred.apply_grad(grad_y_pred * grad).  When backward() was
            # seeded with ones on this very tensor the product is the identity: skip a full pass.
            if getattr(out_ref(), "_seeded_with_ones", False):
                y_pred.apply_grad(grad_y_pred)
                return
            if getattr(grad, "ndim", 0) == 1 and grad.shape[0] != 1:
                grad = grad[:, None]            # cross_entropy.py:112-113: a 1-D upstream gradient is one value per ROW
            y_pred.apply_grad(times_upstream(grad_y_pred, grad))

        self.grad_fn = grad_fn


class HIPCrossEntropyLoss(Module):
    def __init__(self, reduction="none", ignore_index=-100, inplace=False, weight=None):
        """weight (extension over CUDACrossEntropyLoss; neunet.nn.CrossEntropyLoss has it, losses.py:60-64): per-class
        weights as a Tensor / array of shape (C,)."""
        super().__init__()
        self.reduction = reduction
        self.ignore_index = ignore_index
        self.inplace = inplace
        self.weight = None
        if weight is not None:
            import numpy as np
            w = weight.data if isinstance(weight, Tensor) else weight
            self.weight = Tensor(w, dtype=np.float32, requires_grad=False, device="cuda").data

    def forward(self, y_pred: Tensor, y_true: Tensor) -> Tensor:
        if not isinstance(y_pred, Tensor) or not isinstance(y_true, Tensor):
            raise TypeError("Input values must be tensors")
        if y_pred.device != "cuda" or y_true.device != "cuda":
            raise ValueError("Tensors must be on the cuda (HIP) device")
        if y_pred.dtype != "float32":
            raise TypeError("Predictions must be of float32 dtype")
        if y_true.dtype not in ("int16", "int32", "int64"):
            raise TypeError("Target must be of int dtype")
        fused = None if self.inplace else _fused_linear_cross_entropy(y_pred, y_true.data, self.reduction, self.ignore_index,
                                                                     self.weight)
        if fused is not None:
            loss, grad_y_pred = fused
        else:
            loss, grad_y_pred = cross_entropy_forward_backward(y_pred.data, y_true.data, reduction=self.reduction,
                                                               ignore_index=self.ignore_index, inplace=self.inplace,
                                                               weight=self.weight)
        return _HIPCrossEntropyTensor(loss, (y_pred, grad_y_pred), "cross_entropy", device="cuda")


CUDACrossEntropyLoss = HIPCrossEntropyLoss


# ------------------------------------------------------------------------------------------------- BCELoss
class _HIPBCETensor(Tensor):
    _implicit_seed = True      # backward() with no argument needs no ones tensor: grad_fn below handles the unit seed

    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)
        out_ref = weakref.ref(self)

        def grad_fn(y_pred: Tensor, grad_pred, grad):
            if getattr(out_ref(), "_seeded_with_ones", False):
                y_pred.apply_grad(grad_pred)
            else:
                y_pred.apply_grad(times_upstream(grad_pred, grad))

        self.grad_fn = grad_fn


class HIPBCELoss(Module):
    """neunet/nn/losses.py:25-56, same constructor: -(y log p + (1 - y) log(1 - p)) * weight, reduced by 'mean', 'sum' or not at all
    ('none'); the reference's expression literally, NO clamp (p = 0 or 1 gives inf / NaN as np.log does).  weight: None, a scalar, or an
    array / Tensor of the prediction's shape -- anything else raises ValueError (the reference accepts whatever broadcasts to the
    prediction's shape, :41-44; the HIP path takes the two cases the kernel reads without a broadcast).  Loss and d(pred) come from one
    pass (nnhipBCELossForwardBackward); the reduced loss is a 0-d tensor.

    BCELoss(Sigmoid(z)): when the prediction is a Sigmoid's output (and NNHIP_VISION_FUSION is on) the kernel hands
    dz = (p - y) * weight * scale straight to the Sigmoid's input, as HIPMSELoss does -- one launch less, and finite where a saturated
    p would make the unfolded gradient 0 * inf.  The loss value is the literal expression on p either way."""

    def __init__(self, weight=None, reduction="mean"):
        super().__init__()
        if reduction not in _RED:
            raise ValueError("Reduction must be 'none', 'mean', or 'sum'")
        self.weight = weight
        self.reduction = reduction
        self._weight_dev = None

    def _weight_kind(self, shape):
        """('scalar', value) or ('array', the weight as given): None, a scalar or a one-element array is a scalar; an array of the
        prediction's shape is an array; anything else raises."""
        import numpy as np
        w = self.weight
        if w is None:
            return "scalar", 1.0
        w = w.data if isinstance(w, Tensor) else w
        if isinstance(w, (int, float, np.floating, np.integer)):
            return "scalar", float(w)
        if isinstance(w, (list, tuple)):
            w = np.asarray(w, dtype=np.float32)
        wshape = getattr(w, "shape", None)
        if wshape is None:
            raise ValueError("BCELoss weight must be None, a scalar, or an array of the prediction's shape")
        if tuple(wshape) == tuple(shape):
            return "array", w
        if int(np.prod(tuple(wshape), dtype=np.int64)) == 1:
            return "scalar", float(w.reshape(-1)[0])
        raise ValueError("BCELoss weight must be None, a scalar, or an array of the prediction's shape")

    def _weight_args(self, kind, w, like):
        """(device array or None, scalar) for the kernel; the device copy of an array weight is made once."""
        import numpy as np
        import torch
        if kind == "scalar":
            return None, w
        if self._weight_dev is None or self._weight_dev[0] is not self.weight:
            dev = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float32)))
            self._weight_dev = (self.weight, contiguous(dev.to(device=like.device, dtype=torch.float32)))
        return self._weight_dev[1], 1.0

    def forward(self, y_pred: Tensor, y_true: Tensor) -> Tensor:
        import torch
        from .vision import _FUSE, _HIPSigmoidTensor
        if not isinstance(y_pred, Tensor) or not isinstance(y_true, Tensor):
            raise TypeError("Input values must be tensors")
        if y_pred.device != y_true.device:
            raise ValueError("Tensors must be on the same device")
        if y_pred.shape != y_true.shape:
            raise ValueError("BCELoss on the HIP path needs equal shapes")
        kind, w = self._weight_kind(y_pred.shape)
        require_device_f32(y_pred, y_true)
        p, t = contiguous(y_pred.data), contiguous(y_true.data)
        w_arr, w_scalar = self._weight_args(kind, w, p)
        none = self.reduction == "none"
        loss = torch.empty(p.shape if none else (), dtype=torch.float32, device=p.device)
        dpred = torch.empty_like(p)
        fold = isinstance(y_pred, _HIPSigmoidTensor) and _FUSE
        call_hip_function("nnhipBCELossForwardBackward", p, t, w_arr, w_scalar, loss, dpred, p.numel(), _RED[self.reduction],
                          int(fold), get_current_stream_ptr())
        # fold: d(loss)/dz goes to the Sigmoid's input; the Sigmoid node drops out of this loss's backward
        return _HIPBCETensor(loss, (y_pred.args[0] if fold else y_pred, dpred), "bce", device="cuda")


# ------------------------------------------------------------------------------------------------- NLLLoss
class _HIPNLLTensor(Tensor):
    """args = (y_pred, dlogp): the dense route -- the kernel's gradient with respect to the log-probabilities."""
    _implicit_seed = True      # backward() with no argument needs no ones tensor: grad_fn below handles the unit seed

    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)
        out_ref = weakref.ref(self)

        def grad_fn(y_pred: Tensor, dlogp, grad):
            if getattr(out_ref(), "_seeded_with_ones", False):
                y_pred.apply_grad(dlogp)
                return
            if getattr(grad, "ndim", 0) >= 1 and grad.numel() != 1:
                # reduction 'none': one upstream value per position -- (N, 1) or the labels' shape -- against dlogp [N, C, d...]
                grad = grad.reshape((dlogp.shape[0], 1) + tuple(dlogp.shape[2:]))
            y_pred.apply_grad(times_upstream(dlogp, grad))

        self.grad_fn = grad_fn


class _HIPNLLFoldTensor(Tensor):
    """args = (x, log_probs, labels, pos_grad): NLLLoss(LogSoftmax(x)) -- the node hangs on the LogSoftmax's INPUT and its backward is one
    pass over the log-probabilities (nnhipLogSoftmaxNLLBackward); the dense [N, C] gradient of the NLL never exists."""
    _implicit_seed = True

    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)
        out_ref = weakref.ref(self)

        def grad_fn(x: Tensor, log_probs, labels, pos_grad, grad):
            import torch
            upstream = None
            if not getattr(out_ref(), "_seeded_with_ones", False):
                g = grad if isinstance(grad, torch.Tensor) else torch.as_tensor(grad, dtype=torch.float32, device=log_probs.device)
                upstream = g.to(torch.float32).reshape(1).contiguous()
            dx = torch.empty_like(log_probs)
            rows, classes = log_probs.shape
            call_hip_function("nnhipLogSoftmaxNLLBackward", dx, log_probs, labels, _LABEL_BYTES()[labels.dtype], pos_grad, upstream,
                              rows, classes, get_current_stream_ptr())
            x.apply_grad(dx)

        self.grad_fn = grad_fn


class HIPNLLLoss(Module):
    """neunet/nn/losses.py:83-126, same constructor.  y_pred: log-probabilities (N, C) or (N, C, d1, ...), y_true: int16 / int32 / int64
    class indices (N,) or (N, d1, ...).  loss = -y_pred[n, y, ...] * weight[y] per position, reduced by 'mean' (over the summed
    weights of the counted positions), 'sum' or not at all ('none': shape (N, 1) for 2-D predictions with 1-D labels, the labels'
    shape otherwise, as the reference returns).  Loss and gradient come from one launch (nnhipNLLLossForwardBackward); reduced losses
    are 0-d.

    Differences from the reference, on the side of nnhipCrossEntropyLossEx: a position whose label equals ignore_index is never
    dereferenced (the reference indexes weight[y] before masking: its default ignore_index = -100 raises IndexError below 100
    classes); a label outside [0, C) counts as nothing; a zero 'mean' denominator gives loss 0 and a zero gradient (reference: NaN).

    NLLLoss(LogSoftmax(x)) with 2-D x, axis 1 and a reduced loss -- the reference's own CrossEntropyLoss, losses.py:66-77 -- folds the
    two backward passes into one: the loss node hangs on x and nnhipLogSoftmaxNLLBackward writes dx from the log-probabilities and one
    value per row.  Same loss bits as the dense route."""

    def __init__(self, weight=None, ignore_index=-100, reduction="mean"):
        super().__init__()
        if reduction not in _RED:
            raise ValueError("Reduction must be 'none', 'mean', or 'sum'")
        self.reduction = reduction
        self.ignore_index = ignore_index
        self.weight = None
        if weight is not None:
            import numpy as np
            w = weight.data if isinstance(weight, Tensor) else weight
            if hasattr(w, "detach"):
                w = w.detach().cpu().numpy()
            self.weight = np.ascontiguousarray(np.asarray(w, dtype=np.float32))
        self._weight_dev = None

    def _device_weight(self, like):
        import torch
        if self.weight is None:
            return None
        if self._weight_dev is None or self._weight_dev.device != like.device:
            self._weight_dev = torch.from_numpy(self.weight).to(like.device)
        return self._weight_dev

    def forward(self, y_pred: Tensor, y_true: Tensor) -> Tensor:
        import torch
        from .activations import _HIPLogSoftmaxTensor
        if not isinstance(y_pred, Tensor) or not isinstance(y_true, Tensor):
            raise TypeError("Input values must be tensors")
        if y_pred.ndim < 2:
            raise ValueError("Predictions must be (N, C) or (N, C, d1, ...)")
        classes = y_pred.shape[1]
        if self.weight is not None and tuple(self.weight.shape) != (classes,):      # losses.py:98-101, in the reference's order
            raise ValueError("Weight shape must be equal to number of classes")
        if y_true.dtype not in ("int16", "int32", "int64"):
            raise TypeError("Target must be of int dtype")
        if y_pred.device != "cuda" or y_true.device != "cuda":
            raise ValueError("Tensors must be on the cuda (HIP) device")
        if y_pred.dtype != "float32":
            raise TypeError("Predictions must be of float32 dtype")
        pshape, lshape = tuple(y_pred.shape), tuple(y_true.shape)
        if lshape != (pshape[0],) + pshape[2:]:
            raise ValueError(f"Target of shape {lshape} does not match predictions of shape {pshape}")
        logp, labels = contiguous(y_pred.data), contiguous(y_true.data)
        outer, inner = pshape[0], 1
        for d in pshape[2:]:
            inner *= d
        none = self.reduction == "none"
        fold = (not none and isinstance(y_pred, _HIPLogSoftmaxTensor) and len(pshape) == 2 and y_pred.args[2] % 2 == 1
                and y_pred.args[0].requires_grad)
        loss = torch.empty(((lshape[0], 1) if len(lshape) == 1 else lshape) if none else (), dtype=torch.float32, device=logp.device)
        dlogp = None if fold else torch.empty_like(logp)
        pos_grad = torch.empty(outer, dtype=torch.float32, device=logp.device) if fold else None
        call_hip_function("nnhipNLLLossForwardBackward", logp, labels, _LABEL_BYTES()[labels.dtype], self._device_weight(logp),
                          int(self.ignore_index), outer, classes, inner, _RED[self.reduction], loss, dlogp, pos_grad,
                          get_current_stream_ptr())
        if fold:
            # d(loss)/dx goes to the LogSoftmax's input; the LogSoftmax node drops out of this loss's backward
            return _HIPNLLFoldTensor(loss, (y_pred.args[0], logp, labels, pos_grad), "nll_log_softmax", device="cuda")
        return _HIPNLLTensor(loss, (y_pred, dlogp), "nll", device="cuda")


# ------------------------------------------------------------------------------------------------- L1Loss, KLDivLoss
_RED_KL = dict(_RED, batchmean=b"b")


class HIPL1Loss(Module):
    """neunet/nn/losses.py:129-146, same constructor: |y_pred - y_true| reduced by 'mean', 'sum' or not at all ('none'); the gradient is
    sign(y_pred - y_true) * scale with sign(0) = 0.  Loss and d(pred) come from one pass (nnhipL1LossForwardBackward); y_true receives
    no gradient."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction not in _RED:
            raise ValueError("Reduction must be 'none', 'mean', or 'sum'")
        self.reduction = reduction

    def forward(self, y_pred: Tensor, y_true: Tensor) -> Tensor:
        import torch
        if not isinstance(y_pred, Tensor) or not isinstance(y_true, Tensor):
            raise TypeError("Input values must be tensors")
        if y_pred.device != y_true.device:
            raise ValueError("Tensors must be on the same device")
        if y_pred.shape != y_true.shape:
            raise ValueError("L1Loss on the HIP path needs equal shapes")
        require_device_f32(y_pred, y_true)
        p, t = contiguous(y_pred.data), contiguous(y_true.data)
        none = self.reduction == "none"
        loss = torch.empty(p.shape if none else (), dtype=torch.float32, device=p.device)
        dpred = torch.empty_like(p)
        call_hip_function("nnhipL1LossForwardBackward", p, t, loss, dpred, p.numel(), _RED[self.reduction], get_current_stream_ptr())
        return _HIPBCETensor(loss, (y_pred, dpred), "l1", device="cuda")


class HIPKLDivLoss(Module):
    """neunet/nn/losses.py:152-175, same constructor: y_true * (log(y_true) - y_pred), or with log_target exp(y_true) * (y_true - y_pred)
    -- the reference's expression literally (a zero target gives NaN as np.log does) -- reduced by 'mean', 'batchmean' (sum / N),
    'sum' or not at all ('none').  Loss and d(pred) come from one pass (nnhipKLDivLossForwardBackward); y_true receives no gradient."""

    def __init__(self, reduction="mean", log_target=False):
        super().__init__()
        if reduction not in _RED_KL:
            raise ValueError("Reduction must be 'none', 'mean', 'batchmean', or 'sum'")
        self.reduction = reduction
        self.log_target = log_target

    def forward(self, y_pred: Tensor, y_true: Tensor) -> Tensor:
        import torch
        if not isinstance(y_pred, Tensor) or not isinstance(y_true, Tensor):
            raise TypeError("Input values must be tensors")
        if y_pred.device != y_true.device:
            raise ValueError("Tensors must be on the same device")
        if y_pred.shape != y_true.shape:
            raise ValueError("KLDivLoss on the HIP path needs equal shapes")
        require_device_f32(y_pred, y_true)
        p, t = contiguous(y_pred.data), contiguous(y_true.data)
        none = self.reduction == "none"
        loss = torch.empty(p.shape if none else (), dtype=torch.float32, device=p.device)
        dpred = torch.empty_like(p)
        call_hip_function("nnhipKLDivLossForwardBackward", p, t, loss, dpred, p.numel(), p.shape[0] if p.ndim else 1,
                          int(bool(self.log_target)), _RED_KL[self.reduction], get_current_stream_ptr())
        return _HIPBCETensor(loss, (y_pred, dpred), "kldiv", device="cuda")
