"""neunet_hip.nn.utils -- gradient clipping by global norm for callers that do not use one of the optimizers of neunet_hip.optim
(those clip inside step(): `opt.max_grad_norm`) or that want to look at the clipped gradients.  An extension: the reference has no
gradient clipping.  torch.nn.utils.clip_grad_norm_'s arithmetic on the kernels of csrc/grad_norm.hip: one launch for the norm of all
gradients, one for the in-place scale, nothing read back."""
import ctypes
from ctypes import c_int64, c_void_p

from .._lib import call_hip_function, get_current_stream_ptr, load_hip_function
from ..optim import check_max_norm, norm_type_id

_handle = {"ptr": None}


def _opt_handle():
    """One library handle for the module: it owns the plan cache and the partials buffer of the launches below."""
    if _handle["ptr"] is None:
        ptr = load_hip_function("nnhipCreateFusedOptimizer")()
        if not ptr:
            raise RuntimeError("nnhipCreateFusedOptimizer failed")
        _handle["ptr"] = ptr
    return _handle["ptr"]


def _gradients(parameters):
    """[(parameter, contiguous float32 device gradient, strided original or None)] of the parameters that have a gradient."""
    import torch
    if hasattr(parameters, "data") and not isinstance(parameters, (list, tuple)):
        parameters = [parameters]
    out = []
    for p in parameters:
        if getattr(p, "device", "cuda") != "cuda":
            raise NotImplementedError("neunet_hip.nn.utils: parameters on the HIP device ('cuda') only; there is no CPU path")
        g = p.grad
        if g is None:
            continue
        if not isinstance(g, torch.Tensor) or not g.is_cuda:
            raise NotImplementedError("neunet_hip.nn.utils: gradients on the HIP device only; there is no CPU path")
        if g.dtype != torch.float32:
            raise ValueError(f"neunet_hip.nn.utils: float32 gradients only, got {g.dtype}")
        out.append((p, g, None) if g.is_contiguous() else (p, g.contiguous(), g))
    return out


def _tables(grads):
    n = len(grads)
    ptrs, sizes = (c_void_p * max(1, n))(), (c_int64 * max(1, n))()
    for i, (_, g, _) in enumerate(grads):
        ptrs[i], sizes[i] = g.data_ptr(), g.numel()
    return ctypes.cast(ptrs, ctypes.POINTER(c_void_p)), ctypes.cast(sizes, ctypes.POINTER(c_int64)), (ptrs, sizes)


def _norm_words(grads, max_norm, norm_type):
    import torch
    words = torch.zeros(4, dtype=torch.float32, device="cuda")
    ptrs, sizes, keep = _tables(grads)
    call_hip_function("nnhipGradNormMultiTensor", _opt_handle(), len(grads), ptrs, sizes, norm_type_id(norm_type), max_norm, None, 1,
                      1.0, words, get_current_stream_ptr())
    return words, ptrs, sizes, keep


def get_grad_norm(parameters, norm_type=2.0):
    """The global norm (2.0 or float('inf')) of the parameters' gradients as a 1-element device tensor: the norm launch alone.
    Parameters without a gradient are skipped; no gradients at all give 0."""
    norm_type_id(norm_type)
    words, _, _, _ = _norm_words(_gradients(parameters), 1.0, norm_type)
    return words[0:1]


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_: scale the gradients in place by min(1, max_norm / (norm + 1e-6)); returns the norm BEFORE
    clipping as a 1-element device tensor (reading it is the caller's synchronisation).  Parameters without a gradient are skipped;
    a strided gradient is copied to contiguous memory, scaled there and written back."""
    max_norm = check_max_norm(max_norm)
    norm_type_id(norm_type)
    grads = _gradients(parameters)
    words, ptrs, sizes, keep = _norm_words(grads, max_norm, norm_type)
    call_hip_function("nnhipScaleMultiTensor", _opt_handle(), len(grads), ptrs, sizes, words[1:2], get_current_stream_ptr())
    for _, g, strided in grads:
        if strided is not None:
            strided.copy_(g)
    return words[0:1]
