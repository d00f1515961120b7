"""neunet_hip -- MI355X (gfx950) backend for the dense hot path of AkiRusProd/numpy-nn-model (`neunet`).

Host side: the reference's Module / Tensor / tape shape (neunet/autograd.py, neunet/nn/modules.py);
device side: hand-written HIP kernels in libneunet_hip.so behind a flat C ABI (include/neunet_hip.h),
bound with ctypes exactly where the reference binds its CUDA .so files
(neunet/nn/experimental/utils.py:64-92).
"""
import numpy as np

from . import nn, optim  # noqa: F401
from ._lib import NeunetHipError, lib_path, load_library  # noqa: F401
from .autograd import Tensor  # noqa: F401

float32, int32, int64 = np.float32, np.int32, np.int64


def tensor(data, requires_grad=True, dtype=np.float32, device="cpu"):
    """neunet.tensor (neunet/__init__.py:40-47)."""
    return Tensor(data, requires_grad=requires_grad, dtype=dtype, device=device)


def _arg_extreme(x: Tensor, axis, keepdims, which):
    """argmax / argmin -> int32; `which`: 'argmax' | 'argmin' (np.<which>, torch.<which>, nnhipArgmaxF32 / nnhipArgminF32)."""
    if x.device == "cpu":
        out = getattr(np, which)(x.data, axis=axis, keepdims=keepdims).astype(np.int32)
        return Tensor(out, dtype=np.int32, requires_grad=False, device="cpu")
    import torch
    from ._lib import call_hip_function, get_current_stream_ptr
    d = x.data
    if d.dtype != torch.float32:
        # np.argmax takes labels / ids / masks too (neunet/__init__.py:132-139).  The library's kernel compares fp32: integer types
        # whose EVERY value is exact in fp32 (|v| < 2^24: bool, uint8, int16) ride on it; wider integers and float64 keep torch's
        # argmax -- same first-maximum rule.  Decided from the dtype alone: a range test on the data (round 5: `d.abs().max()`)
        # is a host read in the middle of a step and breaks hipGraph capture (advisor, round 5).
        if d.dtype in (torch.int16, torch.uint8, torch.bool):
            d = d.to(torch.float32)
        else:
            fn = getattr(torch, which)
            out = fn(d) if axis is None else fn(d, dim=axis, keepdim=keepdims)
            if axis is None and keepdims:
                out = out.reshape((1,) * d.dim())
            return Tensor(out.to(torch.int32), dtype=np.int32, requires_grad=False, device="cuda")
    d = d.contiguous()
    shape = tuple(d.shape)
    if axis is None:
        outer, n, inner, oshape = 1, d.numel(), 1, ((1,) * len(shape) if keepdims else ())
    else:
        ax = axis + len(shape) if axis < 0 else axis
        if not 0 <= ax < len(shape):
            raise ValueError(f"axis {axis} is out of bounds for array of dimension {len(shape)}")
        outer, n, inner = int(np.prod(shape[:ax], dtype=np.int64)), shape[ax], int(np.prod(shape[ax + 1:], dtype=np.int64))
        oshape = shape[:ax] + ((1,) if keepdims else ()) + shape[ax + 1:]
    if n == 0 and outer * inner > 0:
        raise ValueError(f"attempt to get {which} of an empty sequence")
    out = torch.empty(oshape, dtype=torch.int32, device=d.device)
    call_hip_function("nnhipArgmaxF32" if which == "argmax" else "nnhipArgminF32", out, d, outer, n, inner, get_current_stream_ptr())
    return Tensor(out, dtype=np.int32, requires_grad=False, device="cuda")


def argmax(x: Tensor, axis=None, keepdims=False):
    """neunet.argmax -> int32 (neunet/__init__.py:132-139); index results must be bit-exact."""
    return _arg_extreme(x, axis, keepdims, "argmax")


def argmin(x: Tensor, axis=None, keepdims=False):
    """neunet.argmin -> int32 (neunet/__init__.py:142-149): the first minimum wins, a NaN wins (np.argmin); nnhipArgminF32."""
    return _arg_extreme(x, axis, keepdims, "argmin")


# ---- constructors (neunet/__init__.py:45-129, 283-287): the reference's signatures and defaults (requires_grad=False, float32, "cpu") ----
def _normalize_shape(shape):
    return tuple(*shape) if shape and all(isinstance(a, (list, tuple)) for a in shape) else tuple(shape)


def _filled(data, dtype, requires_grad, device):
    return Tensor(data, requires_grad=requires_grad, dtype=dtype, device="cpu" if device is None else device)


def ones(*shape, dtype=None, requires_grad=False, device=None):
    dtype = np.float32 if dtype is None else dtype
    return _filled(np.ones(_normalize_shape(shape), dtype=dtype), dtype, requires_grad, device)


def zeros(*shape, dtype=None, requires_grad=False, device=None):
    dtype = np.float32 if dtype is None else dtype
    return _filled(np.zeros(_normalize_shape(shape), dtype=dtype), dtype, requires_grad, device)


def rand(*shape, dtype=None, requires_grad=False, device=None):
    """Uniform [0, 1) from np.random on the host (the reference's CPU path), then moved."""
    dtype = np.float32 if dtype is None else dtype
    return _filled(np.random.rand(*_normalize_shape(shape)).astype(dtype), dtype, requires_grad, device)


def randn(*shape, dtype=None, requires_grad=False, device=None):
    dtype = np.float32 if dtype is None else dtype
    return _filled(np.random.randn(*_normalize_shape(shape)).astype(dtype), dtype, requires_grad, device)


def arange(start=0, end=None, step=1, dtype=None, requires_grad=False, device=None):
    if end is None:
        start, end = 0, start
    dtype = np.float32 if dtype is None else dtype
    return _filled(np.arange(start, end, step, dtype=dtype), dtype, requires_grad, device)


def ones_like(tensor, dtype=None, requires_grad=False, device=None):       # noqa: A002  (the reference's argument name)
    dtype = tensor.dtype if dtype is None else dtype
    return _filled(np.ones(tensor.shape, dtype=dtype), dtype, requires_grad, tensor.device if device is None else device)


def zeros_like(tensor, dtype=None, requires_grad=False, device=None):      # noqa: A002
    dtype = tensor.dtype if dtype is None else dtype
    return _filled(np.zeros(tensor.shape, dtype=dtype), dtype, requires_grad, tensor.device if device is None else device)


def copy(x: Tensor) -> Tensor:
    """A new leaf with a copy of the data (Tensor.__init__ copies)."""
    return Tensor(x.data, requires_grad=x.requires_grad, dtype=x.dtype, device=x.device)


def clone(x: Tensor) -> Tensor:
    return copy(x)


SAMPLE_MAX_K = 1024      # NNHIP_SAMPLE_MAX_K (include/neunet_hip.h)


def sample_top_k(logits, top_k, temperature=1.0, seed=0, seed_dev=None, out=None, return_u=False):
    """Draw one id per row of `logits` [..., n] on the device (nnhipSampleTopK): temperature, top-k and the multinomial draw of the
    reference's GPT-2 script (examples/gpt2/gpt2_infer.py:331-338) without a host copy of the logits.  logits: a device Tensor or
    torch tensor, float32, unit stride along the last axis; the leading axes may sit in a wider buffer (one row stride, passed as
    ld).  The row's uniform is a hash of (seed + *seed_dev, row): seed_dev is an optional device int32 / uint32 word (its first
    element is read inside the kernel, so a captured hipGraph draws afresh on every replay).  Returns the int32 ids (a device
    torch tensor of shape logits.shape[:-1], or `out`, which only needs that many int32 elements); with return_u also the float32
    uniforms each row used.  top_k < 1 is a ValueError: greedy decoding is argmax."""
    top_k = int(top_k)
    if top_k < 1:
        raise ValueError(f"sample_top_k needs top_k >= 1 (got {top_k}); greedy decoding is neunet_hip.argmax")
    if top_k > SAMPLE_MAX_K:
        raise ValueError(f"sample_top_k supports top_k <= {SAMPLE_MAX_K} (got {top_k})")
    temperature = float(temperature)
    if not temperature >= 0.0:
        raise ValueError(f"sample_top_k needs a temperature >= 0 (got {temperature})")
    import torch
    from ._lib import StridedView, call_hip_function, get_current_stream_ptr
    d = logits.data if isinstance(logits, Tensor) else logits
    if not isinstance(d, torch.Tensor) or not d.is_cuda or d.dtype != torch.float32:
        raise ValueError("sample_top_k needs float32 logits on the device")
    if d.dim() < 1 or d.shape[-1] < 1:
        raise ValueError("sample_top_k needs a last axis of at least one element")
    n, lead = d.shape[-1], tuple(d.shape[:-1])
    rows = int(np.prod(lead, dtype=np.int64))
    ld = n
    if not d.is_contiguous():
        # one row stride for all leading axes (e.g. logits[:, -1] of [B, T, n]); anything else would need a copy: refuse
        axes = [(d.shape[i], d.stride(i)) for i in range(d.dim() - 1) if d.shape[i] > 1]
        ld = axes[-1][1] if axes else n
        ok = d.stride(-1) == 1 and ld >= n
        for (_, s0), (n1, s1) in zip(axes[:-1], axes[1:]):
            ok = ok and s0 == s1 * n1
        if not ok:
            raise ValueError("sample_top_k needs unit stride along the last axis and one row stride >= n for the leading axes")
    if seed_dev is not None and not (isinstance(seed_dev, torch.Tensor) and seed_dev.is_cuda and seed_dev.numel() >= 1
                                     and seed_dev.dtype in (torch.int32, torch.uint32)):
        raise ValueError("seed_dev must be a device int32 / uint32 tensor")
    if out is None:
        out = torch.empty(lead, dtype=torch.int32, device=d.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int32 and out.numel() == rows and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous device int32 tensor of {rows} elements")
    u = torch.empty(lead, dtype=torch.float32, device=d.device) if return_u else None
    call_hip_function("nnhipSampleTopK", out, u, StridedView(d), rows, n, ld, top_k, temperature, int(seed) & 0xFFFFFFFF, seed_dev,
                      get_current_stream_ptr())
    return (out, u) if return_u else out


def set_linear_gemv(enable: bool) -> None:
    """The process-wide switch nnhipSetLinearGemv: while it is on, a Linear forward of 1..8 rows (nnhipLinearModuleForward[Ex], which
    is every nn.Linear / HIPLinear forward, `residual=` included) streams its weights through the GEMV kernel instead of the tiled
    GEMM.  Off by default: the kernel adds in another order, so results move in their last bits."""
    from ._lib import call_hip_function
    call_hip_function("nnhipSetLinearGemv", 1 if enable else 0)


def get_linear_gemv() -> bool:
    from ._lib import call_hip_function
    return bool(call_hip_function("nnhipGetLinearGemv"))


class linear_gemv:
    """`with neunet_hip.linear_gemv():` -- the switch of set_linear_gemv for the duration of a block; the value it had before comes
    back on exit, exceptions included."""

    def __init__(self, enable=True):
        self.enable = bool(enable)

    def __enter__(self):
        self.previous = get_linear_gemv()
        set_linear_gemv(self.enable)
        return self

    def __exit__(self, *exc):
        set_linear_gemv(self.previous)
        return False


class conv_transpose_route:
    """`with neunet_hip.conv_transpose_route("phase" | "gather" | "auto"):` -- how ConvTranspose2d forwards with a stride above 1
    run for the duration of a block (nnhipSetConvTransposeRoute; process-wide): the stride-phase kernel, the Conv2d
    input-gradient gather, or the library's own choice.  The previous route comes back on exit, exceptions included."""

    def __init__(self, route="auto"):
        from .nn.experimental.conv_transpose2d import ROUTES
        if route not in ROUTES:
            raise ValueError(f"route must be one of {sorted(ROUTES)} (got {route!r})")
        self.route = ROUTES[route]

    def __enter__(self):
        from ._lib import call_hip_function
        self.previous = call_hip_function("nnhipSetConvTransposeRoute", self.route)
        return self

    def __exit__(self, *exc):
        from ._lib import call_hip_function
        call_hip_function("nnhipSetConvTransposeRoute", self.previous)
        return False


def concatenate(*tensors, axis=1):
    """neunet.concatenate (neunet/__init__.py): the U-Net's skip connections.  Plumbing: the copy is torch.cat (np.concatenate on the
    host), the gradient is handed back as `narrow` views of the output's."""
    if not tensors or not all(isinstance(t, Tensor) for t in tensors):
        raise TypeError("concatenate takes Tensors")
    device = tensors[0].device
    if any(t.device != device for t in tensors):
        raise ValueError("Tensors must be on the same device")
    ax = axis + tensors[0].ndim if axis < 0 else axis
    sizes = [t.shape[ax] for t in tensors]
    if device == "cpu":
        data = np.concatenate([t.data for t in tensors], axis=ax)
    else:
        import torch
        data = torch.cat([t.data for t in tensors], dim=ax)
    rg = any(t.requires_grad for t in tensors)
    out = Tensor(data, tensors if rg else None, "concatenate", requires_grad=rg, device=device, _nocopy=True)

    def grad_fn(*args, grad):
        start = 0
        for t, n in zip(args, sizes):
            if t.requires_grad:
                if isinstance(grad, np.ndarray):
                    t.apply_grad(np.take(grad, range(start, start + n), axis=ax))
                else:
                    t.apply_grad(grad.narrow(ax, start, n).contiguous())
            start += n

    out.grad_fn = grad_fn
    return out


def add_channel_bias(h: Tensor, t: Tensor) -> Tensor:
    """h [B, C, H, W] + t [B, C][:, :, None, None] -- the U-Net's time embedding joining a feature map (the reference writes it as a
    broadcasting Tensor add, examples/ddpm.ipynb cell 5).  dh = grad, dt = grad summed over H and W.  Plumbing (a broadcast add
    and a sum); Tensor.add keeps refusing broadcasts."""
    if not isinstance(h, Tensor) or not isinstance(t, Tensor):
        raise TypeError("add_channel_bias takes Tensors")
    if h.device != t.device:
        raise ValueError("Tensors must be on the same device")
    if h.ndim != 4 or tuple(t.shape) != tuple(h.shape[:2]):
        raise ValueError(f"add_channel_bias needs h [B, C, H, W] and t [B, C] (got {h.shape} and {t.shape})")
    rg = h.requires_grad or t.requires_grad
    out = Tensor(h.data + t.data[:, :, None, None], (h, t) if rg else None, "add_channel_bias", requires_grad=rg, device=h.device,
                 _nocopy=True)

    def grad_fn(a, b, grad):
        if a.requires_grad:
            a.apply_grad(grad)
        if b.requires_grad:
            b.apply_grad(grad.sum(axis=(2, 3)) if isinstance(grad, np.ndarray) else grad.sum(dim=(2, 3)))

    out.grad_fn = grad_fn
    return out


def reparameterize(mu: Tensor, logvar: Tensor, eps: Tensor) -> Tensor:
    """z = mu + eps * exp(logvar / 2) -- VAE.reparameterize of the reference's examples/vae.ipynb (which writes it as
    logvar.mul(0.5).exp(), eps * std, mu + ...: three tape nodes) as ONE launch forward (nnhipGaussianReparamForward) and one backward:
    dmu = grad, dlogvar = grad * eps * 0.5 * std.  eps is a tensor the caller draws (the notebook draws it with the host NumPy RNG);
    it receives no gradient."""
    import torch
    from ._lib import call_hip_function, get_current_stream_ptr
    if not all(isinstance(t, Tensor) for t in (mu, logvar, eps)):
        raise TypeError("reparameterize takes Tensors")
    if not (mu.device == logvar.device == eps.device == "cuda"):
        raise ValueError("reparameterize needs its three tensors on the HIP device ('cuda')")
    if not (tuple(mu.shape) == tuple(logvar.shape) == tuple(eps.shape)):
        raise ValueError(f"reparameterize needs equal shapes (got {mu.shape}, {logvar.shape}, {eps.shape})")
    if any(t.dtype != "float32" for t in (mu, logvar, eps)):
        raise NotImplementedError("Only float32 is supported")
    md, ld, ed = (t.data.contiguous() for t in (mu, logvar, eps))
    z, std = torch.empty_like(md), torch.empty_like(md)
    call_hip_function("nnhipGaussianReparamForward", md, ld, ed, z, std, z.numel(), get_current_stream_ptr())
    rg = mu.requires_grad or logvar.requires_grad
    out = Tensor(z, (mu, logvar) if rg else None, "reparameterize", requires_grad=rg, device="cuda", _nocopy=True)

    def grad_fn(a, b, grad):
        dmu, dlv = torch.empty_like(md), torch.empty_like(md)
        call_hip_function("nnhipGaussianReparamBackward", grad.contiguous(), ed, std, dmu, dlv, dmu.numel(), get_current_stream_ptr())
        a.apply_grad(dmu)
        b.apply_grad(dlv)

    out.grad_fn = grad_fn
    return out


class _KLDTensor(Tensor):
    _implicit_seed = True      # backward() with no argument needs no ones tensor (as the fused loss tensors)


def gaussian_kld(mu: Tensor, logvar: Tensor) -> Tensor:
    """KLD = -0.5 * sum(1 + logvar - mu^2 - exp(logvar)), a 0-d tensor -- VAE.loss_function of examples/vae.ipynb; value and both
    gradients (dmu = mu, dlogvar = 0.5 (exp(logvar) - 1), times the upstream gradient) from one launch (nnhipGaussianKLDForwardBackward)."""
    import torch
    from ._lib import call_hip_function, get_current_stream_ptr
    from .nn.experimental.utils import times_upstream
    if not isinstance(mu, Tensor) or not isinstance(logvar, Tensor):
        raise TypeError("gaussian_kld takes Tensors")
    if not (mu.device == logvar.device == "cuda"):
        raise ValueError("gaussian_kld needs its tensors on the HIP device ('cuda')")
    if tuple(mu.shape) != tuple(logvar.shape):
        raise ValueError(f"gaussian_kld needs equal shapes (got {mu.shape} and {logvar.shape})")
    if mu.dtype != "float32" or logvar.dtype != "float32":
        raise NotImplementedError("Only float32 is supported")
    md, ld = mu.data.contiguous(), logvar.data.contiguous()
    loss = torch.empty((), dtype=torch.float32, device=md.device)
    dmu, dlv = torch.empty_like(md), torch.empty_like(md)
    call_hip_function("nnhipGaussianKLDForwardBackward", md, ld, loss, dmu, dlv, md.numel(), get_current_stream_ptr())
    rg = mu.requires_grad or logvar.requires_grad
    out = _KLDTensor(loss, (mu, logvar) if rg else None, "gaussian_kld", requires_grad=rg, device="cuda", _nocopy=True)

    def grad_fn(a, b, grad):
        unit = getattr(out_ref(), "_seeded_with_ones", False)
        a.apply_grad(dmu if unit else times_upstream(dmu, grad))
        b.apply_grad(dlv if unit else times_upstream(dlv, grad))

    import weakref
    out_ref = weakref.ref(out)
    out.grad_fn = grad_fn
    return out


VQ_NARROW_MAX_D = 8      # NNHIP_VQ_NARROW_MAX_D (include/neunet_hip.h): up to here the search runs one lane per row, beyond on MFMA


def quantize(z: Tensor, codebook: Tensor, straight_through: bool = False):
    """(z_q, indices): every row of z [..., D] replaced by the nearest row of codebook [K, D] in squared Euclidean distance, and the
    int32 indices of those rows (shape z.shape[:-1], requires_grad=False) -- VQVAE.quantize of the reference's examples/vqvae.ipynb
    (matmul, two norm sums, a broadcast add, argmin and an Embedding gather there) as ONE launch that never writes the N x K distance
    matrix (nnhipVQNearest); ties and NaNs resolve as np.argmin does.
    Gradients of z_q: a codebook that requires a gradient receives the reference's -- `Tensor.__getitem__`'s backward ASSIGNS, so a
    code chosen by several rows keeps the gradient of the LAST of them (nnhipEmbeddingBackward, as nn.Embedding).  z receives the
    upstream gradient unchanged if straight_through (the usual z + (z_q - z).detach(); off by default: the notebook has none) and
    nothing otherwise.  With neither, z_q is off the tape (requires_grad=False): the notebook's case, whose codebook is a plain
    tensor."""
    import torch
    from ._lib import call_hip_function, get_current_stream_ptr
    if not isinstance(z, Tensor) or not isinstance(codebook, Tensor):
        raise TypeError("quantize takes Tensors")
    if z.dtype != "float32" or codebook.dtype != "float32":
        raise NotImplementedError("Only float32 is supported")
    if codebook.ndim != 2:
        raise ValueError(f"quantize needs a 2-D codebook [K, D] (got {codebook.shape})")
    if z.ndim < 1 or z.shape[-1] != codebook.shape[1]:
        raise ValueError(f"quantize needs z [..., D] and codebook [K, D] with one D (got {z.shape} and {codebook.shape})")
    K, D = codebook.shape
    lead = tuple(z.shape[:-1])
    N = int(np.prod(lead, dtype=np.int64))
    if N == 0 or K == 0 or D == 0:
        raise ValueError(f"quantize needs at least one row, one code and one component (got {z.shape} and {codebook.shape})")
    if not (z.device == codebook.device == "cuda"):
        raise ValueError("quantize needs its tensors on the HIP device ('cuda')")
    zd, cd = z.data.contiguous(), codebook.data.contiguous()
    zq = torch.empty_like(zd)
    idx = torch.empty(lead, dtype=torch.int32, device=zd.device)
    call_hip_function("nnhipVQNearest", zd, cd, idx, zq, N, D, K, get_current_stream_ptr())
    indices = Tensor(idx, dtype=np.int32, requires_grad=False, device="cuda", _nocopy=True)
    to_z, to_cb = bool(straight_through) and z.requires_grad, codebook.requires_grad
    if not (to_z or to_cb):
        return Tensor(zq, None, "quantize", requires_grad=False, device="cuda", _nocopy=True), indices
    out = Tensor(zq, (z, codebook), "quantize", requires_grad=True, device="cuda", _nocopy=True)

    def grad_fn(a, cb, grad):
        from .nn.experimental.embedding import hip_embedding_backward
        from .nn.experimental.linear import _finish_param, _grad_out
        grad = grad if grad.is_contiguous() else grad.contiguous()
        if to_cb:
            grad_cb = _grad_out(cb, cb.data)
            hip_embedding_backward(grad_cb, grad.reshape(N, D), idx.reshape(N), 1.0)
            _finish_param(cb, grad_cb)
        if to_z:
            a.apply_grad(grad)

    out.grad_fn = grad_fn
    return out, indices


class _VQLossTensor(Tensor):
    _implicit_seed = True      # backward() with no argument needs no ones tensor (as the fused loss tensors)


def vq_loss(z_e: Tensor, z_q: Tensor, beta: float = 0.25) -> Tensor:
    """vq_loss + beta * commit_loss of VQVAE.loss_function (examples/vqvae.ipynb) = MSE(z_q, z_e.detach()) + beta * MSE(z_q.detach(), z_e),
    a 0-d tensor: (1 + beta) mean((z_q - z_e)^2).  Value and both gradients from one launch (nnhipVQLossForwardBackward):
    2 beta (z_e - z_q) / n goes to z_e, 2 (z_q - z_e) / n to z_q if it is on the tape, each times the upstream gradient."""
    import torch
    from ._lib import call_hip_function, get_current_stream_ptr
    from .nn.experimental.utils import times_upstream
    if not isinstance(z_e, Tensor) or not isinstance(z_q, Tensor):
        raise TypeError("vq_loss takes Tensors")
    if z_e.dtype != "float32" or z_q.dtype != "float32":
        raise NotImplementedError("Only float32 is supported")
    if tuple(z_e.shape) != tuple(z_q.shape):
        raise ValueError(f"vq_loss needs equal shapes (got {z_e.shape} and {z_q.shape})")
    if z_e.size == 0:
        raise ValueError("vq_loss needs at least one element")
    if not (z_e.device == z_q.device == "cuda"):
        raise ValueError("vq_loss needs its tensors on the HIP device ('cuda')")
    ed, qd = z_e.data.contiguous(), z_q.data.contiguous()
    loss = torch.empty((), dtype=torch.float32, device=ed.device)
    dze = torch.empty_like(ed) if z_e.requires_grad else None
    dzq = torch.empty_like(qd) if z_q.requires_grad else None
    call_hip_function("nnhipVQLossForwardBackward", ed, qd, float(beta), loss, dze, dzq, ed.numel(), get_current_stream_ptr())
    rg = z_e.requires_grad or z_q.requires_grad
    out = _VQLossTensor(loss, (z_e, z_q) if rg else None, "vq_loss", requires_grad=rg, device="cuda", _nocopy=True)

    def grad_fn(a, b, grad):
        unit = getattr(out_ref(), "_seeded_with_ones", False)
        if dze is not None:
            a.apply_grad(dze if unit else times_upstream(dze, grad))
        if dzq is not None:
            b.apply_grad(dzq if unit else times_upstream(dzq, grad))

    import weakref
    out_ref = weakref.ref(out)
    out.grad_fn = grad_fn
    return out


def save(obj, path):
    """neunet.save = pickle (neunet/__init__.py:26-29)."""
    import pickle
    with open(path, "wb") as f:
        pickle.dump(obj, f)


def load(path):
    import pickle
    with open(path, "rb") as f:
        return pickle.load(f)


# ---- the Tensor arithmetic as functions (neunet/__init__.py:152-246); device float32, see neunet_hip/tensor_ops.py ------------------
def add(x, y):
    return x + y


def sub(x, y):
    return x - y


def mul(x, y):
    return x * y


def div(x, y):
    return x / y


def matmul(x, y):
    return x.matmul(y)


def sum(x, axis=None, keepdims=False):      # noqa: A001  (the reference's names)
    return x.sum(axis=axis, keepdims=keepdims)


def mean(x, axis=None, keepdims=False):
    return x.mean(axis=axis, keepdims=keepdims)


def var(x, axis=None, keepdims=False):
    return x.var(axis=axis, keepdims=keepdims)


def power(x, y):
    return x ** y


def sqrt(x):
    return x.sqrt()


def log(x):
    return x.log()


def exp(x):
    return x.exp()


def tanh(x):
    return x.tanh()


def sin(x):
    return x.sin()


def cos(x):
    return x.cos()


def maximum(x, y):
    return x.maximum(y)


def minimum(x, y):
    return x.minimum(y)


def max(x, axis=None, keepdims=False):      # noqa: A001
    return x.max(axis=axis, keepdims=keepdims)


def min(x, axis=None, keepdims=False):      # noqa: A001
    return x.min(axis=axis, keepdims=keepdims)


def reshape(x, *shape):
    return x.reshape(*shape)


def abs(x):                                 # noqa: A001
    return x.abs()


def transpose(x, *axes):
    return x.transpose(*axes)


def swapaxes(x, axis1, axis2):
    return x.swapaxes(axis1, axis2)


# ---- comparisons, logical ops, where, flip as functions (neunet/__init__.py:249-281); see neunet_hip/tensor_index.py ---------------------
def flip(x, axis):
    return x.flip(axis=axis)


def where(condition, x, y):
    """np.where(condition, x, y): x and y float32 Tensors or scalars (a scalar travels by value, it becomes no tensor)."""
    from .tensor_index import where as _where
    return _where(condition, x, y)


def equal(x, y):
    return x.equal(y)


def not_equal(x, y):
    return x.not_equal(y)


def greater(x, y):
    return x.greater(y)


def greater_equal(x, y):
    return x.greater_equal(y)


def less(x, y):
    return x.less(y)


def less_equal(x, y):
    return x.less_equal(y)


def logical_and(x, y):
    return x.logical_and(y)


def logical_or(x, y):
    return x.logical_or(y)


def logical_not(x):
    return x.logical_not()
