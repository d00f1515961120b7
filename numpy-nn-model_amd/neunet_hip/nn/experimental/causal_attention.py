"""HIPCausalSelfAttention + KVCache -- GPT-2's attention block (the CausalSelfAttention class of the reference's
examples/gpt2/gpt2_infer.py:129-182: c_attn D -> 3D, causal softmax(q k^T / sqrt(head_dim)) v, c_proj) with incremental decoding.

Training and prefill run the flash-style kernels on the three column blocks of c_attn's [B,T,3D] output (no transposes, the score
matrix is never written); a head dim outside FUSED_HEAD_DIMS takes the unfused GEMM + masked-softmax path.  With a KVCache:
T > 1 is the prefill (causal forward, then k and v go into the cache), T == 1 is one decode step on nnhipAttentionDecode
(csrc/attention_decode.hip).  No autograd tape is recorded on the cache path.

Cache layout (the decode kernel's choice): K and V each [n_layer, B, H, Tmax, dh] fp32, HEAD-MAJOR inside a layer, so a head's
keys are one contiguous stream.  `cache_len` is ONE device int32[B] shared by the layers: every layer of a step appends at the same
index, and the model advances it once per step with a torch op (KVCache.advance) -- nothing of a decode step depends on a
host-side position, so the step can be captured into a hipGraph and replayed."""
import math

from ...autograd import Tensor
from ..modules import Module
from ..._lib import load_hip_function
from .attention import (FUSED_HEAD_DIMS, FusedAttentionOptions, _HIPAttentionTensor, _HIPFusedSelfAttentionTensor, _SEEDS,
                        attention_forward, fused_attention_forward)
from .embedding import HIPDropout, check_capture_seed, process_dropout_seed
from .linear import HIPLinear, hip_linear_module_forward
from .utils import call_hip_function, get_current_stream_ptr, require_device_f32


def decode_workspace_bytes(B, H, Tmax, dh) -> int:
    """nnhipAttentionDecodeWorkspace: bytes of split partials one decode call needs (a host-side computation, no device involved)."""
    n = load_hip_function("nnhipAttentionDecodeWorkspace")(B, H, Tmax, dh)
    if n < 0:
        from ..._lib import NeunetHipError, last_error
        raise NeunetHipError(f"nnhipAttentionDecodeWorkspace failed with status {n}: {last_error()}")
    return int(n)


class KVCacheLayer:
    """One layer's view of a KVCache: what HIPCausalSelfAttention.forward(x, cache=...) takes."""
    __slots__ = ("owner", "index", "k", "v")

    def __init__(self, owner, index):
        self.owner, self.index = owner, index
        self.k, self.v = owner.k[index], owner.v[index]


class KVCache:
    """KVCache(B, Tmax, n_layer, H, dh): owns the K / V buffers, the device-side `cache_len` int32[B] and the decode workspace.

    `tokens` is the host's mirror of the longest row (what the layers check capacity against without reading the device);
    cache_len itself only ever changes through advance() / reset() / set_lengths()."""

    def __init__(self, B, Tmax, n_layer, H, dh, device="cuda"):
        import torch
        if dh not in FUSED_HEAD_DIMS:
            raise ValueError(f"KVCache: head dim {dh} is not one the decode kernel has ({FUSED_HEAD_DIMS})")
        if min(B, Tmax, n_layer, H) < 1:
            raise ValueError("KVCache: B, Tmax, n_layer and H must be >= 1")
        self.B, self.Tmax, self.n_layer, self.H, self.dh = B, Tmax, n_layer, H, dh
        self.k = torch.zeros((n_layer, B, H, Tmax, dh), dtype=torch.float32, device=device)
        self.v = torch.zeros((n_layer, B, H, Tmax, dh), dtype=torch.float32, device=device)
        self.cache_len = torch.zeros((B,), dtype=torch.int32, device=device)
        nbytes = decode_workspace_bytes(B, H, Tmax, dh)
        self.workspace = torch.empty((max(nbytes // 4, 1),), dtype=torch.float32, device=device) if nbytes else None
        self.tokens = 0
        self._layers = [KVCacheLayer(self, i) for i in range(n_layer)]

    def layer(self, i) -> KVCacheLayer:
        return self._layers[i]

    def room(self) -> int:
        return self.Tmax - self.tokens

    def check_room(self, T):
        if T > self.room():
            raise ValueError(f"KVCache: {T} more token(s) do not fit ({self.tokens} of {self.Tmax} used)")

    def advance(self, T=1):
        """After EVERY layer of a step has appended: cache_len += T on the device (one torch op, capturable)."""
        self.check_room(T)
        self.cache_len.add_(T)
        self.tokens += T

    def replayed(self, T=1):
        """Host bookkeeping for a captured step that was replayed (its advance() ran on the device only)."""
        self.check_room(T)
        self.tokens += T

    def set_lengths(self, lengths):
        """Ragged rows: cache_len[b] = lengths[b] (the caller filled the buffers accordingly)."""
        import torch
        lengths = [int(n) for n in lengths]
        if len(lengths) != self.B or min(lengths) < 0 or max(lengths) > self.Tmax:
            raise ValueError("KVCache.set_lengths: one length in 0 .. Tmax per row")
        self.cache_len.copy_(torch.tensor(lengths, dtype=torch.int32))
        self.tokens = max(lengths)

    def reset(self):
        self.cache_len.zero_()
        self.tokens = 0


def kv_cache_fill(qkv, layer: KVCacheLayer, T):
    """Prefill copy: k and v of qkv [B, T, 3D] into the layer's cache at cache_len[b] + 0..T-1 (nnhipKVCacheFill)."""
    c = layer.owner
    call_hip_function("nnhipKVCacheFill", qkv, layer.k, layer.v, c.cache_len, c.B, c.H, T, c.Tmax, c.dh, qkv.shape[-1],
                      get_current_stream_ptr())


def attention_decode(qkv, layer: KVCacheLayer, out, scale):
    """One decode step of one layer: qkv [B, 3D] -> out [B, D]; appends k, v at cache_len[b] (nnhipAttentionDecode)."""
    c = layer.owner
    call_hip_function("nnhipAttentionDecode", qkv, layer.k, layer.v, c.cache_len, out, c.workspace, c.B, c.H, c.Tmax, c.dh,
                      qkv.shape[-1], float(scale), get_current_stream_ptr())
    return out


class _ColumnBlockTensor(Tensor):
    """A dense copy of columns [lo, hi) of a [B,T,3D] projection (the unfused attention path's GEMMs want dense q, k, v).  The three
    blocks of one projection gather their gradients in ONE [B,T,3D] buffer; the last to arrive hands it to the parent."""

    def __init__(self, parent: Tensor, lo, hi, shared):
        super().__init__(parent.data[..., lo:hi].contiguous(), (parent, lo, hi, shared), "column_block",
                         requires_grad=parent.requires_grad, device=parent.device, _nocopy=True)

        def grad_fn(p, lo, hi, shared, grad):
            import torch
            if shared.get("buf") is None:
                shared["buf"], shared["got"] = torch.zeros_like(p.data), 0
            shared["buf"][..., lo:hi].copy_(grad)
            shared["got"] += 1
            if shared["got"] == shared["n"]:
                buf, shared["buf"] = shared["buf"], None
                p.apply_grad(buf)

        self.grad_fn = grad_fn


class HIPCausalSelfAttention(Module):
    def __init__(self, n_embd, n_head, attn_pdrop=0.0, resid_pdrop=0.0, device="cuda"):
        super().__init__()
        if n_embd % n_head != 0:
            raise ValueError("n_embd must be divisible by n_head")
        self.n_embd, self.n_head, self.device = n_embd, n_head, device
        self.head_dim = n_embd // n_head
        self.scale = 1.0 / math.sqrt(self.head_dim)
        self.c_attn = HIPLinear(n_embd, 3 * n_embd, bias=True, device=device)
        self.c_proj = HIPLinear(n_embd, n_embd, bias=True, device=device)
        self.attn_drop = HIPDropout(attn_pdrop)
        self.resid_drop = HIPDropout(resid_pdrop)
        self.dropout_seed_dev = None      # graph.attach_step_seed: a device step word for the in-kernel attention dropout
        self._seed_base = (next(_SEEDS) * 0x9E3779B9) & 0x7FFFFFFF
        self._calls = 0

    def _next_seed(self):
        check_capture_seed(self.dropout_seed_dev, "HIPCausalSelfAttention")
        self._calls += 1
        return (self._seed_base + self._calls + process_dropout_seed()) & 0xFFFFFFFF

    def forward(self, x: Tensor, cache: KVCacheLayer = None, residual: Tensor = None) -> Tensor:
        """residual (extension, as HIPLinear's): returns residual + attention(x), the add folded into c_proj's epilogue."""
        require_device_f32(x)
        if x.ndim != 3 or x.shape[-1] != self.n_embd:
            raise ValueError(f"expected [B, T, {self.n_embd}], got {x.shape}")
        if cache is not None:
            return self._forward_cached(x, cache, residual)
        D, H = self.n_embd, self.n_head
        divisor = math.sqrt(self.head_dim)         # the attention entry points take the DIVISOR of the scores
        dropping = self.attn_drop.p != 0 and self.attn_drop.training
        qkv_t = self.c_attn(x)
        qkv = qkv_t.data
        if self.head_dim in FUSED_HEAD_DIMS:
            opts = None
            if dropping:
                opts = FusedAttentionOptions(dropout_p=self.attn_drop.p, seed=self._next_seed(), seed_dev=self.dropout_seed_dev)
            ctx, lse = fused_attention_forward(qkv[..., 0:D], qkv[..., D:2 * D], qkv[..., 2 * D:], None, H, divisor, True, opts)
            ctx_t = _HIPFusedSelfAttentionTensor(ctx, (qkv_t, lse, None, H, divisor, True, opts), "fused_self_attention", device="cuda")
        else:
            shared = {"n": 3}
            q, k, v = (_ColumnBlockTensor(qkv_t, i * D, (i + 1) * D, shared) for i in range(3))
            drop_mask = None
            if dropping:
                import torch
                shape = (x.shape[0], H, x.shape[1], x.shape[1])
                drop_mask = torch.empty(shape, dtype=torch.float32, device=qkv.device)
                call_hip_function("nnhipAttentionDropoutMaskEx", drop_mask, *shape, float(self.attn_drop.p), self._next_seed(),
                                  self.dropout_seed_dev, get_current_stream_ptr())
            ctx, attn, used = attention_forward(q.data, k.data, v.data, None, H, divisor, True, drop_mask)
            ctx_t = _HIPAttentionTensor(ctx, (q, k, v, attn, None, H, divisor, True, drop_mask,
                                              used if drop_mask is not None else None, None), "attention", device="cuda")
        if residual is not None and not (self.resid_drop.p != 0 and self.resid_drop.training):
            return self.c_proj(ctx_t, residual=residual)
        y = self.resid_drop(self.c_proj(ctx_t))
        return y if residual is None else residual + y

    def _forward_cached(self, x: Tensor, layer: KVCacheLayer, residual=None) -> Tensor:
        import torch
        c = layer.owner
        B, T, D = x.shape
        if (B, self.n_head, self.head_dim) != (c.B, c.H, c.dh):
            raise ValueError(f"KVCache is for (B, H, dh) = {(c.B, c.H, c.dh)}, the input needs {(B, self.n_head, self.head_dim)}")
        c.check_room(T)
        xd = x.data if x.data.is_contiguous() else x.data.contiguous()
        qkv = torch.empty((B, T, 3 * D), dtype=torch.float32, device=xd.device)
        hip_linear_module_forward(xd, self.c_attn.weight.data, self.c_attn.bias.data, qkv, B * T, D, 3 * D)
        if T == 1:
            ctx = torch.empty((B, 1, D), dtype=torch.float32, device=xd.device)
            attention_decode(qkv, layer, ctx, self.scale)
        else:
            if c.tokens != 0:
                raise ValueError("KVCache: a multi-token call is the prefill of an EMPTY cache; continue token by token (T == 1)")
            ctx, _ = fused_attention_forward(qkv[..., 0:D], qkv[..., D:2 * D], qkv[..., 2 * D:], None, self.n_head,
                                             math.sqrt(self.head_dim), True, None)
            kv_cache_fill(qkv, layer, T)
        out = torch.empty((B, T, D), dtype=torch.float32, device=xd.device)
        hip_linear_module_forward(ctx, self.c_proj.weight.data, self.c_proj.bias.data, out, B * T, D, D,
                                  addend=residual.data if residual is not None else None)
        return Tensor._wrap(out, None, "causal_self_attention", "cuda", requires_grad=False)
