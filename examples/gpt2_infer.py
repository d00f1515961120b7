"""GPT-2 inference on the HIP path -- the reference's examples/gpt2/gpt2_infer.py with a KV cache.

    python examples/gpt2_infer.py --random --seed 0 --mode graph --max-new-tokens 64
    python examples/gpt2_infer.py --weights /path/to/pytorch_model.bin --ids 15496,11,314 --mode cached

Module tree and attribute names are the reference script's (wte, wpe, h[i].ln_1 / attn.c_attn / attn.c_proj / ln_2 / mlp.c_fc /
mlp.c_proj, ln_f, a tied lm_head), so load_gpt2_weights is a key-for-key copy of a Hugging Face state dict with the reference
loader's transposes.  Nothing is downloaded: --weights takes a local pytorch_model.bin (or .safetensors if that package is
importable), --random builds GPT-2-small-shaped random weights.  Token ids go in and out; --prompt needs the `tokenizers` package
and a local tokenizer.json (--tokenizer).

generate(ids, max_new_tokens, temperature, top_k, mode):
  recompute  the reference's loop (NeunetGPT2Runner.generate): a full forward over the whole prefix per token, O(T^2) per sequence
  cached     prefill once, then one single-token step per new token on the KV cache (nnhipAttentionDecode), eager launches
  graph      the single-token step is captured into a hipGraph once and replayed; greedy: nnhipArgmaxF32 writes the next id into
             the buffer the next replay reads and the positional row is gathered by cache_len, so the host synchronises once, at
             the end.  Sampling (top_k > 0) with sampler="host" reads the logits on the host after every replay, as the eager
             modes do; with sampler="device" nnhipSampleTopK sits where the argmax does and the loop is the greedy one.

sampler (top_k > 0 only; top_k == 0 is greedy either way):
  host    the reference's choice in NumPy (argpartition, softmax, Generator.choice) on a host copy of the logits: one
          synchronisation and a [B, vocab] transfer per token in every mode
  device  neunet_hip.sample_top_k: the token at sequence position p (0-based, prompt included) of row b is drawn with the uniform
          of (seed + p, b) in every mode -- the eager modes add p on the host, the captured step reads it from cache_len

linear (cached and graph modes; recompute ignores it):
  gemm    every Linear on the tiled MFMA GEMM (the default: the tokens of existing seeds stay what they are)
  gemv    the run happens under neunet_hip.linear_gemv(): every Linear forward of 1..8 rows -- the single-token steps up to batch 8,
          the graph mode's warm-up and capture included, and a prefill of at most 8 rows -- streams its weights once through
          nnhipLinearGemvForward's kernel, one launch and no split-K reduce.  Another summation order: logits move in their last
          bits.  The switch is back at its previous value when generate returns.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip  # noqa: E402,F401
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip import Tensor  # noqa: E402
from neunet_hip.nn.experimental.embedding import hip_embedding_backward, hip_embedding_forward  # noqa: E402
from neunet_hip.nn.experimental.linear import _finish_param, _grad_out, hip_linear_module_forward  # noqa: E402
from neunet_hip.nn.experimental.utils import call_hip_function, get_current_stream_ptr  # noqa: E402

GPT2_SMALL = {"n_embd": 768, "n_head": 12, "n_layer": 12, "vocab_size": 50257, "n_positions": 1024, "layer_norm_epsilon": 1e-5}


class MLP(nn.Module):
    def __init__(self, n_embd, resid_pdrop=0.0, device="cuda"):
        super().__init__()
        self.c_fc = nn.Linear(n_embd, 4 * n_embd, bias=True, device=device)
        self.c_proj = nn.Linear(4 * n_embd, n_embd, bias=True, device=device)
        self.act = nn.GELU()
        self.drop = nn.Dropout(resid_pdrop)

    def forward(self, x, residual=None):
        h = self.act(self.c_fc(x))
        if residual is not None and not (self.drop.p != 0 and self.drop.training):
            return self.c_proj(h, residual=residual)          # x + mlp(...) with the add in the GEMM epilogue
        y = self.drop(self.c_proj(h))
        return y if residual is None else residual + y


class GPT2Block(nn.Module):
    def __init__(self, n_embd, n_head, ln_eps, attn_pdrop, resid_pdrop, device="cuda"):
        super().__init__()
        self.ln_1 = nn.LayerNorm(n_embd, eps=ln_eps, device=device)
        self.attn = nn.CausalSelfAttention(n_embd, n_head, attn_pdrop, resid_pdrop, device=device)
        self.ln_2 = nn.LayerNorm(n_embd, eps=ln_eps, device=device)
        self.mlp = MLP(n_embd, resid_pdrop, device=device)

    def forward(self, x, cache=None):
        x = self.attn(self.ln_1(x), cache=cache, residual=x)
        return self.mlp(self.ln_2(x), residual=x)


class _TokenPlusPositionTensor(Tensor):
    """wte(idx) + wpe(pos) from ONE gather launch (nnhipEmbeddingForward with the positional table fused in).  Backward: the token
    table gets the embedding gradient (the reference's last-occurrence-wins assignment, autograd.py:905-912), the first T rows of
    the positional table get the gradient summed over the batch -- what the reference's reverse broadcast of wpe(pos [1,T]) leaves."""

    def __init__(self, data, args, op, device):
        super().__init__(data, args, op, device=device, _nocopy=True)

        def grad_fn(wte: Tensor, wpe: Tensor, ids, T, grad):
            import torch
            grad = grad if grad.is_contiguous() else grad.contiguous()
            g_tok = _grad_out(wte, wte.data)
            hip_embedding_backward(g_tok, grad, ids, 1.0)
            _finish_param(wte, g_tok)
            g_pos = torch.zeros_like(wpe.data)
            g_pos[:T] = grad.reshape(-1, T, grad.shape[-1]).sum(0)
            _finish_param(wpe, g_pos)

        self.grad_fn = grad_fn


class GPT2(nn.Module):
    def __init__(self, cfg, device="cuda"):
        """device="cpu" builds the parameter skeleton only (host-side tests of the loader): every forward needs the HIP device."""
        super().__init__()
        self.cfg = dict(cfg)
        n_embd, n_head, n_layer = cfg["n_embd"], cfg["n_head"], cfg["n_layer"]
        self.n_embd, self.n_head, self.n_layer, self.vocab_size = n_embd, n_head, n_layer, cfg["vocab_size"]
        self.n_positions = cfg.get("n_positions", cfg.get("n_ctx", 1024))
        ln_eps = cfg.get("layer_norm_epsilon", 1e-5)
        attn_pdrop, resid_pdrop, embd_pdrop = cfg.get("attn_pdrop", 0.0), cfg.get("resid_pdrop", 0.0), cfg.get("embd_pdrop", 0.0)
        self.wte = nn.Embedding(self.vocab_size, n_embd, device=device)
        self.wpe = nn.Embedding(self.n_positions, n_embd, device=device)
        self.drop = nn.Dropout(embd_pdrop)
        self.h = nn.ModuleList([GPT2Block(n_embd, n_head, ln_eps, attn_pdrop, resid_pdrop, device=device) for _ in range(n_layer)])
        self.ln_f = nn.LayerNorm(n_embd, eps=ln_eps, device=device)
        self.lm_head = nn.Linear(n_embd, self.vocab_size, bias=False, device=device)
        self.lm_head.weight = self.wte.weight           # weight tying: ONE Parameter object, so ONE gradient (the sum of both uses)
        self.device = device

    def to(self, device):
        super().to(device)
        self.lm_head.weight = self.wte.weight           # Module.to rebinds attribute by attribute: tie again
        return self

    def new_cache(self, B, Tmax=None):
        return nn.KVCache(B, Tmax or self.n_positions, self.n_layer, self.n_head, self.n_embd // self.n_head)

    def forward(self, idx, cache=None, last_only=False):
        """idx: int ids [B, T] (NumPy, torch or Tensor).  Returns the logits Tensor [B, T, vocab].  With a cache: T > 1 prefills an
        empty cache, T == 1 is one decode step at position cache_len (the same for every row here); the cache is advanced.
        last_only (cache path): logits of the last position only, [B, 1, vocab] -- all a prefill needs."""
        import torch
        ids = idx.data if isinstance(idx, Tensor) else idx
        ids = torch.as_tensor(np.asarray(ids) if not isinstance(ids, torch.Tensor) else ids).to(device="cuda", dtype=torch.int32).contiguous()
        B, T = ids.shape
        pos0 = cache.tokens if cache is not None else 0
        if pos0 + T > self.n_positions:
            raise ValueError(f"sequence of {pos0 + T} tokens exceeds n_positions = {self.n_positions}")
        out = torch.empty((B, T, self.n_embd), dtype=torch.float32, device="cuda")
        hip_embedding_forward(out, self.wte.weight.data, ids, self.wpe.weight.data[pos0:pos0 + T], T, 1.0)
        if cache is None:
            x = _TokenPlusPositionTensor(out, (self.wte.weight, self.wpe.weight, ids, T), "gpt2_embedding", device="cuda")
        else:
            x = Tensor._wrap(out, None, "gpt2_embedding", "cuda", requires_grad=False)
        x = self.drop(x)
        for i, block in enumerate(self.h):
            x = block(x, cache=cache.layer(i) if cache is not None else None)
        if cache is not None:
            cache.advance(T)
            if last_only and T > 1:
                x = Tensor._wrap(x.data[:, -1:, :].contiguous(), None, "last_position", "cuda", requires_grad=False)
        return self.lm_head(self.ln_f(x))


def _to_numpy(x):
    if isinstance(x, np.ndarray):
        return x
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _get_key(state, key):
    for pref in ("", "transformer.", "gpt2.", "model.", "module."):
        if pref + key in state:
            return state[pref + key]
    for pref in ("transformer.", "gpt2.", "model.", "module."):
        if key.startswith(pref) and key[len(pref):] in state:
            return state[key[len(pref):]]
    raise KeyError(f"Key '{key}' not found in state dict. Sample keys: {list(state.keys())[:20]}")


def _assign(param, value):
    """Copy into the parameter's device buffer in place (shapes must agree: a wrong transpose is an error, not a reshape)."""
    value = np.ascontiguousarray(_to_numpy(value), dtype=np.float32)
    if tuple(value.shape) != tuple(param.shape):
        raise ValueError(f"shape mismatch: parameter {tuple(param.shape)}, checkpoint {tuple(value.shape)}")
    if isinstance(param.data, np.ndarray):
        param.data[...] = value
    else:
        import torch
        param.data.copy_(torch.from_numpy(value))


def load_gpt2_weights(model: GPT2, state) -> None:
    """Key-for-key copy of a Hugging Face GPT-2 state dict.  HF's Conv1D stores [in, out]; nn.Linear here holds [out, in] and a
    [1, out] bias: the same transposes and reshapes as the reference loader.  lm_head stays tied to wte."""
    _assign(model.wte.weight, _get_key(state, "transformer.wte.weight"))
    _assign(model.wpe.weight, _get_key(state, "transformer.wpe.weight"))
    for i in range(len(model.h)):
        prefix, block = f"transformer.h.{i}.", model.h[i]
        _assign(block.ln_1.weight, _get_key(state, prefix + "ln_1.weight"))
        _assign(block.ln_1.bias, _get_key(state, prefix + "ln_1.bias"))
        _assign(block.attn.c_attn.weight, _to_numpy(_get_key(state, prefix + "attn.c_attn.weight")).T)
        _assign(block.attn.c_attn.bias, _to_numpy(_get_key(state, prefix + "attn.c_attn.bias")).reshape(1, -1))
        _assign(block.attn.c_proj.weight, _to_numpy(_get_key(state, prefix + "attn.c_proj.weight")).T)
        _assign(block.attn.c_proj.bias, _to_numpy(_get_key(state, prefix + "attn.c_proj.bias")).reshape(1, -1))
        _assign(block.ln_2.weight, _get_key(state, prefix + "ln_2.weight"))
        _assign(block.ln_2.bias, _get_key(state, prefix + "ln_2.bias"))
        _assign(block.mlp.c_fc.weight, _to_numpy(_get_key(state, prefix + "mlp.c_fc.weight")).T)
        _assign(block.mlp.c_fc.bias, _to_numpy(_get_key(state, prefix + "mlp.c_fc.bias")).reshape(1, -1))
        _assign(block.mlp.c_proj.weight, _to_numpy(_get_key(state, prefix + "mlp.c_proj.weight")).T)
        _assign(block.mlp.c_proj.bias, _to_numpy(_get_key(state, prefix + "mlp.c_proj.bias")).reshape(1, -1))
    _assign(model.ln_f.weight, _get_key(state, "transformer.ln_f.weight"))
    _assign(model.ln_f.bias, _get_key(state, "transformer.ln_f.bias"))
    model.lm_head.weight = model.wte.weight


def random_gpt2_state(cfg, seed=0):
    """A Hugging-Face-shaped state dict of N(0, 0.02) weights (HF's own initialisation scale), unit LayerNorm gains."""
    rng = np.random.default_rng(seed)
    D, V, P = cfg["n_embd"], cfg["vocab_size"], cfg.get("n_positions", 1024)
    n = lambda *s: (rng.standard_normal(s) * 0.02).astype(np.float32)  # noqa: E731
    sd = {"transformer.wte.weight": n(V, D), "transformer.wpe.weight": n(P, D),
          "transformer.ln_f.weight": np.ones(D, np.float32), "transformer.ln_f.bias": np.zeros(D, np.float32)}
    for i in range(cfg["n_layer"]):
        p = f"transformer.h.{i}."
        sd.update({p + "ln_1.weight": np.ones(D, np.float32), p + "ln_1.bias": np.zeros(D, np.float32),
                   p + "ln_2.weight": np.ones(D, np.float32), p + "ln_2.bias": np.zeros(D, np.float32),
                   p + "attn.c_attn.weight": n(D, 3 * D), p + "attn.c_attn.bias": n(3 * D),
                   p + "attn.c_proj.weight": n(D, D), p + "attn.c_proj.bias": n(D),
                   p + "mlp.c_fc.weight": n(D, 4 * D), p + "mlp.c_fc.bias": n(4 * D),
                   p + "mlp.c_proj.weight": n(4 * D, D), p + "mlp.c_proj.bias": n(D)})
    return sd


def load_state_dict_file(path):
    """A local checkpoint: .safetensors (if the package is importable) or a torch pickle.  Nothing is fetched."""
    if str(path).endswith(".safetensors"):
        try:
            from safetensors.numpy import load_file
        except Exception as exc:  # noqa: BLE001
            raise RuntimeError("the safetensors package is needed to read .safetensors weights; use pytorch_model.bin instead") from exc
        state = load_file(str(path))
    else:
        import torch
        state = torch.load(str(path), map_location="cpu")
    for wrap in ("state_dict", "model"):
        if wrap in state and isinstance(state[wrap], dict):
            state = state[wrap]
            break
    if any(k.startswith("module.") for k in state):
        state = {k.replace("module.", "", 1): v for k, v in state.items()}
    return state


def softmax_np(x):
    e = np.exp(x - np.max(x))
    return e / np.sum(e)


def _pick(last, temperature, top_k, rng):
    """The reference's choice of the next id from one row of logits (NeunetGPT2Runner.generate)."""
    if temperature != 1.0:
        last = last / max(temperature, 1e-6)
    if top_k > 0:
        k = min(top_k, last.shape[0])
        inds = np.argpartition(last, -k)[-k:]
        return int(rng.choice(inds, p=softmax_np(last[inds].astype(np.float64))))
    return int(np.argmax(last))


class GraphedDecodeStep:
    """One single-token step of `model` on `cache`, captured into a hipGraph: ids_buf [B,1] -> embedding (positional row gathered
    by cache_len) -> the blocks -> ln_f -> lm_head -> logits; greedy: argmax -> ids_buf; cache_len += 1; device sampler: top-k
    draw -> ids_buf.  One stream, no parallel branches.  kernel_nodes / graph_nodes: what graph.count_graph_nodes finds in the
    captured graph."""

    def __init__(self, model: GPT2, cache, greedy=True, sampler=None):
        """sampler: None, or (top_k, temperature, seed): the step ends in nnhipSampleTopK instead of the argmax, drawing with the
        uniform of (seed + cache_len, row) -- cache_len AFTER the step's advance, the position of the token being chosen."""
        import torch
        from neunet_hip.graph import count_graph_nodes
        self.model, self.cache, self.greedy, self.sampler = model, cache, greedy and sampler is None, sampler
        B, D = cache.B, model.n_embd
        self.ids_buf = torch.zeros((B, 1), dtype=torch.int32, device="cuda")
        self._tok = torch.empty((B, 1, D), dtype=torch.float32, device="cuda")
        self._pos = torch.empty((B, 1, D), dtype=torch.float32, device="cuda")
        self.logits = torch.empty((B, 1, model.vocab_size), dtype=torch.float32, device="cuda")
        self.replays = 0
        # warm-up on a side stream (grows the library workspace), on a scratch copy of the lengths: the cache is left as it was
        saved_len, saved_tokens = cache.cache_len.clone(), cache.tokens
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        cache.cache_len.copy_(saved_len)
        cache.tokens = saved_tokens
        self.graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self._step()
        cache.tokens = saved_tokens                      # the capture ran the host bookkeeping of one step without executing it
        self.kernel_nodes, self.graph_nodes = count_graph_nodes(self.graph.raw_cuda_graph())
        self.graph.instantiate()
        call_hip_function("nnhipWorkspaceLock", 1)       # the graph holds library-owned addresses: nothing may move them
        self._locked = True

    def _step(self):
        m, c = self.model, self.cache
        st = get_current_stream_ptr
        # token row + positional row gathered by cache_len (device-side position), then the blocks on the cache
        hip_embedding_forward(self._tok, m.wte.weight.data, self.ids_buf, None, 1, 1.0)
        hip_embedding_forward(self._pos, m.wpe.weight.data, c.cache_len, None, 1, 1.0)
        call_hip_function("nnhipAdd", self._tok, self._tok, self._pos, self._tok.numel(), st())
        x = Tensor._wrap(self._tok, None, "gpt2_embedding", "cuda", requires_grad=False)
        for i, block in enumerate(m.h):
            x = block(x, cache=c.layer(i))
        x = m.ln_f(x)
        hip_linear_module_forward(x.data, m.lm_head.weight.data, None, self.logits, c.B, m.n_embd, m.vocab_size)
        if self.greedy:
            call_hip_function("nnhipArgmaxF32", self.ids_buf, self.logits, c.B, m.vocab_size, 1, st())
        c.advance(1)
        if self.sampler is not None:
            # after the advance: cache_len[0] is now the position of the token this step chooses (rows advance in lockstep)
            top_k, temperature, seed = self.sampler
            neunet_hip.sample_top_k(self.logits[:, 0], top_k, temperature, seed=seed, seed_dev=c.cache_len, out=self.ids_buf)

    def replay(self):
        self.cache.replayed(1)
        self.graph.replay()
        self.replays += 1

    def release(self):
        if getattr(self, "_locked", False):
            self._locked = False
            call_hip_function("nnhipWorkspaceLock", 0)
        self.graph = None

    def __del__(self):
        try:
            self.release()
        except Exception:  # noqa: BLE001
            pass


def _sync_clock():
    """Host clock after a device synchronise: the edges of generate's timing windows (never between two tokens)."""
    import torch
    torch.cuda.synchronize()
    return time.perf_counter()


def generate(model: GPT2, ids, max_new_tokens, temperature=1.0, top_k=0, mode="cached", seed=None, stats=None, sampler="host",
             linear="gemm"):
    """ids: int array [B, T0] (or [T0]).  Returns int32 [B, T0 + max_new_tokens].  temperature / top_k as in the reference script
    (top_k == 0: greedy).  sampler: who draws when top_k > 0, "host" (NumPy on a copy of the logits) or "device"
    (neunet_hip.sample_top_k, seeded per position: see the module docstring).  linear: "gemm" or "gemv" (module docstring).  stats (a
    dict, optional) receives what the run did: host synchronisations between tokens, replays, graph node counts, the linear setting,
    and prefill_s / capture_s / decode_s, the seconds of the prefill, of the graph warm-up + capture and of the token loop (the last
    new token's choice included)."""
    if sampler not in ("host", "device"):
        raise ValueError(f"unknown sampler {sampler!r} (host, device)")
    if linear not in ("gemm", "gemv"):
        raise ValueError(f"unknown linear {linear!r} (gemm, gemv)")
    stats = stats if stats is not None else {}
    stats["linear"] = linear
    if linear == "gemv" and mode in ("cached", "graph"):
        with neunet_hip.linear_gemv(True):
            return _generate(model, ids, max_new_tokens, temperature, top_k, mode, seed, stats, sampler)
    return _generate(model, ids, max_new_tokens, temperature, top_k, mode, seed, stats, sampler)


def _generate(model, ids, max_new_tokens, temperature, top_k, mode, seed, stats, sampler):
    import torch
    ids = np.atleast_2d(np.asarray(ids, dtype=np.int32))
    B, T0 = ids.shape
    if T0 < 1 or max_new_tokens < 0:
        raise ValueError("generate needs a prompt of at least one token and max_new_tokens >= 0")
    if T0 + max_new_tokens > model.n_positions:
        raise ValueError(f"{T0} + {max_new_tokens} tokens exceed n_positions = {model.n_positions}")
    rng = np.random.default_rng(seed)
    greedy = top_k <= 0
    device_draw = sampler == "device" and not greedy
    seed0 = int(seed or 0)

    def draw(logits, p, out=None):
        """The device sampler on the last position's logits, for the token at sequence position p."""
        return neunet_hip.sample_top_k(logits.data[:, -1], top_k, temperature, seed=seed0 + p, out=out)

    def pick_rows(logits, p):
        """The next id of every row as a host array: the one transfer per token of the eager modes."""
        if device_draw:
            return draw(logits, p).cpu().numpy().astype(np.int32)
        last = logits.data[:, -1].cpu().numpy()
        return np.array([_pick(last[b], temperature, top_k, rng) for b in range(B)], dtype=np.int32)

    stats.update({"mode": mode, "host_syncs_between_tokens": 0, "replays": 0})
    was_training = model.training
    model.eval()
    try:
        if mode == "recompute":
            seq = ids.copy()
            t_loop = _sync_clock()
            for _ in range(max_new_tokens):
                logits = model(seq)
                nxt = pick_rows(logits, seq.shape[1])
                stats["host_syncs_between_tokens"] += 1
                seq = np.concatenate([seq, nxt[:, None]], axis=1)
            stats["decode_s"] = _sync_clock() - t_loop
            return seq
        if mode not in ("cached", "graph"):
            raise ValueError(f"unknown mode {mode!r} (recompute, cached, graph)")
        if max_new_tokens == 0:
            return ids.copy()
        cache = model.new_cache(B, T0 + max_new_tokens)
        t_start = _sync_clock()
        logits = model(ids, cache=cache, last_only=True)                   # prefill
        stats["prefill_s"] = _sync_clock() - t_start
        if mode == "cached":
            seq = ids.copy()
            t_loop = _sync_clock()
            for i in range(max_new_tokens):
                nxt = pick_rows(logits, T0 + i)
                stats["host_syncs_between_tokens"] += 1
                seq = np.concatenate([seq, nxt[:, None]], axis=1)
                if i + 1 < max_new_tokens:
                    logits = model(nxt[:, None], cache=cache)
            stats["decode_s"] = _sync_clock() - t_loop
            return seq
        # graph: the first new id comes from the prefill's logits; every later one from a replay of the captured step
        t_setup = _sync_clock()
        step = GraphedDecodeStep(model, cache, greedy=greedy, sampler=(top_k, temperature, seed0) if device_draw else None)
        stats["kernel_nodes"], stats["graph_nodes"] = step.kernel_nodes, step.graph_nodes
        out = torch.empty((B, max_new_tokens), dtype=torch.int32, device="cuda")
        t_loop = _sync_clock()
        stats["capture_s"] = t_loop - t_setup
        try:
            if greedy or device_draw:
                if greedy:
                    call_hip_function("nnhipArgmaxF32", step.ids_buf, logits.data[:, -1].contiguous(), B, model.vocab_size, 1,
                                      get_current_stream_ptr())
                else:
                    draw(logits, T0, out=step.ids_buf)                     # the first new token: from the prefill's logits
                out[:, 0:1].copy_(step.ids_buf)                            # stream-ordered device copies: no host involvement
                for i in range(1, max_new_tokens):
                    step.replay()
                    out[:, i:i + 1].copy_(step.ids_buf)
                new = out.cpu().numpy()                                    # the one synchronisation, at the end
            else:
                new = np.empty((B, max_new_tokens), dtype=np.int32)
                last = logits.data[:, -1].cpu().numpy()
                for i in range(max_new_tokens):
                    stats["host_syncs_between_tokens"] += 1
                    new[:, i] = [_pick(last[b], temperature, top_k, rng) for b in range(B)]
                    if i + 1 < max_new_tokens:
                        step.ids_buf.copy_(torch.from_numpy(new[:, i:i + 1].copy()))
                        step.replay()
                        last = step.logits[:, 0].cpu().numpy()
            stats["replays"] = step.replays
            stats["decode_s"] = _sync_clock() - t_loop
        finally:
            step.release()
        return np.concatenate([ids, new], axis=1)
    finally:
        model.train(was_training)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default=None, help="local pytorch_model.bin or model.safetensors")
    ap.add_argument("--random", action="store_true", help="GPT-2-small-shaped random weights")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ids", default=None, help="comma-separated prompt token ids")
    ap.add_argument("--prompt", default=None, help="text prompt (needs the tokenizers package and --tokenizer)")
    ap.add_argument("--tokenizer", default=None, help="local tokenizer.json")
    ap.add_argument("--prompt-len", type=int, default=16, help="random prompt length when neither --ids nor --prompt is given")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--max-new-tokens", type=int, default=50)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0, help="0 = greedy; the reference script's default is 40: pass --top-k 40, with "
                    "--sampler device to keep the graph mode free of host synchronisations (tokens then differ from --sampler host: "
                    "another random stream)")
    ap.add_argument("--sampler", default="host", choices=["host", "device"], help="who draws when --top-k > 0: NumPy on a host copy of "
                    "the logits (one synchronisation per token), or nnhipSampleTopK on the device")
    ap.add_argument("--mode", default="graph", choices=["recompute", "cached", "graph"])
    ap.add_argument("--linear", default="gemm", choices=["gemm", "gemv"], help="cached / graph: gemv streams the weights of every Linear "
                    "forward of 1..8 rows through the GEMV kernel (one launch, no split-K reduce; logits move in their last bits)")
    return ap


def main():
    ap = build_parser()
    a = ap.parse_args()
    if not a.random and not a.weights:
        ap.error("give --weights PATH or --random")
    import torch
    neunet_hip.load_library()
    np.random.seed(a.seed)
    cfg = dict(GPT2_SMALL)
    model = GPT2(cfg)
    load_gpt2_weights(model, random_gpt2_state(cfg, a.seed) if a.random else load_state_dict_file(a.weights))
    tok = None
    if a.prompt is not None:
        try:
            from tokenizers import Tokenizer
        except Exception as exc:  # noqa: BLE001
            raise SystemExit(f"--prompt needs the tokenizers package ({exc}); pass token ids with --ids") from exc
        if not a.tokenizer or not os.path.exists(a.tokenizer):
            raise SystemExit("--prompt needs --tokenizer /path/to/tokenizer.json (nothing is downloaded)")
        tok = Tokenizer.from_file(a.tokenizer)
        ids = np.array([tok.encode(a.prompt).ids] * a.batch, dtype=np.int32)
    elif a.ids:
        ids = np.array([[int(t) for t in a.ids.split(",")]] * a.batch, dtype=np.int32)
    else:
        ids = np.random.default_rng(a.seed).integers(0, cfg["vocab_size"], (a.batch, a.prompt_len)).astype(np.int32)
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = generate(model, ids, a.max_new_tokens, a.temperature, a.top_k, a.mode, seed=a.seed, stats=stats, sampler=a.sampler,
                   linear=a.linear)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for row in out:
        print(tok.decode(row.tolist()) if tok is not None else ",".join(str(int(t)) for t in row))
    print(f"mode: {a.mode}  stats: {stats}")
    print(f"tokens_per_sec: {a.batch * a.max_new_tokens / dt:.2f} end to end (prefill and, in graph mode, warm-up + capture included); "
          f"{a.batch * a.max_new_tokens / stats['decode_s']:.2f} in the token loop alone")


if __name__ == "__main__":
    main()
