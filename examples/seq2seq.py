"""Seq2seq Transformer on the HIP path -- user-level model code with the module graph of the reference's examples/seq2seq.ipynb
(cells 2-9): an encoder-decoder Transformer, post-LayerNorm (eps 0.001), ReLU feed-forward, Q/K/V projections without bias,
Embedding * sqrt(d) + sinusoidal PE, CrossEntropy(ignore_index=PAD), Adam(lr 3e-4, betas (0.9, 0.98), eps 1e-9).  Same attribute
names and creation order as the notebook, so a checkpoint written by the reference loads with load_state_dict and state_dict()
lists the same keys in the same order.

    python examples/seq2seq.py --config tiny --task reverse --steps 200 --mode graph

Masks.  The notebook's src_mask (get_pad_mask(src), [B, 1, S]) is carried as key_valid = (src != PAD) with causal=False; its
tgt_mask (get_pad_mask(tgt) & get_sub_mask(tgt)) as (key_valid of the target, causal=True).  Training never looks at the attention
map and runs the fused flash-style kernels (need_weights=False); forward(..., need_weights=True) materialises the map of the LAST
decoder layer's cross-attention, the one the notebook returns and plots.

translate(model, src_ids, max_length=50, mode=...) is greedy with the notebook's stop rule (cell 17: EOS, or max_length tokens with
the leading SOS counted) and returns the raw token lists, SOS and EOS included:
  recompute  the notebook's predict() loop: the whole decoder over the prefix for every token
  cached     encode once, project the encoder output into a CrossAttentionMemory once, then one single-row decoder step per token:
             self-attention on a KVCache (nnhipAttentionDecode), cross-attention on the memory (nnhipAttentionDecodeCross)
  graph      that step captured into a hipGraph once and replayed; nnhipArgmaxF32 writes the next id into the buffer the next
             replay reads and the positional row is gathered by cache_len, so the host synchronises once per call and trims every
             row at its first EOS
Several sentences go in as one right-padded batch (PAD + key_valid); all rows start at SOS and advance in lockstep.  (A PAD id
chosen by the argmax would be masked as a key by the recompute loop, as in the notebook, and not by the cached steps; a model that
has learnt anything never emits PAD.)
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "numpy-nn-model_amd"))
import neunet_hip  # noqa: E402,F401
import neunet_hip.nn as nn  # noqa: E402
from neunet_hip import Tensor  # noqa: E402
from neunet_hip.nn.experimental.embedding import hip_embedding_forward  # noqa: E402
from neunet_hip.nn.experimental.linear import hip_linear_module_forward  # noqa: E402
from neunet_hip.nn.experimental.utils import call_hip_function, get_current_stream_ptr  # noqa: E402

PAD, SOS, EOS = 0, 1, 2
CONFIGS = {"tiny": dict(vocab=40, d_model=64, n_heads=2, d_ff=96, n_layers=2),
           "notebook": dict(vocab=15000, d_model=256, n_heads=8, d_ff=512, n_layers=3)}      # cell 13
LN_EPS = 0.001


def _nograd(array):
    return Tensor._wrap(array, None, "seq2seq_step", "cuda", requires_grad=False)


class PositionwiseFeedForward(nn.Module):
    def __init__(self, d_model, d_ff, dropout=0.1):
        super().__init__()
        self.fc_1 = nn.Linear(d_model, d_ff)
        self.fc_2 = nn.Linear(d_ff, d_model)
        self.dropout = nn.Dropout(dropout)
        self.activation = nn.ReLU()

    def forward(self, x, residual=None):
        x = self.dropout(self.activation(self.fc_1(x)))
        return self.fc_2(x) if residual is None else self.fc_2(x, residual=residual)


def _sublayer(module_dropout, norm, x, call):
    """norm(x + dropout(sublayer(x))): with dropout off the add rides in the sublayer's last GEMM (residual=x)."""
    if module_dropout.p == 0 or not module_dropout.training:
        y, extra = call(x)
        return norm(y), extra
    y, extra = call(None)
    return norm(x + module_dropout(y)), extra


class EncoderLayer(nn.Module):
    def __init__(self, d_model, n_heads, d_ff, dropout=0.1):
        super().__init__()
        self.self_attn = nn.MultiHeadAttention(d_model, n_heads, dropout, bias=False)
        self.ffn = PositionwiseFeedForward(d_model, d_ff, dropout)
        self.norm1 = nn.LayerNorm(d_model, eps=LN_EPS)
        self.norm2 = nn.LayerNorm(d_model, eps=LN_EPS)
        self.dropout = nn.Dropout(dropout)

    def forward(self, src, src_valid=None):
        src, _ = _sublayer(self.dropout, self.norm1, src,
                           lambda r: self.self_attn(src, src, src, src_valid, causal=False, need_weights=False, residual=r))
        src, _ = _sublayer(self.dropout, self.norm2, src, lambda r: (self.ffn(src, residual=r), None))
        return src


class DecoderLayer(nn.Module):
    def __init__(self, d_model, n_heads, d_ff, dropout=0.1):
        super().__init__()
        self.self_attn = nn.MultiHeadAttention(d_model, n_heads, dropout, bias=False)
        self.cross_attn = nn.MultiHeadAttention(d_model, n_heads, dropout, bias=False)
        self.ffn = PositionwiseFeedForward(d_model, d_ff, dropout)
        self.norm1 = nn.LayerNorm(d_model, eps=LN_EPS)
        self.norm2 = nn.LayerNorm(d_model, eps=LN_EPS)
        self.norm3 = nn.LayerNorm(d_model, eps=LN_EPS)
        self.dropout = nn.Dropout(dropout)

    def forward(self, tgt, tgt_valid, src, src_valid, need_weights=False):
        tgt, _ = _sublayer(self.dropout, self.norm1, tgt,
                           lambda r: self.self_attn(tgt, tgt, tgt, tgt_valid, causal=True, need_weights=False, residual=r))
        tgt, attn = _sublayer(self.dropout, self.norm2, tgt,
                              lambda r: self.cross_attn(tgt, src, src, src_valid, causal=False, need_weights=need_weights, residual=r))
        tgt, _ = _sublayer(self.dropout, self.norm3, tgt, lambda r: (self.ffn(tgt, residual=r), None))
        return tgt, attn

    def step(self, x, cache, memory, need_weights=False):
        """One cached step (no tape): x is the device array [B, 1, D] of the new row; cache / memory are this layer's KVCacheLayer
        and CrossAttentionMemoryLayer.  Returns (x, attn): attn is None or the cross-attention map [B, H, 1, S]."""
        x = self.norm1(_nograd(self.self_attn.self_step(x, cache, residual=x)))
        y, attn = self.cross_attn.cross_step(x, memory, residual=x, need_weights=need_weights)
        x = self.norm2(_nograd(y))
        x = self.norm3(self.ffn(x, residual=x))
        return x.data, attn


class Encoder(nn.Module):
    def __init__(self, src_vocab_size, d_model, n_heads, d_ff, n_layers, dropout=0.1, max_len=5000):
        super().__init__()
        self.token_embedding = nn.Embedding(src_vocab_size, d_model)
        self.position_embedding = nn.PositionalEncoding(d_model, max_len)
        self.layers = nn.ModuleList([EncoderLayer(d_model, n_heads, d_ff, dropout) for _ in range(n_layers)])
        self.dropout = nn.Dropout(dropout)
        self.scale = math.sqrt(d_model)

    def forward(self, src, src_valid=None):
        # emb * sqrt(d) + pe[:, :S] fused into the gather
        src = self.dropout(self.token_embedding(src, scale=self.scale, pe=self.position_embedding.table))
        for layer in self.layers:
            src = layer(src, src_valid)
        return src


class Decoder(nn.Module):
    def __init__(self, tgt_vocab_size, d_model, n_heads, d_ff, n_layers, dropout=0.1, max_len=5000):
        super().__init__()
        self.token_embedding = nn.Embedding(tgt_vocab_size, d_model)
        self.position_embedding = nn.PositionalEncoding(d_model, max_len)
        self.layers = nn.ModuleList([DecoderLayer(d_model, n_heads, d_ff, dropout) for _ in range(n_layers)])
        self.fc_out = nn.Linear(d_model, tgt_vocab_size)
        self.dropout = nn.Dropout(dropout)
        self.scale = math.sqrt(d_model)

    def forward(self, tgt, tgt_valid, src, src_valid, need_weights=False):
        tgt = self.dropout(self.token_embedding(tgt, scale=self.scale, pe=self.position_embedding.table))
        attn = None
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            tgt, attn = layer(tgt, tgt_valid, src, src_valid, need_weights=need_weights and i == last)
        return self.fc_out(tgt), attn

    # ---- cached decoding (no tape) ----------------------------------------------------------------------------------------------
    def fill_memory(self, enc_src, src_valid):
        """The encoder output [B, S, D] projected by every layer's cross-attention (one K|V GEMM + one copy each)."""
        layer0 = self.layers[0].cross_attn
        B, S, _ = enc_src.shape
        mem = nn.CrossAttentionMemory(B, S, len(self.layers), layer0.n_heads, layer0.depth, key_valid=src_valid)
        for i, layer in enumerate(self.layers):
            layer.cross_attn.fill_memory(enc_src, mem.layer(i))
        return mem

    def new_cache(self, B, Tmax):
        a = self.layers[0].self_attn
        return nn.KVCache(B, Tmax, len(self.layers), a.n_heads, a.depth)

    def embed_step(self, ids_buf, cache, tok, pos):
        """tok [B, 1, D] = embedding(ids_buf) * sqrt(d) + pe[cache_len[b]]: the positional row is gathered by the DEVICE-side
        position, so the same launches serve every step of a captured graph."""
        hip_embedding_forward(tok, self.token_embedding.weight.data, ids_buf, None, 1, self.scale)
        hip_embedding_forward(pos, self.position_embedding.table, cache.cache_len, None, 1, 1.0)
        call_hip_function("nnhipAdd", tok, tok, pos, tok.numel(), get_current_stream_ptr())
        return tok

    def step(self, ids_buf, cache, memory, tok, pos, logits, need_weights=False):
        """One cached decoder step for the ids in ids_buf (int32 device [B, 1]) at position cache_len: logits [B, 1, V] is written,
        the cache advanced.  Returns the last layer's cross-attention map when asked."""
        x = self.embed_step(ids_buf, cache, tok, pos)
        attn, last = None, len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            x, attn = layer.step(x, cache.layer(i), memory.layer(i), need_weights=need_weights and i == last)
        B, D = x.shape[0], x.shape[-1]
        hip_linear_module_forward(x, self.fc_out.weight.data, self.fc_out.bias.data, logits, B, D, self.fc_out.out_features)
        cache.advance(1)
        return attn


def key_valid_of(ids, pad_idx):
    """ids: int32 device array [B, T] -> int32 device array [B, T], 1 where ids != pad_idx (the notebook's get_pad_mask)."""
    import torch
    out = torch.empty_like(ids)
    call_hip_function("nnhipNotEqualInt32", out, ids, ids.numel(), int(pad_idx), get_current_stream_ptr())
    return out


def device_ids(x):
    """Host int array (or Tensor) [B, T] -> a contiguous int32 device array."""
    import torch
    if isinstance(x, Tensor):
        x = x.data
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.int32))
    return x.to(device="cuda", dtype=torch.int32).contiguous()


class Seq2SeqTransformer(nn.Module):
    def __init__(self, encoder, decoder, pad_idx):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.pad_idx = pad_idx

    def encode(self, src):
        """src: int ids [B, S] -> (encoder output Tensor [B, S, D], key_valid of the source)."""
        ids = device_ids(src)
        valid = key_valid_of(ids, self.pad_idx)
        return self.encoder(Tensor._wrap(ids, None, "ids", "cuda", requires_grad=False), valid), valid

    def decode(self, tgt, enc_src, src_valid, need_weights=False):
        ids = device_ids(tgt)
        return self.decoder(Tensor._wrap(ids, None, "ids", "cuda", requires_grad=False), key_valid_of(ids, self.pad_idx), enc_src,
                            src_valid, need_weights=need_weights)

    def forward(self, src, tgt, need_weights=False):
        """src [B, S], tgt [B, T] host int arrays -> (logits [B, T, V], attention): attention is None, or with need_weights the
        last decoder layer's cross-attention map [B, H, T, S] (what the notebook's forward returns)."""
        enc_src, src_valid = self.encode(src)
        return self.decode(tgt, enc_src, src_valid, need_weights=need_weights)


def build_seq2seq(vocab=15000, d_model=256, n_heads=8, d_ff=512, n_layers=3, dropout=0.1, pad_idx=PAD, max_len=5000, tgt_vocab=None):
    enc = Encoder(vocab, d_model, n_heads, d_ff, n_layers, dropout, max_len)
    dec = Decoder(tgt_vocab or vocab, d_model, n_heads, d_ff, n_layers, dropout, max_len)
    return Seq2SeqTransformer(enc, dec, pad_idx)


def train_step(model, optimizer, loss_fn, src, tgt):
    """cell 14's loop body: forward on (src, tgt[:, :-1]), CE against tgt[:, 1:], backward, step, zero_grad."""
    output, _ = model.forward(src, tgt[:, :-1])
    output = output.reshape(output.shape[0] * output.shape[1], output.shape[2])
    targets = Tensor(np.ascontiguousarray(tgt[:, 1:]).reshape(-1), dtype=np.int32, requires_grad=False, device="cuda")
    loss = loss_fn(output, targets)
    loss.backward()
    optimizer.step()
    optimizer.zero_grad()
    return loss


# ---- host-side pieces (no device needed) -----------------------------------------------------------------------------------------
def pad_batch(seqs, pad_idx=PAD):
    """Lists of ids -> one right-padded int32 array [B, longest]."""
    seqs = [list(map(int, s)) for s in seqs]
    if not seqs or min(len(s) for s in seqs) < 1:
        raise ValueError("every sentence needs at least one token")
    out = np.full((len(seqs), max(len(s) for s in seqs)), pad_idx, dtype=np.int32)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out


def trim_at_eos(row, eos_idx=EOS):
    """The tokens up to and including the first EOS (the notebook's loop stops there); the whole row if there is none."""
    row = [int(t) for t in row]
    return row[:row.index(eos_idx) + 1] if eos_idx in row else row


def reverse_batches(vocab, batch, steps, seed=0, min_len=3, max_len=12):
    """The toy task: target = the source reversed.  Yields (src, tgt) int32 arrays, each row SOS + tokens + EOS, right-padded with
    PAD; tokens are drawn from 3 .. vocab-1 with random lengths, everything from `seed`."""
    if vocab < 4:
        raise ValueError("the reverse task needs a vocabulary of at least 4 ids (PAD, SOS, EOS and one token)")
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        srcs, tgts = [], []
        for n in rng.integers(min_len, max_len + 1, batch):
            toks = rng.integers(3, vocab, int(n)).tolist()
            srcs.append([SOS] + toks + [EOS])
            tgts.append([SOS] + toks[::-1] + [EOS])
        yield pad_batch(srcs), pad_batch(tgts)


# ---- translation ---------------------------------------------------------------------------------------------------------------------
class _GraphStep:
    """One cached decoder step captured into a hipGraph (as examples/gpt2_infer.py's GraphedDecodeStep): ids_buf -> embedding with
    the positional row gathered by cache_len -> the layers on the KV cache and the encoder memory -> fc_out -> argmax -> ids_buf;
    cache_len += 1.  One stream, no parallel branches."""

    def __init__(self, decoder, cache, memory, ids_buf, tok, pos, logits):
        import torch
        from neunet_hip.graph import count_graph_nodes
        self.cache = cache

        def step():
            decoder.step(ids_buf, cache, memory, tok, pos, logits)
            call_hip_function("nnhipArgmaxF32", ids_buf, logits, cache.B, logits.shape[-1], 1, get_current_stream_ptr())

        # warm-up on a side stream (grows the library workspace), then put back what it changed: lengths and the start ids
        saved_len, saved_tokens, saved_ids = cache.cache_len.clone(), cache.tokens, ids_buf.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        cache.cache_len.copy_(saved_len)
        ids_buf.copy_(saved_ids)
        cache.tokens = saved_tokens
        self.graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            step()
        cache.tokens = saved_tokens                      # the capture ran the host bookkeeping of one step without executing it
        self.kernel_nodes, self.graph_nodes = count_graph_nodes(self.graph.raw_cuda_graph())
        self.graph.instantiate()
        call_hip_function("nnhipWorkspaceLock", 1)       # the graph holds library-owned addresses: nothing may move them
        self._locked = True

    def replay(self):
        self.cache.replayed(1)
        self.graph.replay()

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
    import torch
    torch.cuda.synchronize()
    return time.perf_counter()


def translate(model, src_ids, max_length=50, mode="cached", sos_idx=SOS, eos_idx=EOS, stats=None, need_weights=False):
    """src_ids: one sentence (a flat list of ids) or several (a list of lists, padded here).  Returns the raw greedy token list(s):
    SOS first, the first EOS last if one was produced, at most max_length tokens.  stats (a dict, optional) receives mode,
    host_syncs_between_tokens, encode_s / decode_s and, in graph mode, kernel_nodes / graph_nodes / capture_s.  need_weights
    (recompute and cached): stats["attention"] holds the last layer's cross-attention map of the last step, as the notebook's
    predict() returns it -- [B, H, T, S] in recompute mode, [B, H, 1, S] in cached mode."""
    import torch
    if max_length < 2:
        raise ValueError("max_length counts the leading SOS: it must be at least 2")
    if mode not in ("recompute", "cached", "graph"):
        raise ValueError(f"unknown mode {mode!r} (recompute, cached, graph)")
    if need_weights and mode == "graph":
        raise ValueError("need_weights is for the recompute and cached modes")
    single = len(src_ids) > 0 and np.ndim(src_ids[0]) == 0
    src = pad_batch([src_ids] if single else src_ids, model.pad_idx)
    B = src.shape[0]
    stats = stats if stats is not None else {}
    stats.update({"mode": mode, "host_syncs_between_tokens": 0})
    was_training = model.training
    model.eval()
    try:
        t0 = _sync_clock()
        enc_src, src_valid = model.encode(src)
        dec = model.decoder
        rows = np.full((B, 1), sos_idx, dtype=np.int32)
        done = np.zeros(B, bool)
        if mode == "recompute":
            t1 = _sync_clock()
            stats["encode_s"] = t1 - t0
            nxt_buf = torch.empty((B, 1), dtype=torch.int32, device="cuda")
            for _ in range(max_length):
                logits, attn = model.decode(rows, enc_src, src_valid, need_weights=need_weights)
                call_hip_function("nnhipArgmaxF32", nxt_buf, logits.data[:, -1].contiguous(), B, logits.shape[-1], 1,
                                  get_current_stream_ptr())
                nxt = nxt_buf.cpu().numpy()[:, 0]
                stats["host_syncs_between_tokens"] += 1
                rows = np.concatenate([rows, nxt[:, None]], axis=1)
                done |= nxt == eos_idx
                if done.all() or rows.shape[1] >= max_length:
                    break
            if need_weights:
                stats["attention"] = attn.cpu().numpy()
            stats["decode_s"] = _sync_clock() - t1
        else:
            V, D = dec.fc_out.out_features, dec.fc_out.in_features
            memory = dec.fill_memory(enc_src.data, src_valid)
            cache = dec.new_cache(B, max_length)
            ids_buf = torch.full((B, 1), sos_idx, dtype=torch.int32, device="cuda")
            tok = torch.empty((B, 1, D), dtype=torch.float32, device="cuda")
            pos = torch.empty((B, 1, D), dtype=torch.float32, device="cuda")
            logits = torch.empty((B, 1, V), dtype=torch.float32, device="cuda")
            t1 = _sync_clock()
            stats["encode_s"] = t1 - t0
            if mode == "cached":
                for _ in range(max_length):
                    attn = dec.step(ids_buf, cache, memory, tok, pos, logits, need_weights=need_weights)
                    call_hip_function("nnhipArgmaxF32", ids_buf, logits, B, V, 1, get_current_stream_ptr())
                    nxt = ids_buf.cpu().numpy()[:, 0]
                    stats["host_syncs_between_tokens"] += 1
                    rows = np.concatenate([rows, nxt[:, None]], axis=1)
                    done |= nxt == eos_idx
                    if done.all() or rows.shape[1] >= max_length:
                        break
                if need_weights:
                    stats["attention"] = attn.cpu().numpy()
                stats["decode_s"] = _sync_clock() - t1
            else:
                step = _GraphStep(dec, cache, memory, ids_buf, tok, pos, logits)
                stats["kernel_nodes"], stats["graph_nodes"] = step.kernel_nodes, step.graph_nodes
                out = torch.empty((B, max_length - 1), dtype=torch.int32, device="cuda")
                t2 = _sync_clock()
                stats["capture_s"] = t2 - t1
                try:
                    for i in range(max_length - 1):
                        step.replay()
                        out[:, i:i + 1].copy_(ids_buf)                 # stream-ordered device copy: no host involvement
                    rows = np.concatenate([rows, out.cpu().numpy()], axis=1)     # the one synchronisation of the call
                    stats["decode_s"] = _sync_clock() - t2
                finally:
                    step.release()
        result = [trim_at_eos(r, eos_idx) for r in rows]
        return result[0] if single else result
    finally:
        model.train(was_training)


def build_parser():
    ap = argparse.ArgumentParser(description="Train the notebook's seq2seq Transformer on a toy task and translate (HIP backend).")
    ap.add_argument("--config", default="tiny", choices=sorted(CONFIGS))
    ap.add_argument("--task", default="reverse", choices=["reverse"], help="target = the source reversed; generated from --seed")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--vocab", type=int, default=None, help="override the configuration's vocabulary size")
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--mode", default="graph", choices=["recompute", "cached", "graph"], help="how the translation after training decodes")
    ap.add_argument("--max-length", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    return ap


def main():
    from neunet_hip.optim import Adam
    a = build_parser().parse_args()
    cfg = dict(CONFIGS[a.config])
    if a.vocab is not None:
        cfg["vocab"] = a.vocab
    np.random.seed(a.seed)
    model = build_seq2seq(dropout=a.dropout, max_len=max(64, a.max_length + 1), **cfg)
    opt = Adam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9)
    loss_fn = nn.CrossEntropyLoss(ignore_index=PAD)
    for i, (src, tgt) in enumerate(reverse_batches(cfg["vocab"], a.batch, a.steps, seed=a.seed)):
        loss = train_step(model, opt, loss_fn, src, tgt)
        if i % 20 == 0 or i == a.steps - 1:
            print(f"step {i:4d}  loss {loss.item():.4f}", flush=True)
    src, tgt = next(reverse_batches(cfg["vocab"], 3, 1, seed=a.seed + 1))
    stats = {}
    out = translate(model, [trim_at_eos(r) for r in src], max_length=a.max_length, mode=a.mode, stats=stats)
    for s, t, o in zip(src, tgt, out):
        print("source     ", trim_at_eos(s))
        print("target     ", trim_at_eos(t))
        print("translation", o)
    print(f"mode: {a.mode}  stats: { {k: v for k, v in stats.items() if k != 'attention'} }")


if __name__ == "__main__":
    main()
