"""Float64 NumPy restatement of the seq2seq Transformer of the reference's examples/seq2seq.ipynb (cells 2-9: post-LayerNorm with
eps 0.001, ReLU feed-forward, q/k/v projections without bias, scores / sqrt(d_model), masked entries set to -1e9), of its greedy
predict() loop (cell 17) and of one cross-attention query row against a head-major memory -- for the tests, and for
tools/gen_golden.py, which asserts the fixture's greedy margins with it.

Parameters travel as a dict under the model's state_dict() names (`encoder.token_embedding.weight`, `encoder.layers.0.self_attn.wq.weight`,
..., `decoder.layers.1.cross_attn.fc.bias`, `decoder.fc_out.weight`); Linear weights are [out, in], biases [1, out]."""
import numpy as np

LN_EPS = 0.001
MASKED = -1e9


def _p(params, name):
    return np.asarray(params[name], np.float64)


def positional_table(max_len, d_model):
    """cell 6, in float64."""
    pe = np.zeros((max_len, d_model))
    position = np.arange(max_len, dtype=np.float64)[:, None]
    div = np.exp(np.arange(0, d_model, 2, dtype=np.float64) * (-np.log(10000.0) / d_model))
    pe[:, 0::2] = np.sin(position * div)
    pe[:, 1::2] = np.cos(position * div)
    return pe


def layernorm(x, w, b, eps=LN_EPS):
    mean = x.mean(-1, keepdims=True)
    var = x.var(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * w + b


def softmax(s):
    s = s - s.max(-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(-1, keepdims=True)


def mha(params, pre, q_in, kv_in, mask, n_heads):
    """cell 2.  mask: bool, broadcastable to [B, 1, Tq, Tk] (True = visible) or None.  Returns (out, attn [B, H, Tq, Tk])."""
    B, Tq, D = q_in.shape
    Tk = kv_in.shape[1]
    dh = D // n_heads
    split = lambda x, T: x.reshape(B, T, n_heads, dh).transpose(0, 2, 1, 3)  # noqa: E731
    q = split(q_in @ _p(params, pre + "wq.weight").T, Tq)
    k = split(kv_in @ _p(params, pre + "wk.weight").T, Tk)
    v = split(kv_in @ _p(params, pre + "wv.weight").T, Tk)
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(D)
    if mask is not None:
        s = np.where(mask, s, MASKED)
    attn = softmax(s)
    ctx = (attn @ v).transpose(0, 2, 1, 3).reshape(B, Tq, D)
    return ctx @ _p(params, pre + "fc.weight").T + _p(params, pre + "fc.bias").reshape(-1), attn


def ffn(params, pre, x):
    h = np.maximum(x @ _p(params, pre + "fc_1.weight").T + _p(params, pre + "fc_1.bias").reshape(-1), 0.0)
    return h @ _p(params, pre + "fc_2.weight").T + _p(params, pre + "fc_2.bias").reshape(-1)


def _n_layers(params, side):
    return 1 + max(int(k.split(".")[2]) for k in params if k.startswith(side + ".layers."))


def _embed(params, side, ids):
    W = _p(params, side + ".token_embedding.weight")
    D = W.shape[1]
    return W[ids] * np.sqrt(D) + positional_table(ids.shape[1], D)[None]


def encoder_forward(params, src, n_heads, pad_idx=0):
    """src int [B, S] -> (enc [B, S, D], src_valid bool [B, S])."""
    src = np.asarray(src)
    valid = src != pad_idx
    mask = valid[:, None, None, :]
    x = _embed(params, "encoder", src)
    for i in range(_n_layers(params, "encoder")):
        pre = f"encoder.layers.{i}."
        y, _ = mha(params, pre + "self_attn.", x, x, mask, n_heads)
        x = layernorm(x + y, _p(params, pre + "norm1.weight"), _p(params, pre + "norm1.bias"))
        x = layernorm(x + ffn(params, pre + "ffn.", x), _p(params, pre + "norm2.weight"), _p(params, pre + "norm2.bias"))
    return x, valid


def decoder_forward(params, tgt, enc, src_valid, n_heads, pad_idx=0):
    """tgt int [B, T] -> (logits [B, T, V], the last layer's cross-attention map [B, H, T, S])."""
    tgt = np.asarray(tgt)
    T = tgt.shape[1]
    tgt_mask = (tgt != pad_idx)[:, None, None, :] & np.tril(np.ones((T, T), bool))[None, None]
    src_mask = src_valid[:, None, None, :]
    x = _embed(params, "decoder", tgt)
    attn = None
    for i in range(_n_layers(params, "decoder")):
        pre = f"decoder.layers.{i}."
        y, _ = mha(params, pre + "self_attn.", x, x, tgt_mask, n_heads)
        x = layernorm(x + y, _p(params, pre + "norm1.weight"), _p(params, pre + "norm1.bias"))
        y, attn = mha(params, pre + "cross_attn.", x, enc, src_mask, n_heads)
        x = layernorm(x + y, _p(params, pre + "norm2.weight"), _p(params, pre + "norm2.bias"))
        x = layernorm(x + ffn(params, pre + "ffn.", x), _p(params, pre + "norm3.weight"), _p(params, pre + "norm3.bias"))
    return x @ _p(params, "decoder.fc_out.weight").T + _p(params, "decoder.fc_out.bias").reshape(-1), attn


def seq2seq_forward(params, src, tgt, n_heads, pad_idx=0):
    enc, valid = encoder_forward(params, src, n_heads, pad_idx)
    return decoder_forward(params, tgt, enc, valid, n_heads, pad_idx)


def greedy(params, src_ids, n_heads, max_length=50, sos_idx=1, eos_idx=2, pad_idx=0):
    """cell 17's loop for one sentence.  Returns (tokens incl. SOS, step logits [len(tokens) - 1, V], the last step's map)."""
    src = np.asarray(src_ids).reshape(1, -1)
    enc, valid = encoder_forward(params, src, n_heads, pad_idx)
    tokens, steps, attn = [sos_idx], [], None
    for _ in range(max_length):
        logits, attn = decoder_forward(params, np.asarray(tokens).reshape(1, -1), enc, valid, n_heads, pad_idx)
        steps.append(logits[0, -1])
        tokens.append(int(np.argmax(logits[0, -1])))
        if tokens[-1] == eos_idx or len(tokens) >= max_length:
            break
    return tokens, np.stack(steps), attn


def teacher_forced_logits(params, src_ids, tokens, n_heads, pad_idx=0):
    """Step logits for a GIVEN token list (tokens[0] = SOS): row t predicts tokens[t + 1].  [len(tokens) - 1, V].  Causality makes
    one full pass over tokens[:-1] equal to the loop's per-prefix passes."""
    src = np.asarray(src_ids).reshape(1, -1)
    enc, valid = encoder_forward(params, src, n_heads, pad_idx)
    logits, _ = decoder_forward(params, np.asarray(tokens[:-1]).reshape(1, -1), enc, valid, n_heads, pad_idx)
    return logits[0]


def greedy_margins(step_logits):
    """Per step: (top-1 minus top-2) / max|logit| -- the fixture's condition is >= 1e-3 at every step."""
    L = np.asarray(step_logits, np.float64)
    top = np.sort(L, axis=-1)
    return (top[:, -1] - top[:, -2]) / np.abs(L).max(axis=-1)


def cross_decode_ref(Q, Kmem, Vmem, key_valid, scale):
    """Q [B, D]; Kmem, Vmem [B, H, S, dh]; key_valid int [B, S] or None -> (O [B, D], P [B, H, S]): the rule of
    nnhipAttentionDecodeCross (a masked key scores -1e9, so a fully masked row is the plain mean of V)."""
    Q, Kmem, Vmem = (np.asarray(a, np.float64) for a in (Q, Kmem, Vmem))
    B, H, S, dh = Kmem.shape
    q = Q.reshape(B, H, dh)
    s = np.einsum("bhd,bhsd->bhs", q, Kmem) * scale
    if key_valid is not None:
        s = np.where(np.asarray(key_valid)[:, None, :] != 0, s, MASKED)
    P = softmax(s)
    return np.einsum("bhs,bhsd->bhd", P, Vmem).reshape(B, H * dh), P


def adam_first_steps(p, g, lr, betas=(0.9, 0.98), eps=1e-9, steps=1):
    """A float64 Adam from zero moments (neunet/optim.py's update without weight decay): the parameter after `steps` steps on a
    constant gradient."""
    p, g = np.asarray(p, np.float64).copy(), np.asarray(g, np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, steps + 1):
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        p -= lr * (m / (1 - betas[0] ** t)) / (np.sqrt(v / (1 - betas[1] ** t)) + eps)
    return p
