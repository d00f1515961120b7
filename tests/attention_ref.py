"""NumPy restatement of the attention core of examples/gpt.ipynb cell 2 (oracle.neunet_oracle.MHA without the projections), forward and
backward, per head, in any float type: the yardstick for the fused kernels of csrc/attention.hip (float64 for a bound, float32 for what
the reference's own rounding costs) and the subject of tests/test_attention_ref.py, which pins it to the oracle.

    scores = q k^T / scale                       (`scale` DIVIDES: the notebook's sqrt(d_model); the C ABI takes 1 / scale and multiplies)
    visible(i, j) = key_valid[j] != 0 and (not causal or j <= i + (Tk - Tq))      -- or dense[i, j] != 0, which replaces both
    scores = where(visible, scores, -1e9)        (exactly -1e9: a row without a visible key is uniform over ALL keys)
    P = softmax(scores, -1);  O = (P * drop) v   (the denominator is over the un-dropped map; drop holds 0 or 1 / (1 - p))
    dP = (dO v^T) * drop;  dS = where(visible, P (dP - sum_j dP P), 0) / scale;  dQ = dS k;  dK = dS^T q;  dV = (P * drop)^T dO

The row statistics are returned as the kernels store them: row_max_log2 = max_j scores * log2(e), log2_row_sum = log2 sum_j exp(scores -
max).  A fully masked row has row_max_log2 = -1e9 log2(e) and log2_row_sum = log2(Tk)."""
import numpy as np

MASKED = -1e9
LOG2E = 1.4426950408889634


def visible_map(Tq, Tk, key_valid=None, causal=False, dense=None):
    """[..., Tq, Tk] bool.  key_valid [..., Tk]; dense [..., Tq, Tk] replaces (key_valid, causal)."""
    if dense is not None:
        return np.asarray(dense) != 0
    vis = np.ones((Tq, Tk), bool)
    if causal:
        vis = np.arange(Tk)[None, :] <= np.arange(Tq)[:, None] + (Tk - Tq)
    if key_valid is not None:
        vis = vis & (np.asarray(key_valid) != 0)[..., None, :]
    return vis


def attention(q, k, v, key_valid, causal, scale, dO, dtype, drop=None, dense=None):
    """q [..., Tq, dh], k, v [..., Tk, dh], dO [..., Tq, dh] or None (forward only), key_valid [..., Tk] or None, drop / dense
    [..., Tq, Tk] or None; leading axes broadcast (a stack of heads).  Every operation runs in `dtype`.
    Returns O, row_max_log2, log2_row_sum, dQ, dK, dV (the gradients None without dO)."""
    q, k, v = (np.asarray(a, dtype) for a in (q, k, v))
    Tq, Tk = q.shape[-2], k.shape[-2]
    vis = visible_map(Tq, Tk, key_valid, causal, dense)
    kT = np.swapaxes(k, -1, -2)
    s = np.matmul(q, kT) / dtype(scale)
    s = np.where(vis, s, dtype(MASKED)).astype(dtype)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    P = e / l
    used = P if drop is None else (P * np.asarray(drop, dtype)).astype(dtype)
    O = np.matmul(used, v)
    row_max_log2 = (m[..., 0] * dtype(LOG2E)).astype(dtype)
    log2_row_sum = np.log2(l[..., 0]).astype(dtype)
    if dO is None:
        return O, row_max_log2, log2_row_sum, None, None, None
    dO = np.asarray(dO, dtype)
    dP = np.matmul(dO, np.swapaxes(v, -1, -2))
    if drop is not None:
        dP = dP * np.asarray(drop, dtype)
    dS = P * (dP - (dP * P).sum(-1, keepdims=True))
    dS = (np.where(vis, dS, dtype(0)) / dtype(scale)).astype(dtype)
    dQ = np.matmul(dS, k)
    dK = np.matmul(np.swapaxes(dS, -1, -2), q)
    dV = np.matmul(np.swapaxes(used, -1, -2), dO)
    return O, row_max_log2, log2_row_sum, dQ, dK, dV


def heads(x, H):
    """[B, T, H * dh] -> [B, H, T, dh] (a view)."""
    B, T, D = x.shape
    return x.reshape(B, T, H, D // H).transpose(0, 2, 1, 3)


def unheads(x):
    """[B, H, T, dh] -> [B, T, H * dh]."""
    B, H, T, dh = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B, T, H * dh)
