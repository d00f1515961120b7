"""Float64 restatements of the operations of csrc/rowops.hip (Softmax, masked Softmax, RMSNorm, CrossEntropy), csrc/embedding.hip
(gather, last-write-wins gradient) and csrc/elementwise.hip (ReLU, Swish, GELU, SwiGLU, the counter-hash dropout), written from the
definitions the C ABI documents (include/neunet_hip.h), NumPy only, independent of the oracle and of the kernels.
tests/test_rowops_ref.py holds them against the reference's fixtures and against the oracle; tests/test_rowops_tiers_gpu.py and
tests/test_gather_elementwise_gpu.py hold the kernels against them.

Every function takes float32 (or anything) and computes in float64, except where a float32 result is the kernel's own arithmetic and
therefore exact (ReLU, the embedding copy, the dropout hash): those say so."""
import numpy as np

U24 = 2.0 ** -24
MASKED = np.float64(np.float32(-1e9))        # what a masked score is REPLACED by (-1e9 is a float32: 2^9 * 1953125)


def _f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------- Softmax
def softmax_forward(x, axis=-1):
    """y = exp(x - max) / sum exp(x - max) along `axis`."""
    x = _f64(x)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def softmax_backward(y, dy, axis=-1):
    """dx = (dy - sum(dy y)) y along `axis`, y the forward's OUTPUT."""
    y, dy = _f64(y), _f64(dy)
    return (dy - (dy * y).sum(axis=axis, keepdims=True)) * y


def masked_positions(B, H, Tq, Tk, key_valid=None, dense=None, causal=False):
    """[B, H, Tq, Tk] bool, True = masked: key j of batch b is padding (key_valid[b, j] == 0), the dense mask says so
    (dense[b, i, j] == 0, the same for every head), or -- causal -- j > i + (Tk - Tq): the LAST query sees every key, whatever Tq."""
    m = np.zeros((B, H, Tq, Tk), bool)
    if key_valid is not None:
        m |= (np.asarray(key_valid).reshape(B, 1, 1, Tk) == 0)
    if dense is not None:
        m |= (np.asarray(dense).reshape(B, 1, Tq, Tk) == 0)
    if causal:
        i, j = np.arange(Tq)[:, None], np.arange(Tk)[None, :]
        m |= (j > i + (Tk - Tq))[None, None]
    return m


def masked_softmax_forward(S, key_valid=None, dense=None, scale=1.0, causal=False):
    """y = softmax_j(masked ? -1e9 : scale S).  A masked score is REPLACED (not -inf): a row with every position masked is uniform,
    1 / Tk each, and a masked position of a row with a visible one underflows to exactly 0."""
    S = _f64(S)
    m = masked_positions(*S.shape, key_valid, dense, causal)
    return softmax_forward(np.where(m, MASKED, S * np.float64(np.float32(scale))), -1)


def masked_softmax_backward(Y, dY, key_valid=None, dense=None, scale=1.0, causal=False):
    """dS = masked ? 0 : scale (dY - sum_j dY Y) Y: the where() passes no gradient to the replaced scores."""
    Y = _f64(Y)
    m = masked_positions(*Y.shape, key_valid, dense, causal)
    return np.where(m, 0.0, softmax_backward(Y, dY, -1) * np.float64(np.float32(scale)))


# ------------------------------------------------------------------------------------------- RMSNorm
def rmsnorm_forward(X, w, b=None, eps=1e-6):
    """std = sqrt(mean(x^2) + eps) per row; X_norm = x / std; Y = X_norm w (+ b).  Returns (Y, X_norm, std [rows])."""
    X = _f64(X)
    std = np.sqrt((X * X).mean(-1) + np.float64(np.float32(eps)))
    xn = X / std[..., None]
    Y = xn * _f64(w)
    if b is not None:
        Y = Y + _f64(b)
    return Y, xn, std


def rmsnorm_backward(X, w, dY, eps=1e-6, addend=None):
    """With g = w dY: dX = g / std - x sum(g x) / (N std^3) (+ addend); dw = sum_rows dY X_norm; db = sum_rows dY."""
    X, dY = _f64(X), _f64(dY)
    _, xn, std = rmsnorm_forward(X, w, None, eps)
    std = std[..., None]
    g = _f64(w) * dY
    dX = g / std - X * (g * X).sum(-1, keepdims=True) / (X.shape[-1] * std ** 3)
    if addend is not None:
        dX = dX + _f64(addend)
    flat = lambda a: a.reshape(-1, X.shape[-1])  # noqa: E731
    return dX, flat(dY * xn).sum(0), flat(dY).sum(0)


# ------------------------------------------------------------------------------------------- CrossEntropy
def cross_entropy(logits, labels, weight=None, ignore_index=-100, reduction="mean"):
    """CrossEntropyLoss = LogSoftmax -> NLLLoss with class weights.  A row is LIVE when label != ignore_index and 0 <= label < C (the
    kernels' `valid`: an out-of-range label is inert, exactly like an ignored one, in the loss, the gradient and the denominator).
        lse_i = log sum_c exp(x_ic)                        (every row, live or not)
        loss_rows_i = live ? (lse_i - x_i[y_i]) w[y_i] : 0
        'mean': loss = sum_i loss_rows_i / denom, denom = #live (no weights) or sum over live rows of w[y_i]; 'sum': the sum;
        'none': loss is loss_rows
        dlogits_i = live ? (softmax(x_i) - onehot(y_i)) w[y_i] k : 0, k = 1 / denom for 'mean' (0 when denom == 0), else 1
    Returns (loss_rows, lse, loss, dlogits, count) with count = #live."""
    x = _f64(logits)
    rows, C = x.shape
    y = np.asarray(labels).astype(np.int64)
    live = (y != ignore_index) & (y >= 0) & (y < C)
    ys = np.where(live, y, 0)
    m = x.max(1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(1))
    wy = np.where(live, 1.0 if weight is None else _f64(weight)[ys], 0.0)
    loss_rows = np.where(live, (lse - x[np.arange(rows), ys]) * wy, 0.0)
    count = int(live.sum())
    denom = float(count) if weight is None else float(wy.sum())
    k = 1.0
    if reduction[0] == "m":
        k = 1.0 / denom if denom > 0 else 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            loss = np.float64(loss_rows.sum()) / np.float64(denom)
    elif reduction[0] == "s":
        loss = loss_rows.sum()
    else:
        loss = loss_rows
    onehot = np.zeros_like(x)
    onehot[np.arange(rows), ys] = 1.0
    d = (np.exp(x - lse[:, None]) - onehot) * (wy * k)[:, None]
    return loss_rows, lse, loss, np.where(live[:, None], d, 0.0), count


# ------------------------------------------------------------------------------------------- Embedding
def embedding_rows(ids, V):
    """Python indexing of a V-row table: id < 0 means id + V.  Returns (row, ok): ok False where the id is out of range either way."""
    ids = np.asarray(ids).astype(np.int64).reshape(-1)
    row = np.where(ids < 0, ids + V, ids)
    return row, (row >= 0) & (row < V)


def embedding_forward(W, ids, scale=1.0, pe=None, T=1, dtype=np.float64):
    """out[p] = W[ids[p]] scale + pe[p % T]: the decoder's `emb * sqrt(d_model) + pe[:, :T]`, position p counted over the flattened
    ids.  An id outside [-V, V) reads a zero row (the position term is still added).  dtype = float32 with scale == 1 and pe None
    is a row copy: exact."""
    W = np.asarray(W).astype(dtype)
    row, ok = embedding_rows(ids, W.shape[0])
    out = np.zeros((row.size, W.shape[1]), dtype)
    for p in range(row.size):                       # loop-level obvious: one output row per position
        if ok[p]:
            out[p] = W[row[p]]
        out[p] = out[p] * dtype(np.float32(scale))
        if pe is not None:
            out[p] = out[p] + np.asarray(pe).astype(dtype)[p % T]
    return out


def embedding_backward(shape, ids, g, scale=1.0, dtype=np.float64):
    """The reference's getitem backward ASSIGNS (`_grad[index] = grad`): dW[row] = scale g[p] for the LAST position p (C order)
    that addresses `row` -- whether as id or as id - V -- and 0 for rows no position addresses.  Out-of-range ids are skipped."""
    V, D = shape
    g = np.asarray(g).astype(dtype).reshape(-1, D)
    row, ok = embedding_rows(ids, V)
    dW = np.zeros((V, D), dtype)
    for p in range(row.size):
        if ok[p]:
            dW[row[p]] = g[p] * dtype(np.float32(scale))     # a later p overwrites an earlier one
    return dW


# ------------------------------------------------------------------------------------------- elementwise maps
def relu_forward(x):
    """max(x, 0) in float32: exact.  NaN stays NaN (np.maximum(0, x) propagates it, as the reference does); a zero of either sign
    gives +0 here -- NumPy's own np.maximum(0, -0.0) returns either sign depending on its SIMD path, so the sign of a zero result is
    not part of the definition and the tests compare values, not sign bits, there."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, x, np.where(np.isnan(x), x, np.float32(0))).astype(np.float32)


def relu_backward(dy, y):
    """dx = y > 0 ? dy : 0, y the activation's OUTPUT (include/neunet_hip.h), float32: exact.  (The reference writes dy * (y > 0),
    which differs only where dy is non-finite at a dead unit, and in the sign of the zero.)"""
    dy, y = np.asarray(dy, np.float32), np.asarray(y, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(y > 0, dy, np.float32(0)).astype(np.float32)


def sigmoid(x):
    x = _f64(x)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def swish(x, beta=1.0):
    """f = x sigmoid(beta x); beta is the float32 the C ABI receives."""
    x = _f64(x)
    return x * sigmoid(np.float64(np.float32(beta)) * x)


def swish_backward(x, dy, beta=1.0):
    """dx = dy (beta f + s (1 - beta f)), s = sigmoid(beta x), f = x s."""
    x, b = _f64(x), np.float64(np.float32(beta))
    s = sigmoid(b * x)
    f = x * s
    return _f64(dy) * (b * f + s * (1.0 - b * f))


GELU_K, GELU_C = np.sqrt(2.0 / np.pi), 0.044715


def gelu(x):
    """Tanh form: 0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3)."""
    x = _f64(x)
    return 0.5 * x * (1.0 + np.tanh(GELU_K * (x + GELU_C * x ** 3)))


def gelu_backward(x, dy):
    """The exact derivative of that form: 0.5 (1 + tanh u) + 0.5 x (1 - tanh^2 u) du/dx, du/dx = sqrt(2 / pi) (1 + 3 * 0.044715 x^2)."""
    x = _f64(x)
    t = np.tanh(GELU_K * (x + GELU_C * x ** 3))
    return _f64(dy) * (0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * GELU_K * (1.0 + 3.0 * GELU_C * x * x))


def swiglu(x, beta=1.0):
    """Rows are [gate (h) | up (h)]: out = swish(gate) up."""
    x = _f64(x)
    h = x.shape[-1] // 2
    return swish(x[..., :h], beta) * x[..., h:]


def swiglu_backward(x, dy, beta=1.0):
    """d gate = dy up swish'(gate), d up = dy swish(gate); returned as rows [d gate | d up]."""
    x, dy = _f64(x), _f64(dy)
    h = x.shape[-1] // 2
    gate, up = x[..., :h], x[..., h:]
    return np.concatenate([swish_backward(gate, dy * up, beta), dy * swish(gate, beta)], axis=-1)


# ------------------------------------------------------------------------------------------- dropout
def dropout_keep(seed, seed_dev, n, p):
    """The multiplier of each of n elements, float32 [n]: nnhipDropout's counter hash restated in uint32 arithmetic (every operation
    wraps modulo 2^32; `seed_dev` is the value of the optional device word, None = absent).  Element i is kept when
    hash(seed + seed_dev, i) >= floor(p 2^32) (capped at 2^32 - 1), and a kept element is multiplied by float32(1 / (1 - p));
    p == 1 keeps the hash's one top value but multiplies by 0."""
    u = np.uint32
    p = np.float32(p)
    th = float(p) * 4294967296.0
    threshold = u(int(th)) if th < 4294967295.0 else u(4294967295)
    scale = np.float32(1.0) / (np.float32(1.0) - p) if p < 1 else np.float32(0)
    with np.errstate(over="ignore"):
        sd = u((int(seed) + (0 if seed_dev is None else int(seed_dev))) & 0xFFFFFFFF) * u(0x85EBCA6B) + u(0x9E3779B9)
        i = np.arange(n, dtype=np.uint64)
        lo, hi = (i & np.uint64(0xFFFFFFFF)).astype(u), (i >> np.uint64(32)).astype(u)
        x = sd ^ (lo * u(0x9E3779B1)) ^ (hi * u(0xC2B2AE35))
        x ^= x >> u(16)
        x *= u(0x7FEB352D)
        x ^= x >> u(15)
        x *= u(0x846CA68B)
        x ^= x >> u(16)
    return np.where(x >= threshold, scale, np.float32(0)).astype(np.float32)
