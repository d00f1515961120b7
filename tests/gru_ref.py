"""Float64 NumPy restatement of the reference GRU (neunet/nn/layers/gru.py: forward :273-311, BPTT :66-110), RNN (rnn.py: forward
:151-159, BPTT :46-56) and the Bidirectional merge (bidirectional.py:89-103, backward :16-23) for the tests.  GRU params: the nine
arrays in the reference's order (W_z, W_r, W_h, W_hz, W_hr, W_hh, b_z, b_r, b_h); RNN params: (W, W_h, b); a bias may be None (zero).
X is (B, T, in).  dY_all (B, T, H) and dY_last (B, H) may each be None.

reverse=True is the reverse layer of a Bidirectional: the layer applied to X.flip(1) (bidirectional.py:56).  Its outputs, and the
dY it takes, are in STEP order (step s read X[:, T-1-s]; nothing is flipped back); the dX it returns is in the order of X.

dtype=np.float32 keeps every array and every operation (exp, tanh included) in float32: the reference's own arithmetic.  The
distance between the two modes is what the reference's rounding alone uses of an error bound."""
import numpy as np

from lstm_ref import ACT, _dact

MERGE_MODES = ("concat", "sum", "mul", "avg")


def _prep(X, params, h0, n_w, dtype, reverse):
    H = np.shape(params[n_w // 2])[0]
    p = [np.zeros(H, dtype) if a is None else np.asarray(a, dtype) for a in params]
    X = np.asarray(X, dtype)
    if reverse:
        X = X[:, ::-1]
    B = X.shape[0]
    h = np.zeros((B, H), dtype) if h0 is None else np.array(h0, dtype)
    return X, p, h, H


def gru_forward(X, params, h0=None, nl="tanh", rnl="sigmoid", dtype=np.float64, reverse=False):
    X, p, h, H = _prep(X, params, h0, 6, dtype, reverse)
    B, T, _ = X.shape
    cache = dict(X=X, p=p, nl=nl, rnl=rnl, hs=[h], pre=[], z=[], r=[], c=[], dtype=dtype, reverse=reverse)
    Y = np.zeros((B, T, H), dtype)
    one = dtype(1.0)
    for t in range(T):
        uz = X[:, t] @ p[0] + h @ p[3] + p[6]
        ur = X[:, t] @ p[1] + h @ p[4] + p[7]
        z, r = ACT[rnl](uz), ACT[rnl](ur)
        uc = X[:, t] @ p[2] + (r * h) @ p[5] + p[8]
        c = ACT[nl](uc)
        h = z * h + (one - z) * c
        cache["pre"].append((uz, ur, uc))
        cache["z"].append(z)
        cache["r"].append(r)
        cache["c"].append(c)
        cache["hs"].append(h)
        Y[:, t] = h
    return Y, cache


def _grad_seed(cache, dY_all, dY_last, dtype):
    dtype = cache["dtype"] if dtype is None else dtype
    if dtype != cache["dtype"]:
        raise ValueError("backward: dtype differs from the forward pass that made this cache")
    dY_all = None if dY_all is None else np.asarray(dY_all, dtype)
    dY_last = None if dY_last is None else np.asarray(dY_last, dtype)
    return dtype, dY_all, dY_last


def gru_backward(cache, dY_all=None, dY_last=None, dtype=None):
    dtype, dY_all, dY_last = _grad_seed(cache, dY_all, dY_last, dtype)
    X, p, nl, rnl = cache["X"], cache["p"], cache["nl"], cache["rnl"]
    B, T, _ = X.shape
    H = p[3].shape[0]
    grads = [np.zeros_like(a) for a in p]
    dX = np.zeros_like(X)
    carry = np.zeros((B, H), dtype)
    one = dtype(1.0)
    for t in reversed(range(T)):
        uz, ur, uc = cache["pre"][t]
        z, r, c, h_prev = cache["z"][t], cache["r"][t], cache["c"][t], cache["hs"][t]
        hd = carry.copy()
        if dY_all is not None:
            hd += dY_all[:, t]
        if dY_last is not None and t == T - 1:
            hd += dY_last
        dc = hd * (one - z) * _dact(nl, uc)
        tmp = dc @ p[5].T
        dr = tmp * h_prev * _dact(rnl, ur)
        dz = hd * (h_prev - c) * _dact(rnl, uz)
        d = (dz, dr, dc)
        for k in range(3):
            grads[k] += X[:, t].T @ d[k]
            grads[6 + k] += d[k].sum(0)
        grads[3] += h_prev.T @ dz
        grads[4] += h_prev.T @ dr
        grads[5] += (h_prev * r).T @ dc
        carry = dz @ p[3].T + dr @ p[4].T + tmp * r + hd * z
        dX[:, t] = dc @ p[2].T + dz @ p[0].T + dr @ p[1].T
    return (dX[:, ::-1] if cache["reverse"] else dX), grads


def rnn_forward(X, params, h0=None, nl="tanh", dtype=np.float64, reverse=False):
    X, p, h, H = _prep(X, params, h0, 2, dtype, reverse)
    B, T, _ = X.shape
    cache = dict(X=X, p=p, nl=nl, hs=[h], pre=[], dtype=dtype, reverse=reverse)
    Y = np.zeros((B, T, H), dtype)
    for t in range(T):
        u = X[:, t] @ p[0] + h @ p[1] + p[2]
        h = ACT[nl](u)
        cache["pre"].append(u)
        cache["hs"].append(h)
        Y[:, t] = h
    return Y, cache


def rnn_backward(cache, dY_all=None, dY_last=None, dtype=None):
    dtype, dY_all, dY_last = _grad_seed(cache, dY_all, dY_last, dtype)
    X, p, nl = cache["X"], cache["p"], cache["nl"]
    B, T, _ = X.shape
    H = p[1].shape[0]
    grads = [np.zeros_like(a) for a in p]
    dX = np.zeros_like(X)
    carry = np.zeros((B, H), dtype)
    for t in reversed(range(T)):
        hd = carry.copy()
        if dY_all is not None:
            hd += dY_all[:, t]
        if dY_last is not None and t == T - 1:
            hd += dY_last
        ds = hd * _dact(nl, cache["pre"][t])
        grads[0] += X[:, t].T @ ds
        grads[1] += cache["hs"][t].T @ ds
        grads[2] += ds.sum(0)
        dX[:, t] = ds @ p[0].T
        carry = ds @ p[1].T
    return (dX[:, ::-1] if cache["reverse"] else dX), grads


def merge_forward(D, R, mode):
    if mode == "concat":
        return np.concatenate((D, R), axis=-1)
    if mode == "sum":
        return D + R
    if mode == "mul":
        return D * R
    if mode == "avg":
        return (D + R) / 2
    raise ValueError(mode)


def merge_backward(grad, D, R, mode):
    if mode == "concat":
        return tuple(np.split(grad, 2, axis=-1))
    if mode == "sum":
        return grad, grad
    if mode == "mul":
        return grad * R, grad * D
    if mode == "avg":
        return grad / 2, grad / 2
    raise ValueError(mode)
