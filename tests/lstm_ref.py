"""Float64 NumPy restatement of the reference LSTM (neunet/nn/layers/lstm.py: forward :312-362, BPTT :16-143, nonlinearities
:412-460) for the tests: params is the twelve arrays in the reference's order (W_f, W_i, W_o, W_c, W_hf, W_hi, W_ho, W_hc, b_f, b_i,
b_o, b_c), X is (B, T, in).  dY_all (B, T, H) and dY_last (B, H) may each be None; any of the four biases may be None (zero).

dtype=np.float32 keeps every array and every operation (exp, tanh included) in float32: the reference's own arithmetic, which works on
float32 NumPy arrays.  The distance between the two modes is what the reference's rounding alone uses of an error bound."""
import numpy as np

ACT = {"tanh": np.tanh, "sigmoid": lambda x: 1.0 / (1.0 + np.exp(-x)), "relu": lambda x: np.maximum(x, 0.0)}


def _dact(kind, x):
    if kind == "tanh":
        return 1.0 - np.tanh(x) ** 2
    if kind == "sigmoid":
        s = ACT["sigmoid"](x)
        return s * (1.0 - s)
    return (x > 0).astype(x.dtype)


def lstm_forward(X, params, h0=None, c0=None, nl="tanh", rnl="sigmoid", dtype=np.float64):
    H = np.shape(params[4])[0]
    p = [np.zeros(H, dtype) if a is None else np.asarray(a, dtype) for a in params]
    X = np.asarray(X, dtype)
    B, T, _ = X.shape
    h = np.zeros((B, H), dtype) if h0 is None else np.array(h0, dtype)
    c = np.zeros((B, H), dtype) if c0 is None else np.array(c0, dtype)
    cache = dict(X=X, p=p, nl=nl, rnl=rnl, hs=[h], cs=[c], z=[], dtype=dtype)
    Y = np.zeros((B, T, H), dtype)
    for t in range(T):
        z = [X[:, t] @ p[g] + h @ p[4 + g] + p[8 + g] for g in range(4)]
        f, i, o = (ACT[rnl](z[g]) for g in range(3))
        g_ = ACT[nl](z[3])
        c = f * c + i * g_
        h = o * ACT[nl](c)
        cache["z"].append(z)
        cache["hs"].append(h)
        cache["cs"].append(c)
        Y[:, t] = h
    return Y, cache


def lstm_backward(cache, dY_all=None, dY_last=None, dtype=None):
    X, p, nl, rnl = cache["X"], cache["p"], cache["nl"], cache["rnl"]
    dtype = cache.get("dtype", np.float64) if dtype is None else dtype
    if dtype != cache.get("dtype", np.float64):
        raise ValueError("lstm_backward: dtype differs from the forward pass that made this cache")
    dY_all = None if dY_all is None else np.asarray(dY_all, dtype)
    dY_last = None if dY_last is None else np.asarray(dY_last, dtype)
    B, T, _ = X.shape
    H = p[4].shape[0]
    grads = [np.zeros_like(a) for a in p]
    dX = np.zeros_like(X)
    dh_next, dc_next = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
    for t in reversed(range(T)):
        z = cache["z"][t]
        f, i, o = (ACT[rnl](z[g]) for g in range(3))
        g_ = ACT[nl](z[3])
        c, c_prev, h_prev = cache["cs"][t + 1], cache["cs"][t], cache["hs"][t]
        dh = dh_next.copy()
        if dY_all is not None:
            dh += dY_all[:, t]
        if dY_last is not None and t == T - 1:
            dh += dY_last
        dc = dh * o * _dact(nl, c) + dc_next
        d = [dc * c_prev * _dact(rnl, z[0]), dc * g_ * _dact(rnl, z[1]), dh * ACT[nl](c) * _dact(rnl, z[2]), dc * i * _dact(nl, z[3])]
        for k in range(4):
            grads[k] += X[:, t].T @ d[k]
            grads[4 + k] += h_prev.T @ d[k]
            grads[8 + k] += d[k].sum(0)
        dh_next = sum(d[k] @ p[4 + k].T for k in range(4))
        dc_next = dc * f
        dX[:, t] = sum(d[k] @ p[k].T for k in range(4))
    return dX, grads
