"""Float64 NumPy restatements of what the GPT-2 inference path adds, for the tests (and for tools/gen_golden.py, which asserts the
greedy fixture's margins with them): LayerNorm (neunet/nn/layers/layernorm.py:115-147 forward, :48-93 backward), GELU in its tanh
form (neunet/nn/activations.py:386-422) with the EXACT derivative, one-query attention over a key/value cache, and the GPT-2 model
of the reference's examples/gpt2/gpt2_infer.py:129-253 forward and backward.

Model parameters travel as a dict under the state_dict() names of the model (`wte.weight`, `h.0.ln_1.weight`, `h.0.attn.c_attn.weight`
[3D, D], `h.0.attn.c_attn.bias` [1, 3D], ..., `ln_f.bias`, `lm_head.weight`); Linear weights are [out, in] as nn.Linear holds them."""
import numpy as np

SQRT_2_OVER_PI = np.sqrt(2.0 / np.pi)
GELU_C = 0.044715


# ---------------------------------------------------------------------------------------------- LayerNorm
def layernorm_forward(X, w=None, b=None, eps=1e-5, n_axes=1):
    """Normalise over the last n_axes axes (biased variance).  Returns (Y, cache)."""
    X = np.asarray(X, np.float64)
    axis = tuple(range(-n_axes, 0))
    mean = X.mean(axis=axis, keepdims=True)
    var = X.var(axis=axis, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (X - mean) * rstd
    Y = xhat
    if w is not None:
        Y = Y * np.asarray(w, np.float64)
    if b is not None:
        Y = Y + np.asarray(b, np.float64)
    return Y, dict(xhat=xhat, rstd=rstd, w=None if w is None else np.asarray(w, np.float64), axis=axis, mean=mean)


def layernorm_backward(cache, dY):
    """(dX, dw, db): dw / db are the sums over EVERY leading axis (what the reference's axis-0 sum + reverse broadcast leaves)."""
    dY = np.asarray(dY, np.float64)
    xhat, rstd, w, axis = cache["xhat"], cache["rstd"], cache["w"], cache["axis"]
    g = dY if w is None else dY * w
    dX = rstd * (g - g.mean(axis=axis, keepdims=True) - xhat * (g * xhat).mean(axis=axis, keepdims=True))
    lead = tuple(range(dY.ndim - len(axis)))
    return dX, (dY * xhat).sum(axis=lead), dY.sum(axis=lead)


# ---------------------------------------------------------------------------------------------- GELU (tanh form)
def gelu_forward(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(SQRT_2_OVER_PI * (x + GELU_C * x ** 3)))


def gelu_backward(x, dY):
    x = np.asarray(x, np.float64)
    u = SQRT_2_OVER_PI * (x + GELU_C * x ** 3)
    t = np.tanh(u)
    return np.asarray(dY, np.float64) * (0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * SQRT_2_OVER_PI * (1.0 + 3.0 * GELU_C * x * x))


# ---------------------------------------------------------------------------------------------- one query over a cache
def attention_decode(q, K, V, lengths, scale):
    """q [B, H, dh]; K, V [B, H, Tmax, dh]; row b attends keys 0 .. lengths[b]-1.  Returns [B, H, dh]."""
    q, K, V = (np.asarray(a, np.float64) for a in (q, K, V))
    out = np.zeros_like(q)
    for b in range(q.shape[0]):
        n = int(lengths[b])
        s = np.einsum("hd,htd->ht", q[b], K[b, :, :n]) * scale
        s -= s.max(axis=1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(axis=1, keepdims=True)
        out[b] = np.einsum("ht,htd->hd", p, V[b, :, :n])
    return out


# ---------------------------------------------------------------------------------------------- GPT-2
def _p(params, name):
    return np.asarray(params[name], np.float64)


def gpt2_forward(params, ids, n_head, eps=1e-5):
    """ids int [B, T] -> (logits [B, T, V] float64, cache for gpt2_backward)."""
    ids = np.asarray(ids)
    B, T = ids.shape
    wte, wpe = _p(params, "wte.weight"), _p(params, "wpe.weight")
    D = wte.shape[1]
    H, dh = n_head, D // n_head
    n_layer = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("h."))
    x = wte[ids] + wpe[:T][None]
    mask = np.tril(np.ones((T, T), bool))
    layers = []
    for i in range(n_layer):
        pre = f"h.{i}."
        a, c1 = layernorm_forward(x, _p(params, pre + "ln_1.weight"), _p(params, pre + "ln_1.bias"), eps)
        qkv = a @ _p(params, pre + "attn.c_attn.weight").T + _p(params, pre + "attn.c_attn.bias").reshape(-1)
        q, k, v = (qkv[..., j * D:(j + 1) * D].reshape(B, T, H, dh).transpose(0, 2, 1, 3) for j in range(3))
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(dh)
        s = np.where(mask, s, -1e9)
        s = s - s.max(-1, keepdims=True)
        att = np.exp(s)
        att /= att.sum(-1, keepdims=True)
        y = (att @ v).transpose(0, 2, 1, 3).reshape(B, T, D)
        x1 = x + y @ _p(params, pre + "attn.c_proj.weight").T + _p(params, pre + "attn.c_proj.bias").reshape(-1)
        m, c2 = layernorm_forward(x1, _p(params, pre + "ln_2.weight"), _p(params, pre + "ln_2.bias"), eps)
        hfc = m @ _p(params, pre + "mlp.c_fc.weight").T + _p(params, pre + "mlp.c_fc.bias").reshape(-1)
        g = gelu_forward(hfc)
        x2 = x1 + g @ _p(params, pre + "mlp.c_proj.weight").T + _p(params, pre + "mlp.c_proj.bias").reshape(-1)
        layers.append(dict(c1=c1, a=a, q=q, k=k, v=v, att=att, y=y, c2=c2, m=m, hfc=hfc, g=g))
        x = x2
    xf, cf = layernorm_forward(x, _p(params, "ln_f.weight"), _p(params, "ln_f.bias"), eps)
    logits = xf @ _p(params, "lm_head.weight").T
    return logits, dict(ids=ids, layers=layers, cf=cf, xf=xf, n_head=n_head, params=params)


def gpt2_backward(cache, dlogits, embedding_grad="assign"):
    """Gradients of every parameter, as a dict under the same names (lm_head.weight and wte.weight separately: a tied model's
    gradient is their sum).  embedding_grad="assign": the reference's token-embedding gradient, an ASSIGNMENT through the index
    (neunet/autograd.py:905-912) -- of the positions that repeat an id only the last one contributes; "sum": the mathematical one."""
    params, ids, H = cache["params"], cache["ids"], cache["n_head"]
    dlogits = np.asarray(dlogits, np.float64)
    B, T = ids.shape
    grads = {}
    Wlm = _p(params, "lm_head.weight")
    D = Wlm.shape[1]
    dh = D // H
    grads["lm_head.weight"] = dlogits.reshape(-1, Wlm.shape[0]).T @ cache["xf"].reshape(-1, D)
    dx, grads["ln_f.weight"], grads["ln_f.bias"] = layernorm_backward(cache["cf"], dlogits @ Wlm)
    for i in reversed(range(len(cache["layers"]))):
        pre, L = f"h.{i}.", cache["layers"][i]

        def lin_bwd(name, inp, dout):
            W = _p(params, pre + name + ".weight")
            grads[pre + name + ".weight"] = dout.reshape(-1, W.shape[0]).T @ inp.reshape(-1, W.shape[1])
            grads[pre + name + ".bias"] = dout.reshape(-1, W.shape[0]).sum(0).reshape(1, -1)
            return dout @ W

        dg = lin_bwd("mlp.c_proj", L["g"], dx)
        dm = lin_bwd("mlp.c_fc", L["m"], gelu_backward(L["hfc"], dg))
        d1, grads[pre + "ln_2.weight"], grads[pre + "ln_2.bias"] = layernorm_backward(L["c2"], dm)
        dx = dx + d1
        dy = lin_bwd("attn.c_proj", L["y"], dx).reshape(B, T, H, dh).transpose(0, 2, 1, 3)
        datt = dy @ L["v"].transpose(0, 1, 3, 2)
        dv = L["att"].transpose(0, 1, 3, 2) @ dy
        ds = L["att"] * (datt - (datt * L["att"]).sum(-1, keepdims=True)) / np.sqrt(dh)
        dq, dk = ds @ L["k"], ds.transpose(0, 1, 3, 2) @ L["q"]
        dqkv = np.concatenate([t.transpose(0, 2, 1, 3).reshape(B, T, D) for t in (dq, dk, dv)], axis=-1)
        d1, grads[pre + "ln_1.weight"], grads[pre + "ln_1.bias"] = layernorm_backward(L["c1"], lin_bwd("attn.c_attn", L["a"], dqkv))
        dx = dx + d1
    gw = np.zeros_like(_p(params, "wte.weight"))
    if embedding_grad == "sum":
        np.add.at(gw, ids.reshape(-1), dx.reshape(-1, D))
    else:
        for pos, tok in enumerate(ids.reshape(-1)):
            gw[tok] = dx.reshape(-1, D)[pos]
    grads["wte.weight"] = gw
    gp = np.zeros_like(_p(params, "wpe.weight"))
    gp[:T] = dx.sum(0)
    grads["wpe.weight"] = gp
    return grads


def cross_entropy_mean(logits, targets):
    """(loss, dlogits) of the mean cross entropy over every position."""
    logits = np.asarray(logits, np.float64)
    V = logits.shape[-1]
    z = logits.reshape(-1, V)
    z = z - z.max(1, keepdims=True)
    lp = z - np.log(np.exp(z).sum(1, keepdims=True))
    t = np.asarray(targets).reshape(-1)
    n = t.size
    d = np.exp(lp)
    d[np.arange(n), t] -= 1.0
    return -lp[np.arange(n), t].mean(), (d / n).reshape(logits.shape)


def greedy_margins(step_logits):
    """Per step: (top-1 minus top-2) / max|logit| -- the fixture's condition is >= 1e-3 at every step."""
    L = np.asarray(step_logits, np.float64)
    top = np.sort(L, axis=-1)
    return (top[:, -1] - top[:, -2]) / np.abs(L).max(axis=-1)
