"""float64 restatements of what csrc/elementwise.hip (the activation functors), csrc/rowops.hip (LogSoftmax and its fold with NLLLoss)
and csrc/losses_latent.hip (NLLLoss, L1Loss, KLDivLoss) compute -- the closed forms of neunet/nn/activations.py:140-383, 462-492 and
neunet/nn/losses.py:83-178, written so that float64 never overflows or cancels where the functions themselves are finite."""
import numpy as np

KINDS = ("softplus", "softsign", "mish", "tanhexp", "elu", "selu", "log")          # NNHIP_ACT_* in this order
SELU_ALPHA = 1.6732632423543772848170429916717
SELU_LAMBDA = 1.0507009873554804934193349852946


def _f64(a):
    return np.asarray(a, np.float64)


def sigmoid(x):
    x = _f64(x)
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def softplus(x):
    x = _f64(x)
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))      # (np.maximum carries a NaN)


def act_forward(kind, x, alpha=0.1):
    x = _f64(x)
    with np.errstate(all="ignore"):
        if kind == "softplus":
            return softplus(x)
        if kind == "softsign":
            return x / (1 + np.abs(x))
        if kind == "mish":
            return x * np.tanh(softplus(x))
        if kind == "tanhexp":
            return x * np.tanh(np.exp(x))
        if kind == "elu":
            return np.where(x <= 0, alpha * np.expm1(np.minimum(x, 0)), x)
        if kind == "selu":
            return SELU_LAMBDA * np.where(x > 0, x, SELU_ALPHA * np.expm1(np.where(x > 0, 0, x)))
        if kind == "log":
            return np.log(x)
    raise ValueError(kind)


def act_derivative(kind, x, alpha=0.1):
    x = _f64(x)
    with np.errstate(all="ignore"):
        if kind == "softplus":
            return sigmoid(x)
        if kind == "softsign":
            return 1 / (1 + np.abs(x)) ** 2
        if kind == "mish":
            t = np.tanh(softplus(x))
            return t + x * sigmoid(x) * sech2(softplus(x))
        if kind == "tanhexp":
            e = np.exp(x)
            s2 = sech2(e)
            return np.tanh(e) + np.where(s2 == 0, 0.0, x * e * s2)
        if kind == "elu":
            return np.where(x > 0, 1.0, alpha * np.exp(np.where(x > 0, 0, x)))
        if kind == "selu":
            return SELU_LAMBDA * np.where(x > 0, 1.0, SELU_ALPHA * np.exp(np.where(x > 0, 0, x)))
        if kind == "log":
            return 1 / x
    raise ValueError(kind)


def sech2(z):
    """1 - tanh(z)^2 for z >= 0 without cancellation: 4 q / (1 + q)^2, q = exp(-2 z)."""
    q = np.exp(-2 * _f64(z))
    return 4 * q / (1 + q) ** 2


def act_backward(kind, x, dy, alpha=0.1):
    return _f64(dy) * act_derivative(kind, x, alpha)


def logsoftmax_forward(x, axis=-1):
    x = _f64(x)
    with np.errstate(all="ignore"):
        m = x.max(axis, keepdims=True)
        return x - m - np.log(np.exp(x - m).sum(axis, keepdims=True))


def logsoftmax_backward(y, dy, axis=-1):
    y, dy = _f64(y), _f64(dy)
    return dy - np.exp(y) * dy.sum(axis, keepdims=True)


def nll(logp, labels, weight=None, ignore_index=-100, reduction="mean"):
    """(loss, dlogp, pos_grad) for logp [outer, C, inner] and labels [outer, inner]: a position counts when its label is not
    ignore_index and lies in [0, C); 'mean' divides by the summed weights of the counted positions, and a zero denominator gives
    loss 0 and a zero gradient."""
    logp = _f64(logp)
    outer, C, inner = logp.shape
    labels = np.asarray(labels).reshape(outer, inner).astype(np.int64)
    w = np.ones(C) if weight is None else _f64(weight)
    counts = (labels != ignore_index) & (labels >= 0) & (labels < C)
    safe = np.where(counts, labels, 0)
    n_idx, i_idx = np.indices((outer, inner))
    wy = np.where(counts, w[safe], 0.0)
    terms = np.where(counts, -logp[n_idx, safe, i_idx] * wy, 0.0)
    den = wy.sum()
    scale = (1.0 / den if den > 0 else 0.0) if reduction == "mean" else 1.0
    pos_grad = np.where(counts, -wy * scale, 0.0)
    dlogp = np.zeros_like(logp)
    dlogp[n_idx[counts], safe[counts], i_idx[counts]] = pos_grad[counts]
    loss = terms if reduction == "none" else terms.sum() * scale
    return loss, dlogp, pos_grad


def logsoftmax_nll_backward(y, labels, pos_grad, upstream=1.0):
    """dX[n, c] = g_n ([c == y_n] - exp(Y[n, c])) u; rows with g_n == 0 are zeros."""
    y = _f64(y)
    onehot = np.arange(y.shape[1])[None, :] == np.asarray(labels).reshape(-1, 1)
    g = _f64(pos_grad).reshape(-1, 1)
    return np.where(g == 0, 0.0, g * upstream * (onehot - np.exp(y)))


def l1(p, t, reduction="mean"):
    d = _f64(p) - _f64(t)
    scale = 1.0 / d.size if reduction == "mean" else 1.0
    terms = np.abs(d)
    return (terms if reduction == "none" else terms.sum() * scale), np.sign(d) * scale


def kldiv(p, t, reduction="mean", log_target=False):
    p, t = _f64(p), _f64(t)
    with np.errstate(all="ignore"):
        w = np.exp(t) if log_target else t
        terms = w * (t - p) if log_target else w * (np.log(t) - p)
    scale = {"mean": 1.0 / p.size, "batchmean": 1.0 / p.shape[0], "sum": 1.0, "none": 1.0}[reduction]
    return (terms if reduction == "none" else terms.sum() * scale), -w * scale


ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8          # the reference's defaults (neunet/optim.py:5)


def adam_update(grads, lr):
    """The update Adam subtracts in step len(grads) from zero moments, given the gradients of every step so far, in float64
    (neunet/optim.py:27-33: bias-corrected moments, lr m_hat / (sqrt(v_hat) + eps))."""
    m = v = 0.0
    for g in grads:
        m, v = ADAM_B1 * m + (1 - ADAM_B1) * g, ADAM_B2 * v + (1 - ADAM_B2) * g ** 2
    t = len(grads)
    return lr * (m / (1 - ADAM_B1 ** t)) / (np.sqrt(v / (1 - ADAM_B2 ** t)) + ADAM_EPS)


def adam_param_bounds(grads, gscales, lr):
    """For one parameter and the reference's gradients of steps 0 .. S-1: per step (bound on |p - p_ref| after that step WITHOUT the
    rounding term, untouched, clear).  Every step's gradient is assumed within e_k = 1e-4 max(|g_k|, rms(g_k), gscale_k) of the
    reference's (what the gradient check asserts).
      step 0   the first-step rule of test_vae_step_vs_reference (check_first_adam_step): 1e-4 lr + lr eps e / (|g| - e)^2 where the
               gradient's sign is clear (|g| > 2 e), 2 lr elsewhere;
      step k   the sensitivity rule of test_gan_step_vs_reference: 1e-4 lr + twice the largest change of the float64 update over the
               corners g_j +- e_j, j <= k;
    the steps' bounds add up.  untouched: the reference's gradient is exactly 0 in every step so far (embedding rows no pair has used,
    units the ReLU keeps off): Adam moves such an element by exactly 0, so it is held to its initial bits, its bound is 0, and -- since
    any non-zero gradient would have moved it by about lr -- its e_k is 0 in the later steps' corners."""
    import itertools
    gs = [_f64(g) for g in grads]
    es = [1e-4 * np.maximum(np.maximum(np.abs(g), np.sqrt(np.mean(g ** 2))), sc) for g, sc in zip(gs, gscales)]
    out, total = [], 0.0
    untouched = np.ones(gs[0].shape, bool)
    clear = np.abs(gs[0]) > 2 * es[0]
    for k in range(len(gs)):
        untouched = untouched & (gs[k] == 0)
        es[k] = np.where(untouched, 0.0, es[k])          # held to its initial bits after this step: its gradient here was exactly 0
        if k == 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                step = np.where(clear, 1e-4 * lr + lr * ADAM_EPS * es[0] / (np.abs(gs[0]) - es[0]) ** 2, 2 * lr)
        else:
            u = adam_update(gs[:k + 1], lr)
            sens = np.max([np.abs(adam_update([g + sg * e for g, e, sg in zip(gs, es, signs)], lr) - u)
                           for signs in itertools.product((-1, 1), repeat=k + 1)], axis=0)
            step = 1e-4 * lr + 2 * sens
        total = total + np.where(untouched, 0.0, step)
        out.append((total, untouched.copy(), clear))
    return out
