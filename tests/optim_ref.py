"""Float32 NumPy restatement of the reference's SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax and NAdam (neunet/optim.py:76-244)
for the tests.  Every array is float32 and every hyper-parameter a Python float, as in the reference: NumPy rounds a Python float
to float32 where it meets an array, and `1 - x` / `1 - beta ** t` are formed in double first.  `grad_scale` multiplies the gradient
first (1.0: the reference's arithmetic exactly).

    state = init_state(rule, p)             # [] / [m] / [m, v] of zeros
    step(rule, p, g, state, t, **hyper)     # in place; t = 1, 2, ... (used by adamax / nadam)

DEFAULTS holds the reference's constructor defaults per rule."""
import numpy as np

RULES = ("sgd", "momentum", "rmsprop", "adagrad", "adadelta", "adamax", "nadam")
N_STATE = {"sgd": 0, "momentum": 1, "rmsprop": 1, "adagrad": 1, "adadelta": 2, "adamax": 2, "nadam": 2}
BYTES_PER_ELEMENT = {r: 12 + 8 * n for r, n in N_STATE.items()}
CLASS_NAMES = {"sgd": "SGD", "momentum": "Momentum", "rmsprop": "RMSprop", "adagrad": "Adagrad", "adadelta": "Adadelta",
               "adamax": "Adamax", "nadam": "NAdam"}
DEFAULTS = {
    "sgd": dict(lr=0.01),
    "momentum": dict(lr=0.01, momentum=0.9),
    "rmsprop": dict(lr=0.01, alpha=0.99, eps=1e-8),
    "adagrad": dict(lr=0.01, eps=1e-8),
    "adadelta": dict(lr=1.0, rho=0.9, eps=1e-6),
    "adamax": dict(lr=0.002, betas=(0.9, 0.999), eps=1e-8),
    "nadam": dict(lr=0.002, betas=(0.9, 0.999), eps=1e-8),
}
F32 = np.float32


def init_state(rule, p):
    return [np.zeros_like(p, dtype=F32) for _ in range(N_STATE[rule])]


def coefficients(rule, hyper):
    """(coef1, coef2, eps) as the C entries take them."""
    h = dict(DEFAULTS[rule], **hyper)
    if rule == "momentum":
        return h["momentum"], 0.0, 0.0
    if rule == "rmsprop":
        return h["alpha"], 0.0, h["eps"]
    if rule == "adagrad":
        return 0.0, 0.0, h["eps"]
    if rule == "adadelta":
        return h["rho"], 0.0, h["eps"]
    if rule in ("adamax", "nadam"):
        return h["betas"][0], h["betas"][1], h["eps"]
    return 0.0, 0.0, 0.0


def step(rule, p, g, state, t, grad_scale=1.0, **hyper):
    h = dict(DEFAULTS[rule], **hyper)
    assert p.dtype == F32 and g.dtype == F32 and all(s.dtype == F32 for s in state)
    lr = h["lr"]
    g = g * F32(grad_scale)
    if rule == "sgd":
        p -= lr * g
    elif rule == "momentum":
        m, = state
        m[...] = h["momentum"] * m + (1 - h["momentum"]) * g
        p -= m * lr
    elif rule == "rmsprop":
        m, = state
        m[...] = h["alpha"] * m + (1 - h["alpha"]) * g**2
        p -= lr * g / (np.sqrt(m) + h["eps"])
    elif rule == "adagrad":
        m, = state
        m += g**2
        p -= lr * g / (np.sqrt(m) + h["eps"])
    elif rule == "adadelta":
        m, v = state
        m[...] = h["rho"] * m + (1 - h["rho"]) * g**2
        dx = -(np.sqrt(v + h["eps"]) / np.sqrt(m + h["eps"])) * g
        v[...] = h["rho"] * v + (1 - h["rho"]) * dx**2
        p += dx
    elif rule == "adamax":
        m, v = state
        b1, b2 = h["betas"]
        m[...] = b1 * m + (1 - b1) * g
        v[...] = np.maximum(b2 * v, np.abs(g))
        m_hat = m / (1 - b1**t)
        p -= lr * m_hat / (v + h["eps"])
    elif rule == "nadam":
        m, v = state
        b1, b2 = h["betas"]
        m[...] = b1 * m + (1 - b1) * g
        v[...] = b2 * v + (1 - b2) * g**2
        m_hat = m / (1 - b1**t) + (1 - b1) * g / (1 - b1**t)
        v_hat = v / (1 - b2**t)
        p -= lr * m_hat / (np.sqrt(v_hat) + h["eps"])
    else:
        raise ValueError(rule)
    assert p.dtype == F32 and all(s.dtype == F32 for s in state)
