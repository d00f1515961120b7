"""Float32 NumPy restatement of the reference's SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax and NAdam (neunet/optim.py:76-244)
for the tests.  Every array is float32 and every hyper-parameter a Python float, as in the reference: NumPy rounds a Python float
to float32 where it meets an array, and `1 - x` / `1 - beta ** t` are formed in double first.  `grad_scale` multiplies the gradient
first (1.0: the reference's arithmetic exactly).

    state = init_state(rule, p)             # [] / [m] / [m, v] of zeros
    step(rule, p, g, state, t, **hyper)     # in place; t = 1, 2, ... (used by adamax / nadam)

DEFAULTS holds the reference's constructor defaults per rule.

For the path-by-path GPU tests (tests/test_optim_rules_tiers_gpu.py):

    step64(rule, p, g, state, t, **hyper)   float64 arrays: the exact value of what the kernel is asked to compute, from the
                                            float32-rounded hyper-parameters csrc/adam_device.h's make_hyper forms
    plan(sizes) -> (chunk, blocks)          the multi-tensor launch's chunk plan (csrc/optim.hip: fused_optimizer_plan)
    plan_bytes(rule, sizes)                 the size of that plan's blob: (2 + N_STATE) pointer tables, sizes, two int32 per block
    per_tensor_grid(n, vec)                 the per-tensor launch's stride in threads (csrc/optim_rules.hip: launch_rule)
    trips(n, first, stride, U)              what thread `first` of `stride` does in rule_span: (U-round trips, 2-round trips,
                                            single rounds, tail elements); span_elements: the elements those touch
    scenario(name) / Trace(rule, sc)        the inputs of every GPU test that compares with float64, and both references stepped
                                            side by side on them, so that tests/test_optim.py can hold `step` to `step64` on the CPU"""
import collections

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


# ------------------------------------------------------------------------------------------------------------ the float64 value
F64 = np.float64


def rounded_hyper(rule, t, grad_scale=1.0, **hyper):
    """make_hyper's float32 values, as float64: lr, c1, c2, 1 - c1, 1 - c2 (formed in double, then rounded), eps, 1 - c1^t,
    1 - c2^t (likewise), grad_scale.  c1 / c2: the rule's coefficients as the C entries take them."""
    h = dict(DEFAULTS[rule], **hyper)
    c1, c2, eps = (float(x) for x in coefficients(rule, hyper))
    vals = dict(lr=h["lr"], c1=c1, c2=c2, omc1=1.0 - c1, omc2=1.0 - c2, eps=eps, bc1=1.0 - c1 ** t, bc2=1.0 - c2 ** t, gs=grad_scale)
    return {k: float(F32(v)) for k, v in vals.items()}


def step64(rule, p, g, state, t, grad_scale=1.0, **hyper):
    """csrc/optim_rules_device.h: rule1, evaluated in float64 (in place on p and the states)."""
    assert p.dtype == F64 and all(s.dtype == F64 for s in state) and len(state) == N_STATE[rule]
    h = rounded_hyper(rule, t, grad_scale, **hyper)
    lr, c1, c2, omc1, omc2, eps = h["lr"], h["c1"], h["c2"], h["omc1"], h["omc2"], h["eps"]
    g = g.astype(F64) * h["gs"]
    if rule == "sgd":
        p -= lr * g
    elif rule == "momentum":
        m, = state
        m[...] = c1 * m + omc1 * g
        p -= m * lr
    elif rule == "rmsprop":
        m, = state
        m[...] = c1 * m + omc1 * (g * g)
        p -= lr * g / (np.sqrt(m) + eps)
    elif rule == "adagrad":
        m, = state
        m += g * g
        p -= lr * g / (np.sqrt(m) + eps)
    elif rule == "adadelta":
        m, v = state
        m[...] = c1 * m + omc1 * (g * g)
        dx = -(np.sqrt(v + eps) / np.sqrt(m + eps)) * g
        v[...] = c1 * v + omc1 * (dx * dx)
        p += dx
    elif rule == "adamax":
        m, v = state
        m[...] = c1 * m + omc1 * g
        v[...] = np.maximum(c2 * v, np.abs(g))
        p -= lr * (m / h["bc1"]) / (v + eps)
    elif rule == "nadam":
        m, v = state
        m[...] = c1 * m + omc1 * g
        v[...] = c2 * v + omc2 * (g * g)
        mh = m / h["bc1"] + omc1 * g / h["bc1"]
        p -= lr * mh / (np.sqrt(v / h["bc2"]) + eps)
    else:
        raise ValueError(rule)


def worst_ratio(a, b, atol, rtol):
    """max |a - b| / (atol + rtol |b|): <= 1 is what assert_allclose(a, b, rtol, atol) accepts."""
    a, b = np.asarray(a, F64).reshape(-1), np.asarray(b, F64).reshape(-1)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


# ------------------------------------------------------------------------------------------- the plan and rule_span, restated
MT_CHUNK_SMALL, MT_CHUNK, MT_LARGE_FROM = 2048, 16384, 1 << 22     # csrc/optim.hip
GRID_CAP, BLOCK = 2048, 256                                        # csrc/optim_rules.hip: launch_rule
UNROLL = {0: 4, 1: 2, 2: 2}                                        # RuleUnroll: float4 rounds in flight, by state-stream count


def unroll(rule):
    return UNROLL[N_STATE[rule]]


def plan(sizes):
    """(elements per block, blocks) of one multi-tensor launch over tensors of these sizes."""
    sizes = [int(n) for n in sizes]
    chunk = MT_CHUNK if sum(sizes) >= MT_LARGE_FROM else MT_CHUNK_SMALL
    return chunk, sum(-(-n // chunk) for n in sizes)


def plan_bytes(rule, sizes):
    """Bytes of the plan blob: (2 + N_STATE) tables of 8-byte pointers, the int64 sizes, blk_tensor and blk_chunk (int32 each)."""
    return 8 * (2 + N_STATE[rule]) * len(sizes) + 8 * len(sizes) + 8 * plan(sizes)[1]


def chunks(n, chunk):
    """Element counts of a tensor's chunks, in block order."""
    return [min(chunk, n - off) for off in range(0, n, chunk)]


def per_tensor_grid(n, vec):
    """Threads of nnhipOptimizerRuleStep's launch (the span's stride): 256 per block, one thread per float4 (and one block more for
    the tail) or per element, at most 2048 blocks."""
    blocks = -(-((n >> 2) + 1 if vec else n) // BLOCK)
    return min(blocks, GRID_CAP) * BLOCK


def _walk(n, first, stride, U):
    """rule_span's vector path for one thread: (rounds of the loop level, first float4 index) per trip, then ('tail', element)."""
    nv = n >> 2
    i = first
    while i + (U - 1) * stride < nv:
        yield U, i
        i += U * stride
    if U > 2:
        while i + stride < nv:
            yield 2, i
            i += 2 * stride
    while i < nv:
        yield 1, i
        i += stride
    for j in range((nv << 2) + first, n, stride):
        yield "tail", j


def trips(n, first, stride, U):
    """(U-round trips, 2-round trips -- a loop level of its own only where U > 2 --, single rounds, tail elements) of thread `first`."""
    kinds = [k for k, _ in _walk(n, first, stride, U)]
    return kinds.count(U), (kinds.count(2) if U > 2 else 0), kinds.count(1), kinds.count("tail")


def span_elements(n, first, stride, U):
    """The elements thread `first` updates, in the order it does."""
    out = []
    for kind, i in _walk(n, first, stride, U):
        if kind == "tail":
            out.append(i)
        else:
            for u in range(kind):
                out.extend(range(4 * (i + u * stride), 4 * (i + u * stride) + 4))
    return out


def trip_classes(n, stride, U, threads=BLOCK):
    """{trips: number of threads} over threads 0 .. threads - 1 of a span with this stride."""
    return dict(collections.Counter(trips(n, f, stride, U) for f in range(threads)))


# ------------------------------------------------------------------------------------------------------------------- the inputs
# As tests/adam_ref.py.  grads[s][i]: tensor i's gradient at step s (None: no gradient, the optimizer skips it); t0: steps taken
# before; m0 / v0: the states then; idx[i]: flat indices of tensor i that the references follow (None: all) -- the rules are
# elementwise, so a sample of a long tensor is exact; over[s]: what step s changes of lr / betas / grad_scale / `coef` (the rule's
# own coefficient: COEF_NAME).  The data does not depend on the rule; every other hyper-parameter is the rule's default.
Scenario = collections.namedtuple("Scenario", "shapes p0 m0 v0 grads t0 idx over")
COEF_NAME = {"momentum": "momentum", "rmsprop": "alpha", "adadelta": "rho"}

TAIL_SHAPES = [(1,), (3,), (4,), (5,), (1023,), (1027,), (1500,), (2047,), (2048,), (2049,), (4099,), (1000, 333)]
# 16384-element chunks.  The long tensor ends in a chunk of 4 * (7 * 256 + 100) + 3 elements: 1892 float4 for 256 threads
LARGE_LAST = 4 * (7 * 256 + 100) + 3
LARGE_SHAPES = [(256 * MT_CHUNK + LARGE_LAST,), (16385,), (3,)]
# the per-tensor entry beyond its grid cap: a stride of 2048 x 256 float4, k strides and 300 float4 and 3 elements
STRIDE4 = GRID_CAP * BLOCK
PT_SMALL_SHAPES = [(1,), (3,), (4,), (1027,)]
PT_N = {k: 4 * (k * STRIDE4 + 300) + 3 for k in (2, 3, 5)}
PT_STRIDES = {0: (3, 5), 1: (2, 3), 2: (2, 3)}                    # by state count: the smallest sizes that reach every loop level
PT_SCALAR_N = 2 * STRIDE4 + 300                                   # elements: the scalar path's stride is 2048 x 256 floats
ZERO_MID_SHAPES = [(300,), (0,), (2049,)]
DEV_SHAPES = [(2049,), (300,), (5,)]
SCENARIO_NAMES = ("tail", "large", "pt_small", "pt_2", "pt_3", "pt_5", "pt_scalar", "zero_mid", "resume_1000", "resume_99990",
                  "dev_betas", "dev_coef", "dev_blocks", "dev_hyper")
BETA_RULES = ("adamax", "nadam")


def rules_of(name):
    """The rules a scenario is run with."""
    if name in ("pt_2", "pt_3", "pt_5"):
        return tuple(r for r in RULES if int(name[3:]) in PT_STRIDES[N_STATE[r]])
    if name.startswith("resume_") or name == "dev_betas":
        return BETA_RULES
    if name == "dev_coef":
        return tuple(COEF_NAME)
    return RULES


def ends_and_stride(n, ends, stride=1021):
    return np.unique(np.concatenate([np.arange(ends), np.arange(n - ends, n), np.arange(0, n, stride)]))


def _normal(rng, shape):
    a = rng.standard_normal(shape, dtype=F32)
    a.setflags(write=False)
    return a


def _build(name):
    rng = np.random.default_rng([2401, SCENARIO_NAMES.index(name)])
    kw = dict(t0=0, m0=None, v0=None, idx=None)
    steps, skip, over = 3, {}, {}
    if name == "tail":
        shapes = TAIL_SHAPES
    elif name == "large":
        shapes = LARGE_SHAPES
        kw["idx"] = [ends_and_stride(shapes[0][0], MT_CHUNK + 8), None, None]
    elif name == "pt_small":
        shapes, steps = PT_SMALL_SHAPES, 2
    elif name in ("pt_2", "pt_3", "pt_5"):
        shapes, steps = [(PT_N[int(name[3:])],)], 2
        kw["idx"] = [ends_and_stride(shapes[0][0], 16384)]
    elif name == "pt_scalar":
        shapes, steps = [(PT_SCALAR_N,)], 2
        kw["idx"] = [ends_and_stride(PT_SCALAR_N, 16384)]
    elif name == "zero_mid":
        shapes, steps = ZERO_MID_SHAPES, 2
    elif name in ("resume_1000", "resume_99990"):
        shapes, steps, kw["t0"] = DEV_SHAPES, 5, int(name.split("_")[1])
    elif name == "dev_betas":                                      # other betas for two steps, then back
        shapes, steps = DEV_SHAPES, 6
        over = {2: dict(betas=(0.8, 0.99)), 3: dict(betas=(0.8, 0.99))}
    elif name == "dev_coef":                                       # the rule's coefficient: another value from the third step on
        shapes, steps = DEV_SHAPES, 5
        over = {s: dict(coef=0.5) for s in (2, 3, 4)}
    elif name == "dev_blocks":                                     # the 2049-element tensor (2 of the 4 blocks) sits out the second step
        shapes, steps, skip = DEV_SHAPES, 4, {1: (0,)}
    elif name == "dev_hyper":                                      # lr, then grad_scale
        shapes, steps = DEV_SHAPES, 5
        over = {1: dict(lr=3e-3), 2: dict(lr=3e-3), 3: dict(lr=3e-3, grad_scale=0.5), 4: dict(lr=3e-3, grad_scale=0.5)}
    else:
        raise KeyError(name)
    p0 = [_normal(rng, s) for s in shapes]
    if kw["t0"]:                                                   # states as training leaves them: m ~ g, v ~ g^2 >= 0
        kw["m0"] = [_normal(rng, s) for s in shapes]
        kw["v0"] = [np.square(_normal(rng, s)) for s in shapes]
        for a in kw["v0"]:
            a.setflags(write=False)
    grads = [[None if i in skip.get(s, ()) else _normal(rng, shape) for i, shape in enumerate(shapes)] for s in range(steps)]
    return Scenario(shapes=shapes, p0=p0, grads=grads, over=[over.get(s, {}) for s in range(steps)], **kw)


_cache = {}


def scenario(name):
    """Built once, shared by the rules and read-only."""
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def hyper_of(rule, over):
    """A scenario step's `over` as keyword arguments of step / step64 for this rule."""
    h = {k: v for k, v in over.items() if k not in ("coef", "betas")}
    if "coef" in over and rule in COEF_NAME:
        h[COEF_NAME[rule]] = over["coef"]
    if "betas" in over and rule in BETA_RULES:
        h["betas"] = over["betas"]
    return h


class Trace:
    """Both references side by side on a scenario's tensors (restricted to idx): p32[i], s32[i][k] and p64[i], s64[i][k]."""

    def __init__(self, rule, sc):
        self.rule, self.sc, self.t = rule, sc, sc.t0
        n = len(sc.shapes)
        self.p32 = [self.pick(i, sc.p0[i]).copy() for i in range(n)]
        self.s32 = []
        for i in range(n):
            if sc.m0 is None:
                self.s32.append(init_state(rule, self.p32[i]))
            else:
                self.s32.append([self.pick(i, a[i]).copy() for a in (sc.m0, sc.v0)[:N_STATE[rule]]])
        self.p64 = [a.astype(F64) for a in self.p32]
        self.s64 = [[a.astype(F64) for a in s] for s in self.s32]

    def pick(self, i, a):
        a = np.asarray(a).reshape(-1)
        return a if self.sc.idx is None or self.sc.idx[i] is None else a[self.sc.idx[i]]

    def step(self):
        """The scenario's next optimizer step: every tensor with a gradient moves, the step count advances for all."""
        sc = self.sc
        s = self.t - sc.t0
        self.t += 1
        h = hyper_of(self.rule, sc.over[s])
        for i, g in enumerate(sc.grads[s]):
            if g is None or self.p32[i].size == 0:
                continue
            g = self.pick(i, g)
            step(self.rule, self.p32[i], g, self.s32[i], self.t, **h)
            step64(self.rule, self.p64[i], g, self.s64[i], self.t, **h)

    def ratios(self, rtol, atol_p, atol_s):
        """Worst ratio of `step` against `step64`: [p, first state, second state] (as many as the rule has streams)."""
        out = [max([worst_ratio(a, b, atol_p, rtol) for a, b in zip(self.p32, self.p64)] + [0.0])]
        for k in range(N_STATE[self.rule]):
            out.append(max([worst_ratio(a[k], b[k], atol_s[k], rtol) for a, b in zip(self.s32, self.s64)] + [0.0]))
        return out
