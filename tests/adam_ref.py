"""Adam / AdamW references for the tests of csrc/optim.hip, and the inputs those tests share.

    step32(mode, p, g, m, v, t, lr, betas, eps, wd, grad_scale=1.0)    float32: oracle/neunet_oracle.py's adam_step / adamw_step -- the
                                                                       reference's arithmetic exactly -- on float32 arrays
    step64(...)                                                        the same update in float64, from the float32-rounded
                                                                       hyper-parameters csrc/adam_device.h's make_hyper forms: the exact
                                                                       value of what the kernel is asked to compute
    plan(sizes) -> (chunk, blocks)                                     the multi-tensor launch's chunk plan (csrc/optim.hip)

Both steps work in place on p, m and v.  `mode` is the library's decay_mode: 0 decoupled (AdamW), 1 L2-on-gradient (Adam).  The
gradient is multiplied by float32(grad_scale) first, as adam1 does.

scenario(name, mode): the inputs of every GPU test that compares with float64 (tests/test_adam_tiers_gpu.py), so that
tests/test_adam_ref.py can hold step32 to step64 on exactly those inputs on the CPU.  Trace steps both references side by side."""
import collections

import numpy as np

from oracle import neunet_oracle as O

DECOUPLED, L2_ON_GRAD = 0, 1
MODES = (DECOUPLED, L2_ON_GRAD)
F32, F64 = np.float32, np.float64
# test_adam_golden's tolerances (tests/test_hip_parity.py; tests/test_optim.py: RTOL, ATOL_P, ATOL_S): p, m, v
RTOL, ATOL = 1e-5, (1e-6, 1e-7, 1e-8)
MT_CHUNK_SMALL, MT_CHUNK, MT_LARGE_FROM = 2048, 16384, 1 << 22


def step32(mode, p, g, m, v, t, lr, betas, eps, wd, grad_scale=1.0):
    assert p.dtype == g.dtype == m.dtype == v.dtype == F32
    g = g * F32(grad_scale)
    fn = O.adam_step if mode == L2_ON_GRAD else O.adamw_step
    m2, v2 = fn(p, g, m, v, t, lr, betas, eps, wd)
    assert p.dtype == m2.dtype == v2.dtype == F32
    m[...] = m2
    v[...] = v2


def rounded_hyper(t, lr, betas, eps, wd, grad_scale=1.0):
    """make_hyper's float32 values, as float64: (lr, b1, b2, 1 - b1, 1 - b2, eps, wd, bc1, bc2, grad_scale)."""
    b1, b2 = float(betas[0]), float(betas[1])
    vals = (lr, b1, b2, 1.0 - b1, 1.0 - b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t, grad_scale)
    return tuple(float(F32(x)) for x in vals)


def step64(mode, p, g, m, v, t, lr, betas, eps, wd, grad_scale=1.0):
    assert p.dtype == m.dtype == v.dtype == F64
    lr_, b1, b2, omb1, omb2, eps_, wd_, bc1, bc2, gs = rounded_hyper(t, lr, betas, eps, wd, grad_scale)
    g = g.astype(F64) * gs
    if mode == L2_ON_GRAD:
        g = g + wd_ * p
    elif wd_ != 0.0:
        p -= lr_ * wd_ * p
    m[...] = b1 * m + omb1 * g
    v[...] = b2 * v + omb2 * (g * g)
    p -= lr_ * (m / bc1) / (np.sqrt(v / bc2) + eps_)


def plan(sizes):
    """(elements per block, blocks) of one multi-tensor launch over tensors of these sizes."""
    sizes = [int(n) for n in sizes]
    chunk = MT_CHUNK if sum(sizes) >= MT_LARGE_FROM else MT_CHUNK_SMALL
    return chunk, sum(-(-n // chunk) for n in sizes)


def worst_ratio(a, b, atol, rtol=RTOL):
    """max |a - b| / (atol + rtol |b|): <= 1 is what assert_allclose(a, b, rtol, atol) accepts."""
    a, b = np.asarray(a, F64).reshape(-1), np.asarray(b, F64).reshape(-1)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(b))))


# ------------------------------------------------------------------------------------------------------------------- the inputs
# grads[s][i]: tensor i's gradient at step s (None: no gradient, the optimizer skips it); t0: steps taken before; idx[i]: flat
# indices of tensor i that the references follow (None: all) -- the update is elementwise, so a sample of a large tensor is exact;
# over[s]: what step s changes of lr / wd / betas / grad_scale (the effective scale: grad_scale / divisor)
Scenario = collections.namedtuple("Scenario", "mode shapes p0 m0 v0 grads lr betas eps wd t0 idx over")

TAIL_SHAPES = [(1,), (3,), (4,), (5,), (1023,), (1027,), (1500,), (2047,), (2048,), (2049,), (4099,), (1000, 333)]
LARGE_SHAPES = [(2048, 2048), (16385,), (3,)]
# per-tensor entry: 2048 blocks x 256 threads x 2 unrolled float4 rounds, 300 float4 more, 3 elements; then the same past THREE
# grid strides, where threads 0..299 take a second unrolled trip and the others one single round
GRID_CAP_N = 2 * 2048 * 256 * 4 + 4 * 300 + 3
GRID_CAP_N2 = 3 * 2048 * 256 * 4 + 4 * 300 + 3
PER_TENSOR_SHAPES = [(GRID_CAP_N,), (1,), (3,), (4,), (1027,)]
PER_TENSOR_SHAPES2 = [(GRID_CAP_N2,)]
SKIP_SHAPES = [(33, 17), (40,), (17, 33)]
ZERO_MID_SHAPES = [(300,), (0,), (2049,)]
SCALE_SHAPES = [(37, 19), (2049,)]
DEV_SHAPES = [(2049,), (300,), (5,)]


def ends_and_stride(n, ends, stride=1021):
    return np.unique(np.concatenate([np.arange(ends), np.arange(n - ends, n), np.arange(0, n, stride)]))


def _normal(rng, shape):
    a = rng.standard_normal(shape).astype(F32)
    a.setflags(write=False)
    return a


def _build(name, mode):
    rng = np.random.default_rng([2301, sorted(SCENARIO_NAMES).index(name)])      # the same data for both modes
    kw = dict(mode=mode, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, t0=0, m0=None, v0=None, idx=None)
    steps, skip, over = 3, {}, {}
    if name == "tail":
        shapes = TAIL_SHAPES
    elif name == "large":
        shapes, kw["lr"] = LARGE_SHAPES, 1e-3
        n0 = int(np.prod(shapes[0]))
        kw["idx"] = [ends_and_stride(n0, MT_CHUNK + 8), None, None]
    elif name in ("per_tensor", "per_tensor2"):
        shapes, steps = (PER_TENSOR_SHAPES if name == "per_tensor" else PER_TENSOR_SHAPES2), 2
        kw["idx"] = [ends_and_stride(shapes[0][0], 16384)] + [None] * (len(shapes) - 1)
    elif name == "skip":
        shapes, skip = SKIP_SHAPES, {1: (1,)}                      # step index 1 (the second): tensor 1 has no gradient
    elif name == "zero_mid":
        shapes, steps = ZERO_MID_SHAPES, 2
    elif name == "scale":
        shapes, kw["lr"] = SCALE_SHAPES, 1e-3
        over = {s: dict(grad_scale=0.125) for s in range(3)}
    elif name == "dev_betas":                                      # other betas for two steps, then back
        shapes, steps, kw["lr"] = DEV_SHAPES, 6, 1e-3
        over = {2: dict(betas=(0.8, 0.99)), 3: dict(betas=(0.8, 0.99))}
    elif name == "dev_blocks":                                     # the 2049-element tensor (2 of the 4 blocks) sits out the second step
        shapes, steps, kw["lr"], skip = DEV_SHAPES, 4, 1e-3, {1: (0,)}
    elif name == "dev_hyper":                                      # lr, then weight decay, then grad_scale, a divisor, its new value
        shapes, steps, kw["lr"] = DEV_SHAPES, 6, 1e-3
        over = {1: dict(lr=3e-3), 2: dict(lr=3e-3, wd=5e-2), 3: dict(lr=3e-3, wd=5e-2, grad_scale=0.5),
                4: dict(lr=3e-3, wd=5e-2, grad_scale=0.125), 5: dict(lr=3e-3, wd=5e-2, grad_scale=0.25)}
    elif name in ("resume_1000", "resume_99990"):
        shapes, steps, kw["t0"], kw["lr"] = DEV_SHAPES, 5, int(name.split("_")[1]), 1e-3
    else:
        raise KeyError(name)
    p0 = [_normal(rng, s) for s in shapes]
    if kw["t0"]:                                                   # a state as training leaves it: m ~ g, v ~ g^2
        kw["m0"] = [_normal(rng, s) for s in shapes]
        kw["v0"] = [np.square(_normal(rng, s)) for s in shapes]
        for a in kw["v0"]:
            a.setflags(write=False)
    grads = [[None if i in skip.get(s, ()) else _normal(rng, shape) for i, shape in enumerate(shapes)] for s in range(steps)]
    return Scenario(shapes=shapes, p0=p0, grads=grads, over=[over.get(s, {}) for s in range(steps)], **kw)


SCENARIO_NAMES = ("tail", "large", "per_tensor", "per_tensor2", "skip", "zero_mid", "scale", "resume_1000", "resume_99990", "dev_betas",
                  "dev_blocks", "dev_hyper")
_cache = {}


def scenario(name, mode):
    """Built once, shared and read-only."""
    if (name, mode) not in _cache:
        _cache[name, mode] = _build(name, mode)
    return _cache[name, mode]


class Trace:
    """Both references side by side on a scenario's tensors (restricted to idx): p32 / m32 / v32 and p64 / m64 / v64, per tensor."""

    def __init__(self, sc):
        self.sc = sc
        self.t = sc.t0
        n = len(sc.shapes)
        zeros = [np.zeros(s, F32) for s in sc.shapes]
        self.p32 = [self.pick(i, sc.p0[i]).copy() for i in range(n)]
        self.m32 = [self.pick(i, (sc.m0 or zeros)[i]).copy() for i in range(n)]
        self.v32 = [self.pick(i, (sc.v0 or zeros)[i]).copy() for i in range(n)]
        self.p64, self.m64, self.v64 = ([a.astype(F64) for a in x] for x in (self.p32, self.m32, self.v32))

    def pick(self, i, a):
        a = np.asarray(a).reshape(-1)
        return a if self.sc.idx is None or self.sc.idx[i] is None else a[self.sc.idx[i]]

    def step(self):
        """The scenario's next optimizer step: every tensor with a gradient moves, the step count advances for all."""
        sc = self.sc
        s = self.t - sc.t0
        self.t += 1
        h = dict(lr=sc.lr, betas=sc.betas, eps=sc.eps, wd=sc.wd, grad_scale=1.0)
        h.update(sc.over[s])
        for i, g in enumerate(sc.grads[s]):
            if g is None or self.p32[i].size == 0:
                continue
            g = self.pick(i, g)
            step32(sc.mode, self.p32[i], g, self.m32[i], self.v32[i], self.t, **h)
            step64(sc.mode, self.p64[i], g, self.m64[i], self.v64[i], self.t, **h)

    def ratios(self):
        """Worst ratio of step32 against step64, (p, m, v)."""
        return tuple(max([worst_ratio(a, b, atol) for a, b in zip(x32, x64)] + [0.0])
                     for x32, x64, atol in ((self.p32, self.p64, ATOL[0]), (self.m32, self.m64, ATOL[1]), (self.v32, self.v64, ATOL[2])))
