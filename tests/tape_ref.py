"""Float64 restatements of the Tensor arithmetic (neunet/autograd.py:96-531, 588-640), the tier choice of csrc/tensor_ops.hip restated
as route(), the case tables of tests/test_tape_ops.py and tests/test_tape_ops_gpu.py, and the error bounds those tests hold.

Bounds (u = 2^-24, the unit roundoff of float32).
  maps     add, sub, mul are one correctly rounded operation, maximum / minimum are exact: |err| <= u |ref|.
           power goes through powf, div and the gradients of div / power through a few roundings: the bound the project holds its powf- and
           division-based maps to, rtol = atol = 1e-5 (tests/test_activations_losses_gpu.py: FIX).  Every elementwise gradient: FIX.
  sum      depth * u * sum |x_i|, depth the longest chain of additions an element's value can pass through in the tier's FIXED order:
             row-wave   a lane adds ceil(R / 64) values in turn (<= 16), then 4 DPP steps and a 2-level tree over four rows: R64 + 6
             row-block  a thread adds ceil(seg / 256) values, the wave tree (6), two levels over the four waves (2): + 8,
                        and the finishing lane adds the S partials in turn: + S - 1
             col        a wave's lane adds ceil(seg / 4) values, two levels over the four waves: + 2, and + S - 1 for the finish
             general    as row-block: ceil(seg / 256) + 8, + S - 1 for the finish
           For the gradient of a broadcast operand the x_i are the local gradients (float32 values with their own FIX-sized error,
           which the bound adds as rtol 1e-5 of sum |x_i|).
  mean     the sum bound / n plus one rounding of the product with 1 / n: + 2 u |mean|  (1 / n is itself rounded).
  var      with e = (depth + 1) u max |x| the error of a (segment) mean: M2 = sum (x - mean^)^2 = sum (x - mean)^2 + n e^2 exactly, each
           term carries three roundings and the chain `depth`: (depth + 3 + 4 S) u M2 + n e^2, and when the extent is split (S > 1) the
           merged between-segment term moves by at most 2 e sqrt(n M2) (Cauchy-Schwarz over the segments).  var = M2 / n: + u var.
           A single-pass E[x^2] - E[x]^2 at mean 1e4, std 1 is off by about u * 1e8 = 6: far outside.
  max/min  exact.  transpose / copy: exact.  matmul: the GEMM tier tests' bound (tests/gemm_ref.py).
"""
import itertools

import numpy as np

U = 2.0 ** -24
FIX = dict(rtol=1e-5, atol=1e-5)
BINARY = ("add", "sub", "mul", "div", "power", "maximum", "minimum")
UNARY = ("exp", "sqrt", "sin", "cos", "abs", "tanh")
REDUCE = ("sum", "mean", "var", "max", "min")
EXACT_BINARY = ("add", "sub", "mul", "maximum", "minimum")      # one rounding (or none); div and power: FIX

f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731


# ---- the ops ------------------------------------------------------------------------------------------------------------------------
def binary_forward(op, a, b):
    a, b = f64(a), f64(b)
    with np.errstate(all="ignore"):
        return {"add": lambda: a + b, "sub": lambda: a - b, "mul": lambda: a * b, "div": lambda: a / b, "power": lambda: a ** b,
                "maximum": lambda: np.maximum(a, b), "minimum": lambda: np.minimum(a, b)}[op]()


def unbroadcast(g, shape):
    """neunet/autograd.py:948-962."""
    g = f64(g)
    shape = tuple(shape)
    while g.ndim > len(shape):
        g = g.sum(0)
    axes = tuple(i for i, (s, e) in enumerate(zip(shape, g.shape)) if s == 1 and e != 1)
    return g.sum(axes, keepdims=True).reshape(shape) if axes else g.reshape(shape)


def binary_local_grads(op, a, b, g):
    """Full-shape local gradients (before the sum over the broadcast axes)."""
    a, b, g = f64(a), f64(b), f64(g)
    with np.errstate(all="ignore"):
        if op == "add":
            return g + 0 * (a + b), g + 0 * (a + b)
        if op == "sub":
            return g + 0 * (a + b), -g + 0 * (a + b)
        if op == "mul":
            return g * b + 0 * a, g * a + 0 * b
        if op == "div":
            return g / b + 0 * a, -g * a / b ** 2
        if op == "power":
            return g * b * a ** (b - 1), g * a ** b * np.log(a)
        if op == "maximum":
            return g * (a >= b), g * (a <= b)
        return g * (a <= b), g * (a >= b)


def binary_backward(op, a, b, g):
    la, lb = binary_local_grads(op, a, b, g)
    return unbroadcast(la, np.shape(a)), unbroadcast(lb, np.shape(b))


def unary_forward(op, x):
    x = f64(x)
    with np.errstate(all="ignore"):
        return getattr(np, op)(x)


def unary_backward(op, x, g):
    x, g = f64(x), f64(g)
    with np.errstate(all="ignore"):
        return g * {"exp": lambda: np.exp(x), "sqrt": lambda: 0.5 * x ** -0.5, "sin": lambda: np.cos(x), "cos": lambda: -np.sin(x),
                    "abs": lambda: np.sign(x), "tanh": lambda: 1 - np.tanh(x) ** 2}[op]()


def reduce_forward(op, x, axis=None, keepdims=False):
    return getattr(f64(x), op)(axis=axis, keepdims=keepdims)


def reduce_backward(op, x, axis, g):
    """g in the forward's output shape (either keepdims form)."""
    x = f64(x)
    kept = reduce_forward("sum", x, axis, True).shape
    g = f64(g).reshape(kept)
    n = x.size // max(int(np.prod(kept)), 1)
    if op == "sum":
        return np.broadcast_to(g, x.shape).copy()
    if op == "mean":
        return np.broadcast_to(g / n, x.shape).copy()
    if op == "var":
        return g * 2 * (x - x.mean(axis=axis, keepdims=True)) / n
    m = getattr(x, op)(axis=axis, keepdims=True)
    with np.errstate(invalid="ignore"):
        return g * (x == m)


def matmul_backward(a, b, g):
    """neunet/autograd.py:206-226 (the four cases), with the reverse broadcast of a shared right operand."""
    a, b, g = f64(a), f64(b), f64(g)
    if a.ndim > 1 and b.ndim > 1:
        return g @ np.swapaxes(b, -1, -2), unbroadcast(np.swapaxes(a, -1, -2) @ g, b.shape)
    if a.ndim == 1 and b.ndim == 1:
        return g * b, g * a
    if a.ndim == 1:
        return g @ b.T, np.outer(a, g)
    return np.outer(g, b), a.T @ g


# ---- the tier choice, restated ----------------------------------------------------------------------------------------------------------
MAX_RANK, MAX_GROUPS = 8, 6
WAVE_MAX_R, FILL_BLOCKS, ROW_SPLIT_MIN_R, ROW_SEG, COL_SPLIT_MIN_R, COL_SEG, MAX_S = 1024, 512, 8192, 4096, 256, 64, 256
GEN_SPLIT_MIN_R, GEN_SEG = 4096, 2048


def element_strides(shape, out_shape):
    """Strides (in elements) of a contiguous array of `shape` broadcast to `out_shape`, from NumPy's own broadcast view."""
    v = np.broadcast_to(np.empty(shape, np.float32), out_shape)
    return tuple(s // 4 for s in v.strides)


def groups(shape, strides_list, flags=None):
    """Axis groups after dropping extent-1 axes and merging neighbours: [(extent, (stride per operand), flag)]."""
    out = []
    for i, e in enumerate(shape):
        if e == 1:
            continue
        st, f = tuple(s[i] for s in strides_list), bool(flags[i]) if flags is not None else False
        if out and out[-1][2] == f and all(o == s * e for o, s in zip(out[-1][1], st)):
            out[-1] = (out[-1][0] * e, st, f)
        else:
            out.append((e, st, f))
    return out or [(1, tuple(0 for _ in strides_list), False)]


def route(kind, **kw):
    """The tier csrc/tensor_ops.hip picks.
    route("binary", sa=, sb=, aligned=True) -> 'same' | 'scalar' | 'inner' | 'outer' | 'vec2d' | 'general'
    route("reduce", shape=, axis=)           -> (tier, S): 'row-wave' | 'row-block' | 'col' | 'general'
    route("copy", shape=, strides=)           -> 'tile' | 'vec2d' | 'general'"""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    if kind == "binary":
        out_shape = np.broadcast_shapes(kw["sa"], kw["sb"])
        g = groups(out_shape, [element_strides(kw["sa"], out_shape), element_strides(kw["sb"], out_shape)])
        n = int(np.prod([e for e, _, _ in g]))
        full = [n == 1 or all(st[k] == int(np.prod([e for e, _, _ in g[i + 1:]])) for i, (_, st, _) in enumerate(g)) for k in (0, 1)]
        zero = [all(st[k] == 0 for _, st, _ in g) for k in (0, 1)]
        if full[0] and full[1]:
            return "same"
        if (full[0] and zero[1]) or (full[1] and zero[0]):
            return "scalar"
        vec = kw.get("aligned", True) and len(g) <= 2 and g[-1][0] % 4 == 0 and all(
            g[-1][1][k] in (0, 1) and (g[-1][1][k] == 0 or len(g) == 1 or g[0][1][k] % 4 == 0) for k in (0, 1))
        if not vec:
            return "general"
        if len(g) == 2 and (full[0] or full[1]):
            k = 1 if full[0] else 0
            if g[0][1][k] == 0 and g[1][1][k] == 1:
                return "inner"
            if g[1][1][k] == 0:
                return "outer"
        return "vec2d"
    if kind == "reduce":
        shape = tuple(kw["shape"])
        axis = kw["axis"]
        axes = tuple(range(len(shape))) if axis is None else tuple(a % len(shape) for a in ((axis,) if np.isscalar(axis) else axis))
        g = groups(shape, [element_strides(shape, shape)], [i in axes for i in range(len(shape))])
        pat = "".join("R" if f else "K" for _, _, f in g)
        if pat not in ("R", "K", "KR", "RK", "KRK"):
            nout, nred, S = int(np.prod([e for e, _, f in g if not f])), int(np.prod([e for e, _, f in g if f])), 1
            if nout < FILL_BLOCKS and nred >= GEN_SPLIT_MIN_R:
                S = min(cdiv(nred, GEN_SEG), cdiv(2 * FILL_BLOCKS, nout), MAX_S)
                S = cdiv(nred, cdiv(nred, S))
            return "general", S
        ko = g[0][0] if pat in ("KR", "KRK") else 1
        r = g[pat.index("R")][0] if "R" in pat else 1
        ki = g[-1][0] if pat in ("K", "RK", "KRK") else 1
        if ki == 1:
            if r <= WAVE_MAX_R:
                return "row-wave", 1
            S = 1
            if ko < FILL_BLOCKS and r >= ROW_SPLIT_MIN_R:
                S = min(cdiv(r, ROW_SEG), cdiv(2 * FILL_BLOCKS, ko), MAX_S)
                S = cdiv(r, cdiv(r, S))
            return "row-block", S
        nbx, S = cdiv(ki, 64), 1
        if ko * nbx < FILL_BLOCKS and r >= COL_SPLIT_MIN_R:
            S = min(cdiv(r, COL_SEG), cdiv(2 * FILL_BLOCKS, ko * nbx), MAX_S)
            S = cdiv(r, cdiv(r, S))
        return "col", S
    g = groups(kw["shape"], [kw["strides"]])
    if len(g) in (2, 3) and g[-2][1][0] == 1 and g[-1][1][0] != 1:
        return "tile"
    vec = kw.get("aligned", True) and len(g) <= 2 and g[-1][0] % 4 == 0 and g[-1][1][0] in (0, 1) and \
        (g[-1][1][0] == 0 or len(g) == 1 or g[0][1][0] % 4 == 0)
    return "vec2d" if vec else "general"


def sum_depth(shape, axis):
    """Longest addition chain of the tier that reduces `shape` over `axis` (module docstring)."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    tier, S = route("reduce", shape=shape, axis=axis)
    axes = tuple(range(len(shape))) if axis is None else tuple(a % len(shape) for a in ((axis,) if np.isscalar(axis) else axis))
    n = int(np.prod([shape[a] for a in axes])) if axes else 1
    seg = cdiv(n, S)
    if tier == "row-wave":
        return cdiv(n, 64) + 6
    if tier == "row-block":
        return cdiv(seg, 256) + 8 + S - 1
    if tier == "col":
        return cdiv(seg, 4) + 2 + S - 1
    return cdiv(seg, 256) + 8 + S - 1


def sum_bound(x, axis, keepdims=False, extra_rtol=0.0):
    x = f64(x)
    shape = x.shape
    return (sum_depth(shape, axis) * U + extra_rtol) * np.abs(x).sum(axis=axis, keepdims=keepdims) + 1e-45


def mean_bound(x, axis, keepdims=False):
    x = f64(x)
    n = x.size // max(x.sum(axis=axis).size, 1)
    return sum_bound(x, axis, keepdims) / n + 2 * U * np.abs(x.mean(axis=axis, keepdims=keepdims))


def var_bound(x, axis, keepdims=False):
    x = f64(x)
    _, S = route("reduce", shape=x.shape, axis=axis)
    depth = sum_depth(x.shape, axis)
    n = x.size // max(x.sum(axis=axis).size, 1)
    m2 = x.var(axis=axis, keepdims=keepdims) * n
    e = (depth + 1) * U * np.abs(x).max(axis=axis, keepdims=keepdims)
    b = (depth + 3 + 4 * S) * U * m2 + n * e * e + (2 * e * np.sqrt(n * m2) if S > 1 else 0.0)
    return b / n + U * m2 / n + 1e-45


# ---- case tables ----------------------------------------------------------------------------------------------------------------------
INNER_EXTENTS = (1, 3, 4, 5, 63, 64, 65, 257)
RANK6 = ((2, 1, 3, 1, 2, 5), (1, 4, 1, 3, 1, 5))
# (shape a, shape b): every tier of the binary forward; the tier each must reach is route()'s answer, pinned in BINARY_TIERS
BINARY_CASES = [((9, 8), (9, 8)), ((9, 8), (8,)), ((9, 8), (9, 1)), ((8,), (9, 8)), ((9, 1), (9, 8)), ((9, 5), (5,)), ((9, 5), (9, 1)),
                ((9, 8), ()), ((), (9, 8)), ((9, 8), (1,)), ((1, 1), (9, 8)), ((), ()), ((1,), ()), ((9, 1), (1, 8)), RANK6,
                ((2, 3, 4), (3, 1)), ((3, 4, 8), (4, 1))]
BINARY_TIERS = ["same", "inner", "outer", "inner", "outer", "general", "general", "scalar", "scalar", "scalar", "scalar", "same", "same",
                "vec2d", "general", "general", "general"]
# (shape, axis): every reduction tier, extents at each boundary - 1, 0, + 1
REDUCE_CASES = [((5, 1), 1), ((1, 7), 1), ((5, 7), 1), ((3, 1023), 1), ((3, 1024), 1), ((3, 1025), 1), ((3, 8191), 1), ((3, 8192), 1),
                ((3, 8193), 1), ((512, 1025), 1), ((8193,), None), ((70001,), None), ((2, 3, 5, 7), None),
                ((7, 5), 0), ((255, 65), 0), ((256, 65), 0), ((257, 63), 0), ((300, 1), 0), ((2, 255, 3), 1), ((3, 257, 65), 1), ((2, 9, 1), 1),
                ((5, 3, 70), (0, 1)), ((4, 3, 5), (-2,)), ((3, 5, 7), (-1, 1)),
                ((2, 3, 5, 7), (0, 2, 3)), ((2, 3, 4, 5, 6), (1, 3)), ((4, 3, 1023), (0, 2)), ((4, 3, 1024), (0, 2))]
REDUCE_TIERS = [("col", 1), ("row-wave", 1), ("row-wave", 1), ("row-wave", 1), ("row-wave", 1), ("row-block", 1), ("row-block", 1),
                ("row-block", 2), ("row-block", 3), ("row-block", 1), ("row-block", 3), ("row-block", 18), ("row-wave", 1),
                ("col", 1), ("col", 1), ("col", 4), ("col", 5), ("row-wave", 1), ("col", 1), ("col", 5), ("row-wave", 1),
                ("col", 1), ("col", 1), ("row-wave", 1),
                ("general", 1), ("general", 1), ("general", 1), ("general", 2)]
TRANSPOSE_2D = (1, 31, 32, 33, 65)
TRANSPOSE_4D = (((2, 3, 5, 7), (0, 2, 1, 3)), ((2, 3, 5, 7), (0, 3, 1, 2)))


def shapes_up_to_rank4():
    for rank in range(0, 5):
        yield from itertools.product((1, 2, 3), repeat=rank)
