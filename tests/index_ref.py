"""NumPy / float64 restatements of the indexing half of the Tensor tape (neunet/autograd.py:642-808, 895-923), the case tables of
tests/test_tape_index.py and tests/test_tape_index_gpu.py, and the cases of the fixture tests/golden/tape_index.npz
(tools/gen_golden.py: gen_tape_index runs them on the reference, the tests run the same functions on neunet_hip).

Everything but one family is a copy, a select or a comparison and therefore EXACT: the tests ask for bit equality with NumPy.  The one
inexact family is the gradient of a `where` operand that was broadcast -- a sum of the selected gradients over the broadcast axes --
and it is held to the sum bound tests/tape_ref.py derives for the reduction tiers (sum_bound: depth * u * sum |x_i|); no new constant.
"""
import math

import numpy as np

FIX = "tape_index"                      # tests/golden/tape_index.npz
COMPARE = ("equal", "not_equal", "greater", "greater_equal", "less", "less_equal")
NP_COMPARE = {"equal": np.equal, "not_equal": np.not_equal, "greater": np.greater, "greater_equal": np.greater_equal, "less": np.less,
              "less_equal": np.less_equal}
LOGICAL = ("logical_and", "logical_or", "logical_not")
# NNHIP_TIER_* of csrc/tensor_index.hip (include/neunet_hip.h), next to the elementwise and reduction tiers of tensor_ops.h
TIER = {"vec4": 20, "general": 21, "slice-vec": 22, "slice-scalar": 23, "row-vec": 24, "row": 25, "element": 26,
        "ew-vec2d": 3, "ew-general": 4, "red-row-wave": 10, "red-row-block": 11, "red-col": 12, "red-general": 13}
DT = {np.dtype(np.float32): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.bool_): 3, np.dtype(np.uint8): 3}


# ---- restatements -----------------------------------------------------------------------------------------------------------------------
def apply_descriptor(shape, offset, out_shape, strides):
    """What (offset, out_shape, strides) selects from np.arange(n).reshape(shape): the flat elements at offset + c . strides."""
    flat = np.arange(int(np.prod(shape, dtype=np.int64)), dtype=np.int64)
    if int(np.prod(out_shape, dtype=np.int64)) == 0:
        return np.zeros(out_shape, np.int64)
    lin = np.full(out_shape, offset, np.int64)
    for ax, (e, s) in enumerate(zip(out_shape, strides)):
        assert s != 0, "a stride of 0"
        lin += (np.arange(e, dtype=np.int64) * s).reshape((1,) * ax + (e,) + (1,) * (len(out_shape) - ax - 1))
    return flat[lin]


def lattice_scatter(shape, start, step, count, grad):
    """dX of nnhipSliceBackward: grad laid on the lattice start + j * step (0 <= j < count per axis), 0 elsewhere."""
    out = np.zeros(shape, np.asarray(grad).dtype)
    if all(c > 0 for c in count):
        idx = np.ix_(*[np.asarray([s + j * st for j in range(c)], np.int64) for s, st, c in zip(start, step, count)])
        out[idx] = np.asarray(grad).reshape(count)
    return out


def getitem_backward(shape, key, grad):
    """The reference's backward of x[key]: ASSIGN into zeros (for repeated indices the last occurrence in C order stays)."""
    out = np.zeros(shape, np.asarray(grad).dtype)
    out[key] = grad
    return out


def unbroadcast64(g, shape):
    """Sum a full-shape float64 array over the axes along which an operand of `shape` was broadcast."""
    g = np.asarray(g, np.float64)
    shape = tuple(shape)
    while g.ndim > len(shape):
        g = g.sum(0)
    axes = tuple(i for i, (s, e) in enumerate(zip(shape, g.shape)) if s == 1 and e != 1)
    return g.sum(axes, keepdims=True).reshape(shape) if axes else g.reshape(shape)


def where_backward(cond, g, shape_a, shape_b):
    """(dA, dB, |terms of dA|, |terms of dB|): selects (never products: an inf or NaN of g where the operand did not supply the value
    contributes exactly 0), each summed in float64 over its operand's broadcast axes; the absolute sums feed the bound."""
    truth = np.asarray(cond) != 0
    g = np.asarray(g, np.float64)
    truth = np.broadcast_to(truth, g.shape)
    la, lb = np.where(truth, g, 0.0), np.where(truth, 0.0, g)
    return unbroadcast64(la, shape_a), unbroadcast64(lb, shape_b), unbroadcast64(np.abs(la), shape_a), unbroadcast64(np.abs(lb), shape_b)


def reduced_axes(shape, full):
    """The (shape, axes) of the reduction that forms the gradient of an operand of `shape` broadcast to `full`: what
    tape_ref.sum_bound wants.  None when the operand was not broadcast."""
    pad = (1,) * (len(full) - len(shape)) + tuple(shape)
    axes = tuple(i for i, (s, e) in enumerate(zip(pad, full)) if s == 1 and e != 1)
    return axes or None


# ---- case tables ----------------------------------------------------------------------------------------------------------------------
COMPARE_SIZES = (1, 3, 4, 255, 257, 1028)               # n % 4 != 0 and n % 4 == 0, below / above one block of 256 lanes x 4
COMPARE_BROADCAST = [((5, 7), (7,)), ((5, 7), (5, 1)), ((7,), (5, 7)), ((2, 1, 5, 5), (2, 3, 5, 5))]
F32_SPECIALS = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, 1.0, -1.0, 3.4028235e38, 0.5], np.float32)
BASIC_SHAPES = [(6,), (5, 7), (2, 3, 4), (3, 1, 5, 2)]
BASIC_KEYS = [2, -1, (slice(None), -1), slice(1, 5, 2), slice(None, None, -1), (slice(None, None, -2), slice(1, None, 3)),
              (Ellipsis, None), (slice(None), None, Ellipsis), slice(3, 3), slice(None, None, 9), (1, Ellipsis, 0),
              slice(None, None, -9), (slice(None), slice(None, None, 2)), slice(-2, None), (Ellipsis, slice(None, None, -1))]
FLIP_AXES = [None, 0, -1, (0, 2)]
GATHER_INNER = (1, 5, 16, 67, 260)                      # element | general | row-vec | row (67 % 4 != 0) | row-vec past one pass of 64 lanes x 4
WHERE_BACKWARD_SHAPES = [(3, 5), (33, 260)]


def basic_cases():
    """(shape, key) pairs of BASIC_SHAPES x BASIC_KEYS that NumPy accepts."""
    out = []
    for shape in BASIC_SHAPES:
        for key in BASIC_KEYS:
            try:
                np.zeros(shape)[key]
            except IndexError:
                continue
            out.append((shape, key))
    return out


def key_id(key):
    def one(k):
        if isinstance(k, slice):
            return ":".join("" if v is None else str(v) for v in (k.start, k.stop, k.step))
        return {None: "None", Ellipsis: "..."}.get(k, str(k)) if not isinstance(k, (list, np.ndarray)) else "arr"
    return "[" + ",".join(one(k) for k in (key if isinstance(key, tuple) else (key,))) + "]"


def random_key(rng, rank):
    """A random basic key for the fuzz (python's random.Random): ints and slice bounds reach past the extents (1..7) on both sides."""
    items = []
    for _ in range(rng.randint(0, rank + 1)):
        r = rng.random()
        if r < 0.35:
            items.append(rng.randint(-8, 8))
        elif r < 0.8:
            bound = lambda: rng.choice([None] + list(range(-9, 10)))  # noqa: E731
            items.append(slice(bound(), bound(), rng.choice([None, 1, 2, 3, -1, -2, -3, 9, -9])))
        elif r < 0.9:
            items.append(None)
        else:
            items.append(Ellipsis)
    return items[0] if len(items) == 1 and rng.random() < 0.3 else tuple(items)


# ---- the fixture's cases: functions of (module, device, *tensors) that run unchanged on the reference and on neunet_hip ----------------------
# input kinds: f float32 that requires a gradient | c float32 constant | h float32 constant rounded to halves (ties, zeros)
#              m int32 0 / 1 constant | M the composition's padding mask (one row fully masked)
def draw(rng, spec):
    shape, kind = spec
    if kind in "fc":
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "h":
        return (np.round(rng.standard_normal(shape) * 2) / 2).astype(np.float32)
    m = (rng.random(shape) < 0.6).astype(np.int32)
    if kind == "M":
        m[0, 2, :] = 0
        m[1, :, 0] = 1
    return m


LABELS = np.array([1, 4, 0, 4, 2, 3], np.int64)
IDS = np.array([[1, 3, 1], [0, 3, 6]], np.int64)


def _positional(nn, dev, x):
    """x [B, T, D] plus the first T rows of a sinusoidal table [L, D]: table[l, 2 j] = sin(l w_j), table[l, 2 j + 1] = cos(l w_j),
    w_j = 10000^(-2 j / D).  Built the way user code on the tape builds it: zeros, arange, a new axis, two strided assignments, a leading
    axis, a slice of the rows."""
    rows, width, steps = 6, x.shape[2], x.shape[1]
    rates = nn.exp(nn.arange(0, width, 2, device=dev) * (-math.log(10000.0) / width))
    angles = nn.arange(0, rows, dtype=np.float32, device=dev)[:, None, ...] * rates
    table = nn.zeros(rows, width, device=dev)
    table[:, 0::2] = nn.sin(angles)
    table[:, 1::2] = nn.cos(angles)
    return x + table[None, ...][:, :steps]


def _masked_scores(nn, dev, scores, mask, w):
    s = nn.where(mask[:, None, ...] == 0, -1e9, scores)
    e = (s - s.max(axis=-1, keepdims=True)).exp()
    return ((e / e.sum(axis=-1, keepdims=True)) * w).sum(axis=-1)


def _key(nn, t):
    """A comparison's result used as a key: neunet_hip takes the bool Tensor as it is; the reference's comparisons leave float32
    0 / 1 arrays (its Tensor constructor converts), which index its NumPy array as a boolean mask."""
    return t if nn.__name__ == "neunet_hip" else t.data.astype(np.bool_)


def _assigned(x, key, value):
    x[key] = value
    return x


def tape_index_cases():
    """{tag: (input specs, fn(nn, dev, *tensors) -> Tensor)}."""
    A, B5, C41, X = ((4, 5), "h"), ((5,), "h"), ((4, 1), "h"), ((3, 4, 5), "f")
    c = {}
    for op in COMPARE:
        c[f"{op}_row"] = ((A, B5), lambda nn, dev, a, b, op=op: getattr(a, op)(b))
        c[f"{op}_scalar"] = ((A,), lambda nn, dev, a, op=op: getattr(a, op)(0.5))
    c["equal_int_mask"] = ((((4, 5), "m"),), lambda nn, dev, m: m == 0)
    c["logical_and"] = ((A, B5), lambda nn, dev, a, b: (a > 0) & (b < 0.5))
    c["logical_or"] = ((A, C41), lambda nn, dev, a, b: (a > 0) | (b > 0))
    c["logical_not"] = ((A,), lambda nn, dev, a: ~(a >= 0))
    c["logical_float"] = ((A, B5), lambda nn, dev, a, b: a.logical_and(b))
    c["where_row"] = ((((4, 5), "f"), A, ((5,), "f")), lambda nn, dev, a, h, b: a.where(h > 0, b))
    c["where_col_scalar"] = ((((4, 1), "f"), A), lambda nn, dev, a, h: a.where(h != 0, 2.5))
    c["where_function"] = ((((4, 5), "m"), ((4, 5), "f")), lambda nn, dev, m, a: nn.where(m == 0, -1e9, a))
    for i, ax in enumerate(FLIP_AXES):
        c[f"flip_{i}"] = ((X,), lambda nn, dev, x, ax=ax: x.flip(ax))
    keys = [2, (slice(None), -1), slice(None, None, -1), (slice(None, None, -2), slice(1, None, 3)), (Ellipsis, None), (1, Ellipsis, 0),
            [2, 0, 2], (slice(None), [1, 3, 1]), (Ellipsis, [0, 0, 3]), (np.array([0, 2, 2]), np.array([3, 1, 3])),
            (slice(None), np.array([[0], [3]]), np.array([[4, 1, 4]]))]
    for i, key in enumerate(keys):
        c[f"getitem_{i}"] = ((X,), lambda nn, dev, x, key=key: x[key])
    Xc, V45 = ((3, 4, 5), "c"), ((4, 5), "c")
    c["setitem_scalar"] = ((Xc,), lambda nn, dev, x: _assigned(x, (slice(None), slice(None, None, 2)), 2.5))
    c["setitem_rows"] = ((Xc, V45), lambda nn, dev, x, v: _assigned(x, 1, v))
    c["setitem_broadcast"] = ((Xc, ((5,), "c")), lambda nn, dev, x, v: _assigned(x, (slice(None, None, -2), slice(1, 3)), v))
    c["setitem_ids"] = ((Xc, ((3, 4, 5), "c")), lambda nn, dev, x, v: _assigned(x, [0, 2, 0], v))
    c["setitem_mask"] = ((Xc, ((3, 4), "m")), lambda nn, dev, x, m: _assigned(x, _key(nn, m == 1), 0.0))
    # the compositions
    c["masked_scores"] = ((((2, 2, 5, 5), "f"), ((2, 5, 5), "M"), ((2, 2, 5, 5), "c")), _masked_scores)
    c["positional"] = ((((2, 4, 8), "f"),), _positional)
    c["last_step"] = ((((2, 4, 6), "f"),), lambda nn, dev, out: out[:, -1] / 0.7)
    c["nll"] = ((((6, 5), "f"),), lambda nn, dev, logp: -(logp[np.arange(6), LABELS]).mean())
    c["embedding"] = ((((7, 4), "f"),), lambda nn, dev, w: w[IDS])
    c["flip_squares"] = ((((3, 4), "f"), ((3, 4), "c")), lambda nn, dev, x, w: ((x.flip(1) * w) ** 2).sum())
    return c


COMPOSITIONS = ("masked_scores", "positional", "last_step", "nll", "embedding", "flip_squares")
