"""References for the gradient-norm / clipping kernels of csrc/grad_norm.hip (nnhipGradNormMultiTensor, nnhipScaleMultiTensor):
NumPy only, independent of the kernels.

Float64 restatement (`words64`).  With gs = float32(grad_scale) / float32(divisor_in) -- the factor the update kernels apply to a
gradient, formed in float32 as adam_dev_resolve forms it -- the entry is asked for
    norm    = |gs| * sqrt(sum g^2)          (norm_type 2)        or      |gs| * max |g|          (norm_type inf)
    divisor = d_in * max(1, (norm + 1e-6) / max_norm)
    flag    = 1 when the norm is NaN or inf, else 0
which is torch.nn.utils.clip_grad_norm_'s arithmetic on the effective gradient g * gs (tests/test_gradclip.py holds it to torch).

Derived bound for the L2 norm (`l2_rel_bound`) -- a derivation from the kernel's summation tree, restated below, NOT a measurement.
Every term of S = sum g^2 is non-negative, so a float32 summation has no cancellation: if an element passes through a chain of at
most d float32 additions, the computed S differs from the exact one by at most (d + 1) * 2^-24 relative, to first order (the extra 1
is the rounding of the square).  The kernel's chain, for a block of 256 lanes (4 waves of 64) on a chunk of C elements:
    C / (256 * 4)   additions into one of a lane's four accumulators (16 at the 16384-element chunk, 2 at the 2048-element one)
    2               the lane's four accumulators joined pairwise
    6               cross-lane steps: a balanced pairwise tree over the 64 lanes
    4               the block's waves (three additions; counted as the number of waves)
and the blocks' sums are added in double, which adds nothing at this scale.  The norm is sqrt(S): half the relative error of S, plus
three float32-size roundings -- the square root (taken in double), the conversion to float32 and the multiplication by |gs|.
    |norm - norm64| <= ((d + 1) / 2 + 3) * 2^-24 * norm64

The max norm is exact: float32(|gs|) * float32(max |g|), one float32 multiplication, bit for bit (`inf_norm32`).
The divisor word, recomputed in float32 from the RETURNED norm word (`divisor32`), agrees within 4 * 2^-24 relative: the addition, the
division, the multiplication and the conversion of max_norm to float32.

`emulate_l2` restates the kernel's summation ORDER in float32 NumPy (element e of a chunk goes to lane (e / 4) % 256, accumulator
e % 4, in increasing order; then the tree above; then the blocks in double: lane t takes blocks t, t + 256, ..., the lanes combine in a
butterfly, the waves in order).  The kernel is compiled without contraction, so on a device it gives these bits."""
import numpy as np

EPS = 2.0 ** -24
MT_CHUNK, MT_CHUNK_SMALL, BIG_TOTAL = 16384, 2048, 1 << 22        # csrc/optim.hip: the plan's chunk rule
BLOCK, WAVE, ACCS = 256, 64, 4                                    # csrc/grad_norm.hip: lanes per block, per wave, accumulators per lane
NORM_L2, NORM_INF = 0, 1                                          # include/neunet_hip.h: NNHIP_NORM_*
DIVISOR_RTOL = 4 * EPS

MLP_SIZES = [128 * 784, 128, 10 * 128, 10]                        # the README MLP: Linear(784, 128), Linear(128, 10)
# (name, tensor sizes, elements the first tensor's view starts past a 16-byte boundary)
CASES = [
    ("one", [1], 0),                                              # smallest input
    ("three", [3], 0),                                            # smallest unaligned tail
    ("chunk_edges", [2047, 2048, 2049], 0),                       # small-chunk edges
    ("zero_inside", [5, 0, 7], 0),                                # a zero-size tensor in the list
    ("blocks64", [2048] * 64, 0),                                 # 64 blocks, every XCD several times: the cross-XCD finish
    ("big_tail", [2 ** 22 + 5], 0),                               # the 16384-element chunk, 257 blocks, a 5-element tail
    ("misaligned", [4099], 1),                                    # 4 bytes off a 16-byte boundary: the scalar-load path, 3 blocks
    ("mlp", MLP_SIZES, 0),                                        # a real small model
]
CASE_NAMES = [c[0] for c in CASES]


def case(name):
    return next(c for c in CASES if c[0] == name)


def make_grads(name, seed, scale=1.0):
    """The case's gradients: standard normal float32, seeded by (case, seed)."""
    _, sizes, _ = case(name)
    rng = np.random.default_rng([CASE_NAMES.index(name), seed])
    return [(rng.standard_normal(n, dtype=np.float32) * np.float32(scale)) for n in sizes]


def chunk_of(sizes):
    return MT_CHUNK if sum(sizes) >= BIG_TOTAL else MT_CHUNK_SMALL


def plan(sizes):
    """[(tensor, chunk index)] per block, and the chunk size: fused_optimizer_plan restated."""
    chunk = chunk_of(sizes)
    return [(i, c) for i, n in enumerate(sizes) for c in range(-(-n // chunk))], chunk


def depth(chunk):
    """The longest chain of float32 additions an element passes through."""
    return chunk // (BLOCK * ACCS) + 2 + 6 + BLOCK // WAVE


def l2_rel_bound(sizes):
    return ((depth(chunk_of(sizes)) + 1) / 2 + 3) * EPS


def gs32(grad_scale, d_in):
    gs = np.float32(grad_scale)
    return gs if d_in is None else np.float32(gs / np.float32(d_in))


def norm64(grads, norm_type, grad_scale=1.0, d_in=None):
    gs = abs(float(gs32(grad_scale, d_in)))
    flat = [np.asarray(g, np.float64).ravel() for g in grads if np.size(g)]
    if not flat:
        return 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        if norm_type == NORM_L2:
            return gs * float(np.sqrt(sum(float(np.sum(f * f)) for f in flat)))
        m = [float(np.max(np.abs(f))) if not np.isnan(f).any() else float("nan") for f in flat]
        return gs * (float("nan") if any(np.isnan(v) for v in m) else max(m))


def divisor64(norm, max_norm, d_in=None):
    d = 1.0 if d_in is None else float(np.float32(d_in))
    ratio = (norm + 1e-6) / float(max_norm)
    return d * (ratio if (ratio > 1.0 or np.isnan(ratio)) else 1.0)


def words64(grads, norm_type, max_norm, grad_scale=1.0, d_in=None):
    """(norm, divisor, flag) in float64."""
    n = norm64(grads, norm_type, grad_scale, d_in)
    return n, divisor64(n, max_norm, d_in), 0.0 if np.isfinite(n) else 1.0


def divisor32(norm_word, max_norm, d_in=None):
    """The divisor word from the returned norm word, every operation in float32."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = np.float32(1.0) if d_in is None else np.float32(d_in)
        ratio = np.float32(np.float32(np.float32(norm_word) + np.float32(1e-6)) / np.float32(max_norm))
        return np.float32(d * (ratio if (ratio > 1 or np.isnan(ratio)) else np.float32(1.0)))


def inf_norm32(grads, grad_scale=1.0, d_in=None):
    flat = [np.abs(np.asarray(g, np.float32).ravel()) for g in grads if np.size(g)]
    m = np.float32(max(float(f.max()) for f in flat)) if flat else np.float32(0)
    return np.float32(np.abs(gs32(grad_scale, d_in)) * m)


def _tree(v):
    """Balanced pairwise tree over the last axis (neighbours first): the DPP wave reduction."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def emulate_l2_partials(grads):
    """The float32 value each block leaves in its slot, in block order."""
    sizes = [int(np.size(g)) for g in grads]
    chunk = chunk_of(sizes)
    out = []
    for g in grads:
        g = np.asarray(g, np.float32).ravel()
        nb = -(-g.size // chunk)
        if nb == 0:
            continue
        buf = np.zeros(nb * chunk, np.float32)                    # zero padding: x + 0 = x, so absent elements change nothing
        buf[:g.size] = g
        sq = (buf * buf).reshape(nb, chunk // (BLOCK * ACCS), BLOCK, ACCS)       # the square is rounded before it is added
        acc = np.zeros((nb, BLOCK, ACCS), np.float32)
        for r in range(sq.shape[1]):
            acc = acc + sq[:, r]
        lane = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
        wave = _tree(lane.reshape(nb, BLOCK // WAVE, WAVE))
        blk = wave[:, 0]
        for w in range(1, BLOCK // WAVE):
            blk = blk + wave[:, w]
        assert blk.dtype == np.float32
        out.append(blk)
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def emulate_l2(grads, grad_scale=1.0, d_in=None):
    """The norm word, bit for bit as the kernel's order of operations gives it."""
    with np.errstate(over="ignore", invalid="ignore"):
        part = emulate_l2_partials(grads).astype(np.float64)
        lanes = np.zeros(BLOCK, np.float64)
        for b in range(part.size):                                # lane t: blocks t, t + 256, ... in increasing order
            lanes[b % BLOCK] += part[b]
        v = lanes.reshape(BLOCK // WAVE, WAVE)
        k = WAVE // 2
        while k >= 1:                                             # the butterfly, as lane 0 sees it
            v = v[:, :k] + v[:, k:2 * k]
            k //= 2
        s = ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]
        return np.float32(np.abs(gs32(grad_scale, d_in)) * np.float32(np.sqrt(s)))
