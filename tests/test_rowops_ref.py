"""CPU: the float64 restatements of tests/rowops_ref.py against what the project already trusts -- the reference's fixtures under
tests/golden/ (at the tolerances the GPU golden tests of tests/test_hip_parity.py use for them) and oracle/neunet_oracle.py on the
input makers defined here -- each one also shown to REJECT the wrong variant of its rule that it was held against; and the argument
refusals of the C entries of csrc/rowops.hip, csrc/embedding.hip and csrc/elementwise.hip (status codes, no GPU needed: every refusal
happens before a launch).

This file also holds the shape tables and the input makers of tests/test_rowops_tiers_gpu.py and tests/test_gather_elementwise_gpu.py,
so that what the restatements were checked on here is what the kernels are checked on there."""
import numpy as np
import pytest

from oracle import neunet_oracle as O
from rowops_ref import (MASKED, cross_entropy, dropout_keep, embedding_backward, embedding_forward, embedding_rows, gelu, gelu_backward,
                        masked_positions, masked_softmax_backward, masked_softmax_forward, relu_backward, relu_forward, rmsnorm_backward,
                        rmsnorm_forward, softmax_backward, softmax_forward, swiglu, swiglu_backward, swish, swish_backward)
from test_hip_parity import rms_of

EPS = 1e-6
EINVAL, EALIGN = -1, -2


# ============================================================================================ dispatch, restated
def row_tier(cols):
    """row_tier() of csrc/rowops.hip: (threads per row) x (float4 per thread), or the looped kernels above 16384 columns."""
    for limit, name in ((256, "64x1"), (512, "64x2"), (1024, "64x4"), (4096, "256x4"), (8192, "256x8"), (16384, "1024x4")):
        if cols <= limit:
            return name
    return "looped"


def row_variant(cols, off=0, ld=None):
    """The kernel variant a contiguous row op takes: float4 when cols % 4 == 0, every pointer is 16-byte aligned (off = 0: the operands
    start at their allocations; off = 1: four bytes in) and -- CrossEntropy only -- the row pitch ld % 4 == 0."""
    tier = row_tier(cols)
    if tier == "looped":
        return "looped"
    vec = cols % 4 == 0 and off == 0 and (ld is None or ld % 4 == 0)
    return tier + ("-vec" if vec else "-scalar")


def case_id(cols, off=0, rows=None):
    return (f"{rows}x" if rows is not None else "") + f"{cols}-{row_variant(cols, off)}" + ("-off1" if off else "")


# ---- plain Softmax: (cols, off)
SOFTMAX_ROWS = 9
SOFTMAX_CASES = ([(c, 0) for c in (256, 260, 512, 516, 1024, 1028, 4096, 4100, 8192, 8196, 16384)] +      # float4, both sides of each edge
                 [(c, 0) for c in (6, 255, 510, 1001, 2050, 4099, 8190, 12001)] +                          # scalar by width
                 [(c, 1) for c in (256, 4096, 16384)] +                                                    # scalar by alignment
                 [(c, 0) for c in (16385, 20000)])                                                         # looped
SOFTMAX_STRIDED = [(3, 7, 300), (3, 1, 300)]         # (outer, slice, stride): 900 slices = four 256-thread blocks, the last ragged

# ---- masked Softmax
MASKED_B, MASKED_H, MASKED_TQ = 2, 3, 5              # 30 rows: ragged for four rows per block; H > 1: row / (H Tq) != row / Tq
MASKED_TK = (7, 256, 260, 510, 1001, 1024, 1028, 2050, 4100, 8190, 8192, 12000, 12001, 16384)   # 1001, 12001: the scalar 64x4 and 1024x4
MASK_MODES = ("none", "key_valid", "dense", "causal", "all")
MASKED_TQ_NE_TK = [(9, 7), (3, 260)]                 # causal with Tq > Tk (the first rows see nothing) and Tq < Tk
MASKED_OFF1 = (256, 4096, 16384)                     # one per block size: 256 (4 rows), 256 (1 row), 1024

# ---- RMSNorm
RMS_ROWS = 9
RMS_CASES = [(c, 0) for c in (510, 1001, 2050, 4099, 8190, 12001, 16388)] + [(1024, 1), (4096, 1)]

# ---- CrossEntropy: the smallest shapes that leave ce_small_kernel (rows * cols > 65536 or cols > 4096)
CE_SHAPES = [(260, 256), (260, 255), (132, 512), (131, 510), (66, 1024), (68, 1001), (17, 4096), (33, 2050),
             (2, 8192), (3, 4099), (2, 16384), (3, 12001), (2, 16388), (3, 20001)]
CE_MULTI_ROUND = [(12293, 260), (12293, 258), (2053, 4100)]


def ce_kernel(rows, cols, ld=None, off=0):
    """ce_launch() of csrc/rowops.hip, restated: which kernel a problem reaches and with how many blocks at the most."""
    if rows * cols <= 65536 and cols <= 4096:
        return "small"
    v = row_variant(cols, off, cols if ld is None else ld)
    blocks = -(-rows // (4 if cols <= 1024 else 1))
    return v + ("-2blocks" if blocks == 2 else "")


def ce_id(shape):
    return f"{shape[0]}x{shape[1]}-{ce_kernel(*shape)}"


# ---- Embedding: (V, D, n_ids, T)
EMBEDDING_CASES = [(1, 1, 1, 1), (97, 3, 5, 5), (97, 48, 257, 33), (1001, 260, 64, 64), (50, 1026, 9, 3), (4, 256, 300, 300)]

# ---- maps
MAP_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 16387)    # one block's span is 256 threads x 4 float4 = 4096 floats
SWIGLU_CASES = [(1, 5, 0), (3, 5, 0), (4, 5, 0), (132, 5, 0), (64, 70, 0), (4, 5, 1), (132, 5, 1)]      # (h, rows, off)
DROPOUT_SIZES = (1, 5, 4099, 70001)
DROPOUT_P = (0.0, 0.1, 0.5, 1.0)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 2.0 ** -126, 1.0, -1.0, 3.5, -2.25, 1e38], np.float32)


# ============================================================================================ input makers
def softmax_inputs(rows, cols, seed, lift=0.0):
    """Scores of spread 2 with one row lifted by 40 (the max subtraction must carry it) and, in the last row, one dominant entry; an
    upstream gradient of either sign.  The dominant entry is set to the log-sum-exp of the rest of its row (+ lift), so it holds
    half of the row's mass at any width -- short of saturation: at y = 1 - 1e-5 the backward's dy - sum(dy y) cancels to the rounding
    noise of dy in ANY float32 evaluation of the formula, the oracle's included (test_saturated_softmax_row_is_beyond_float32)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((rows, cols)) * 2).astype(np.float32)
    X[rows // 2] += np.float32(40)
    if cols > 1:
        c = cols // 3
        rest = np.delete(X[-1].astype(np.float64), c)
        X[-1, c] = np.float32(rest.max() + np.log(np.exp(rest - rest.max()).sum()) + lift)
    return X, rng.standard_normal((rows, cols)).astype(np.float32)


def masked_inputs(Tk, mode, Tq=MASKED_TQ, B=MASKED_B, H=MASKED_H, seed=0):
    """S, dY [B, H, Tq, Tk]; key_valid [B, Tk] with the LAST batch's last third padding; dense [B, Tq, Tk] with a tenth of its entries
    and the whole row (b, i) = (B - 1, Tq // 2) masked; scale 0.125."""
    rng = np.random.default_rng(seed + 7 * Tk + Tq)
    S = (rng.standard_normal((B, H, Tq, Tk)) * 3).astype(np.float32)
    dY = rng.standard_normal((B, H, Tq, Tk)).astype(np.float32)
    kv = dense = None
    if mode in ("key_valid", "all"):
        kv = np.ones((B, Tk), np.int32)
        kv[B - 1, Tk - max(Tk // 3, 1):] = 0
    if mode in ("dense", "all"):
        dense = (rng.uniform(size=(B, Tq, Tk)) >= 0.1).astype(np.int32)
        dense[B - 1, Tq // 2, :] = 0
    return dict(S=S, dY=dY, key_valid=kv, dense=dense, causal=mode in ("causal", "all"), scale=0.125, B=B, H=H, Tq=Tq, Tk=Tk)


def rms_inputs(rows, cols, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((rows, cols)) * 1.5 + 0.25).astype(np.float32)
    w = rng.uniform(0.5, 1.5, cols).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, cols).astype(np.float32)
    dY = rng.standard_normal((rows, cols)).astype(np.float32)
    addend = rng.standard_normal((rows, cols)).astype(np.float32)
    return X, w, b, dY, addend


CE_IGNORE = 0


def ce_inputs(rows, C, seed=0):
    """logits of spread 3; int64 labels in [1, C) with ignore_index 0 on every fifth row (4, 9, ...), one out-of-range label (== C,
    row 1, when there are three rows) and one negative label that is not ignore_index (-3, row 6, when there are eight): both inert.
    Class weights in [0.25, 2)."""
    rng = np.random.default_rng(seed + rows + 3 * C)
    logits = (rng.standard_normal((rows, C)) * 3).astype(np.float32)
    labels = rng.integers(1, C, rows).astype(np.int64)
    labels[4::5] = CE_IGNORE
    if rows >= 3:
        labels[1] = C
    if rows >= 8:
        labels[6] = -3
    labels[0] = C - 1                     # the last column: the last element of the last thread's tile
    weight = rng.uniform(0.25, 2.0, C).astype(np.float32)
    return logits, labels, weight


def embedding_ids(V, n, seed=0):
    """int32 ids [n].  n >= 9: nine special entries in this order among random ids of [0, V) -- k, k2 - V, -1, -V, V, -V - 1, k, k - V,
    k2: id k twice; then k - V, which aliases row k from a LATER position (it wins); k2 - V BEFORE k2 (k2 wins); -1 and -V, the ends
    of the negative range; V and -V - 1, just outside it.  Fewer ids: as many of V - 1, -1 (one row, the later wins), -V, V, -V - 1
    as fit, from the back (n == 1: the id -1)."""
    rng = np.random.default_rng(seed + V + n)
    if n < 9:
        return np.array([V - 1, -1, -V, V, -V - 1][:max(n, 2)][-n:] if n > 1 else [-1], np.int32)
    k, k2 = int(rng.integers(0, V)), int(rng.integers(0, V))
    ids = rng.integers(0, V, n).astype(np.int32)
    pos = np.sort(rng.choice(n, 9, replace=False))
    ids[pos] = [k, k2 - V, -1, -V, V, -V - 1, k, k - V, k2]
    return ids


def embedding_inputs(V, D, n, T, seed=0):
    rng = np.random.default_rng(seed + D)
    W = rng.standard_normal((V, D)).astype(np.float32)
    pe = rng.standard_normal((T, D)).astype(np.float32)
    g = rng.standard_normal((n, D)).astype(np.float32)
    return W, embedding_ids(V, n, seed), pe, g


def map_inputs(n, seed=0):
    """x of spread 3 (both signs, some exact zeros), an upstream gradient, and a second operand."""
    rng = np.random.default_rng(seed + n)
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    x[::7] = 0
    return x, rng.standard_normal(n).astype(np.float32), rng.uniform(-2, 2, n).astype(np.float32)


# ============================================================================================ fixtures of the reference
@pytest.mark.parametrize("name", ["softmax_last", "softmax_axis1_4d", "softmax_axis1_2d"])
def test_softmax_restatement_matches_reference_fixture(golden, name):
    g = golden(name)
    axis = int(g["axis"])
    np.testing.assert_allclose(softmax_forward(g["X"], axis), g["Y"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(softmax_backward(g["Y"], g["dY"], axis), g["dX"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["rmsnorm_2d", "rmsnorm_3d_bias"])
def test_rmsnorm_restatement_matches_reference_fixture(golden, name):
    g = golden(name)
    Y, _, _ = rmsnorm_forward(g["X"], g["w"], g.get("b"), float(g["eps"]))
    np.testing.assert_allclose(Y, g["Y"], rtol=1e-5, atol=1e-5)
    dX, dw, db = rmsnorm_backward(g["X"], g["w"], g["dY"], float(g["eps"]))
    np.testing.assert_allclose(dX, g["dX"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dw, g["dw"], rtol=1e-4, atol=1e-5)
    if "b" in g:
        np.testing.assert_allclose(db, g["db"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", ["ce_mean", "ce_sum", "ce_none", "ce_mean_ign", "ce_sum_ign", "ce_none_ign", "ce_mean_pad0", "ce_mean_small"])
def test_cross_entropy_restatement_matches_reference_fixture(golden, name):
    g = golden(name)
    _, _, loss, dlogits, _ = cross_entropy(g["logits"], g["labels"], None, int(g["ignore_index"]), str(g["reduction"]))
    np.testing.assert_allclose(np.reshape(loss, g["loss"].shape), g["loss"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dlogits, g["dlogits"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_weighted_cross_entropy_restatement_matches_reference_fixture(golden, reduction):
    g = golden("ce_weighted")
    assert np.any(g["labels"] == int(g["ignore_index"]))
    _, _, loss, dlogits, _ = cross_entropy(g["logits"], g["labels"], g["weight"], int(g["ignore_index"]), reduction)
    np.testing.assert_allclose(np.reshape(loss, -1), g[f"loss_{reduction}"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dlogits, g[f"dlogits_{reduction}"], rtol=1e-5, atol=1e-6)


def test_embedding_restatement_matches_reference_fixture(golden):
    g = golden("embedding")
    ids = g["ids"].reshape(-1)
    assert len(set(ids.tolist())) < ids.size, "the fixture must repeat an id"
    np.testing.assert_array_equal(embedding_forward(g["W"], ids, dtype=np.float32).reshape(g["out"].shape), g["out"])
    np.testing.assert_array_equal(embedding_backward(g["W"].shape, ids, g["grad"], dtype=np.float32), g["dW"])
    # held against first-write-wins: the fixture tells the two rules apart
    first = np.zeros_like(g["dW"])
    for p in reversed(range(ids.size)):
        first[ids[p]] = g["grad"].reshape(ids.size, -1)[p]
    assert not np.array_equal(first, g["dW"])


def test_activation_restatements_match_reference_fixtures(golden):
    g = golden("relu")
    np.testing.assert_array_equal(relu_forward(g["X"]), g["Y"])
    np.testing.assert_array_equal(relu_backward(g["dY"], g["Y"]), g["dX"])
    for name in ("swish_b1.0", "swish_b1.5"):
        g = golden(name)
        np.testing.assert_allclose(swish(g["X"], float(g["beta"])), g["Y"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(swish_backward(g["X"], g["dY"], float(g["beta"])), g["dX"], rtol=1e-5, atol=1e-5)
    for name in ("swiglu_2d", "swiglu_3d"):
        g = golden(name)
        np.testing.assert_allclose(swiglu(g["X"], float(g["beta"])), g["Y"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(swiglu_backward(g["X"], g["dY"], float(g["beta"])), g["dX"], rtol=1e-5, atol=1e-5)
    g = golden("gelu")
    np.testing.assert_allclose(gelu(g["X"]), g["Y"], rtol=1e-5, atol=1e-6)
    # (the reference's backward rounds its constants to six digits: the exact derivative differs by less than the GPU test's 1e-4)
    np.testing.assert_allclose(gelu_backward(g["X"], g["dY"]), g["dX"], rtol=1e-4, atol=1e-5)


# ============================================================================================ the oracle, on this file's makers
@pytest.mark.parametrize("cols", [6, 255, 1028, 4099])
def test_softmax_restatement_matches_oracle(cols):
    X, dY = softmax_inputs(SOFTMAX_ROWS, cols, cols)
    Y = softmax_forward(X)
    np.testing.assert_allclose(O.softmax_forward(X, -1), Y, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(O.softmax_backward(Y.astype(np.float32), dY, -1), softmax_backward(Y, dY), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(Y.sum(-1), 1.0, rtol=1e-12)
    # strided slices are the same rule along another axis
    Z = X.reshape(3, 3, cols)
    np.testing.assert_allclose(softmax_forward(Z, 1), O.softmax_forward(Z, 1), rtol=1e-5, atol=1e-6)


def test_saturated_softmax_row_is_beyond_float32():
    """Why softmax_inputs stops short of a one-hot row.  With the dominant score 12 above the balance point, y there is 1 - 6e-6 and
    dx = (dy - sum(dy y)) y is the difference of two numbers that agree to five digits: the oracle's own float32 evaluation of the
    reference's formula then misses the gradient bound (1e-4 of max(|ref|, rms)) at 20000 columns, where the tensor's rms is small.
    At the balance point (y = 1 / 2) the same evaluation sits below a twentieth of the bound."""
    for lift, over in ((12.0, True), (0.0, False)):
        X, dY = softmax_inputs(SOFTMAX_ROWS, 20000, 20000, lift)
        Y = softmax_forward(X)
        assert abs(Y[-1].max() - (1 - 6e-6 if over else 0.5)) < (1e-6 if over else 1e-3), Y[-1].max()
        ref = softmax_backward(Y, dY)
        err = np.abs(O.softmax_backward(Y.astype(np.float32), dY, -1) - ref) / (1e-4 * np.maximum(np.abs(ref), rms_of(ref)))
        assert (err.max() > 1.0) == over and (over or err.max() < 0.05), err.max()


@pytest.mark.parametrize("mode", MASK_MODES)
@pytest.mark.parametrize("Tq,Tk", [(MASKED_TQ, 7), (MASKED_TQ, 260), (9, 7), (3, 260)])
def test_masked_softmax_restatement_matches_oracle(Tq, Tk, mode):
    """The oracle's attention (MHA.forward / backward): scores = where(mask == 0, -1e9, scores * scale); softmax; and backward
    where(mask == 0, 0, softmax') * scale -- with the [B, 1, Tq, Tk] mask built here from the three sources."""
    c = masked_inputs(Tk, mode, Tq)
    m = masked_positions(c["B"], c["H"], Tq, Tk, c["key_valid"], c["dense"], c["causal"])
    assert m.any() == (mode != "none")
    scores = np.where(m, np.float32(-1e9), c["S"] * np.float32(c["scale"])).astype(np.float32)
    Yo = O.softmax_forward(scores, -1)
    Y = masked_softmax_forward(c["S"], c["key_valid"], c["dense"], c["scale"], c["causal"])
    np.testing.assert_allclose(Yo, Y, rtol=1e-5, atol=1e-6)
    dXo = np.where(m, np.float32(0), O.softmax_backward(Yo, c["dY"], -1)) * np.float32(c["scale"])
    dX = masked_softmax_backward(Y, c["dY"], c["key_valid"], c["dense"], c["scale"], c["causal"])
    np.testing.assert_allclose(dXo, dX, rtol=1e-4, atol=1e-6)
    assert np.all(dX[m] == 0)
    if mode in ("dense", "all"):
        np.testing.assert_allclose(Y[c["B"] - 1, :, Tq // 2], 1.0 / Tk, rtol=1e-12)          # the fully masked row is uniform
    if mode == "causal" and Tq == Tk:
        ids = np.ones((c["B"], Tk), np.int64)
        assert np.array_equal(O.attention_mask(ids, 0)[:, None] == 0, m[:, :1])               # the notebook's get_sub_mask


def test_minus_infinity_is_visibly_wrong_on_a_fully_masked_row():
    """Held against `-inf` for a masked score: a row with nothing visible then has max = -inf and exp(-inf + inf) = NaN, where the
    reference's -1e9 gives the uniform row."""
    c = masked_inputs(7, "dense")
    m = masked_positions(c["B"], c["H"], c["Tq"], 7, None, c["dense"], False)
    with np.errstate(invalid="ignore"):
        wrong = softmax_forward(np.where(m, -np.inf, c["S"] * 0.125), -1)
    right = masked_softmax_forward(c["S"], None, c["dense"], 0.125, False)
    row = (c["B"] - 1, 0, c["Tq"] // 2)
    assert np.all(np.isnan(wrong[row])) and np.all(right[row] == 1.0 / 7)
    assert MASKED == -1e9
    other = ~m.all(-1)
    np.testing.assert_allclose(wrong[other], right[other], rtol=1e-12)                         # elsewhere the two agree


@pytest.mark.parametrize("Tq,Tk", MASKED_TQ_NE_TK)
def test_causal_limit_without_the_shift_is_visibly_wrong(Tq, Tk):
    """Held against `j > i` (no Tk - Tq shift): with Tq != Tk it hides keys the last queries must see (Tq < Tk) or shows keys to
    queries that must see none (Tq > Tk)."""
    c = masked_inputs(Tk, "causal", Tq)
    right = masked_positions(c["B"], c["H"], Tq, Tk, None, None, True)
    i, j = np.arange(Tq)[:, None], np.arange(Tk)[None, :]
    wrong = np.broadcast_to(j > i, right.shape)
    assert not right[..., Tq - 1, :].any(), "the last query sees every key"
    assert (wrong != right).any()
    Y = masked_softmax_forward(c["S"], None, None, c["scale"], True)
    Yw = softmax_forward(np.where(wrong, MASKED, c["S"].astype(np.float64) * c["scale"]), -1)
    assert np.abs(Y - Yw).max() > 1e-2
    if Tq > Tk:
        assert right[..., 0, :].all() and np.allclose(Y[..., 0, :], 1.0 / Tk)                  # query 0 of 9 sees none of 7 keys


@pytest.mark.parametrize("cols", [510, 1001, 4099])
def test_rmsnorm_restatement_matches_oracle(cols):
    X, w, b, dY, addend = rms_inputs(RMS_ROWS, cols, cols)
    Y, xn, std = rmsnorm_forward(X, w, b, EPS)
    Yo, xno, stdo = O.rmsnorm_forward(X, w, b, EPS)
    np.testing.assert_allclose(Yo, Y, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(xno, xn, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(stdo.reshape(-1), std, rtol=1e-6)
    dX, dw, db = rmsnorm_backward(X, w, dY, EPS)
    dXo, dwo, dbo = O.rmsnorm_backward(X, w, True, dY, EPS)
    np.testing.assert_allclose(dXo, dX, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dwo, dw, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dbo, db, rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(rmsnorm_backward(X, w, dY, EPS, addend)[0], dX + addend.astype(np.float64))
    # held against the mean-centred (LayerNorm) statistic: X has mean 0.25, so the two differ visibly
    assert np.abs(std - X.astype(np.float64).std(-1)).max() > 1e-3


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("shape", [(33, 10), (68, 1001)])
def test_cross_entropy_restatement_matches_oracle(shape, reduction, weighted):
    """On the live rows alone the oracle (which has no notion of an out-of-range label) must give the restatement's numbers."""
    logits, labels, weight = ce_inputs(*shape)
    w = weight if weighted else None
    rows, C = shape
    loss_rows, lse, loss, dlogits, count = cross_entropy(logits, labels, w, CE_IGNORE, reduction)
    live = (labels != CE_IGNORE) & (labels >= 0) & (labels < C)
    assert 0 < count == live.sum() < (labels != CE_IGNORE).sum() < rows
    lo, dlo = O.cross_entropy_forward_backward(logits[live], labels[live], w, CE_IGNORE, reduction)
    np.testing.assert_allclose(lo, loss_rows[live] if reduction == "none" else loss, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dlo, dlogits[live], rtol=1e-4, atol=1e-7)
    assert np.all(dlogits[~live] == 0) and np.all(loss_rows[~live] == 0)
    np.testing.assert_allclose(lse, np.log(np.exp(logits.astype(np.float64)).sum(1)), rtol=1e-12)
    np.testing.assert_allclose(dlogits[live].sum(1), 0.0, atol=1e-12)                        # a softmax minus a one-hot, scaled


def test_mean_over_all_rows_is_visibly_wrong():
    """Held against 'mean' = sum / rows: a fifth of the rows is ignored and two more are inert, so the two denominators differ by a
    quarter -- far outside the 1e-5 the loss is held to."""
    logits, labels, weight = ce_inputs(33, 10)
    loss_rows, _, loss, dlogits, count = cross_entropy(logits, labels, None, CE_IGNORE, "mean")
    assert count == 33 - 6 - 2
    wrong = loss_rows.sum() / 33
    assert abs(wrong - loss) > 0.1 * abs(loss)
    np.testing.assert_allclose(loss, loss_rows.sum() / count, rtol=1e-15)
    _, _, loss_w, dl_w, _ = cross_entropy(logits, labels, weight, CE_IGNORE, "mean")
    live = (labels != CE_IGNORE) & (labels >= 0) & (labels < 10)
    np.testing.assert_allclose(loss_w, cross_entropy(logits, labels, weight, CE_IGNORE, "sum")[2] / weight[labels[live]].astype(np.float64).sum(), rtol=1e-12)
    # nothing live: 'mean' is 0 / 0 and the gradient is zero, not NaN
    none = cross_entropy(logits, np.zeros(33, np.int64), None, CE_IGNORE, "mean")
    assert np.isnan(none[2]) and np.all(none[3] == 0) and none[4] == 0


@pytest.mark.parametrize("case", EMBEDDING_CASES, ids=lambda c: "V%d-D%d-n%d-T%d" % c)
def test_embedding_restatement_matches_oracle_and_rejects_first_write_wins(case):
    V, D, n, T = case
    W, ids, pe, g = embedding_inputs(V, D, n, T)
    row, ok = embedding_rows(ids, V)
    if n >= 9:
        assert (~ok).sum() == 2 and -1 in ids and -V in ids and V in ids and -V - 1 in ids
        assert len(set(row[ok].tolist())) < ok.sum()
    # NumPy's own indexing is the oracle's rule; it refuses out-of-range ids, so they are compared on the valid positions
    out = embedding_forward(W, ids, dtype=np.float32)
    np.testing.assert_array_equal(out[ok], O.embedding_forward(W, ids[ok]))
    assert np.all(out[~ok] == 0)
    dW = embedding_backward((V, D), ids, g, dtype=np.float32)
    np.testing.assert_array_equal(dW, O.embedding_backward((V, D), ids[ok], g[ok]))
    s = float(np.sqrt(D))
    full = embedding_forward(W, ids, s, pe, T)
    np.testing.assert_allclose(full[ok], W[row[ok]].astype(np.float64) * np.float64(np.float32(s)) + pe[np.arange(n)[ok] % T], rtol=1e-15)
    np.testing.assert_array_equal(full[~ok], pe[np.arange(n)[~ok] % T].astype(np.float64))
    # held against first-write-wins
    if len(set(row[ok].tolist())) < ok.sum():
        first = np.zeros((V, D), np.float32)
        for p in reversed(range(n)):
            if ok[p]:
                first[row[p]] = g[p]
        assert not np.array_equal(first, dW)
    if n >= 9:
        k_pos = [p for p in range(n) if ok[p] and row[p] == row[np.flatnonzero(ids == -1)[0]]]
        np.testing.assert_array_equal(dW[V - 1], g[k_pos[-1]])                               # the later position, by whichever alias


def test_map_restatements_match_oracle():
    x, dy, u = map_inputs(4097)
    with np.errstate(invalid="ignore"):
        got = relu_forward(SPECIALS)
    np.testing.assert_array_equal(got, O.relu_forward(SPECIALS))                              # (values: NaN == NaN, -0 == +0 here)
    np.testing.assert_array_equal(relu_forward(x), O.relu_forward(x))
    np.testing.assert_array_equal(relu_backward(dy, relu_forward(x)), O.relu_backward(relu_forward(x), dy) + np.float32(0))
    for beta in (1.0, 1.5):
        np.testing.assert_allclose(O.swish_forward(x, np.float32(beta)), swish(x, beta), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(O.swish_backward(x, dy, np.float32(beta)), swish_backward(x, dy, beta), rtol=1e-5, atol=1e-5)
        X2 = np.stack([x[:4096].reshape(64, 64), u[:4096].reshape(64, 64)], 1).reshape(64, 128)[:, :]
        np.testing.assert_allclose(O.swiglu_forward(X2, np.float32(beta)), swiglu(X2, beta), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(O.swiglu_backward(X2, dy[:4096].reshape(64, 64), np.float32(beta)),
                                   swiglu_backward(X2, dy[:4096].reshape(64, 64), beta), rtol=1e-5, atol=1e-5)
    # GELU: the tanh form equals x sigmoid(2u), the identity the kernel evaluates
    from rowops_ref import GELU_C, GELU_K, sigmoid
    x64 = x.astype(np.float64)
    # (absolute: 1 + tanh u cancels on the far negative side, where the value is below 1e-10 and float64 leaves 1e-16 of it)
    np.testing.assert_allclose(gelu(x), x64 * sigmoid(2 * GELU_K * (x64 + GELU_C * x64 ** 3)), rtol=1e-12, atol=1e-15)
    h = 1e-6
    np.testing.assert_allclose(gelu_backward(x, 1.0), (gelu(x64 + h) - gelu(x64 - h)) / (2 * h), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(swish_backward(x, 1.0, 1.5), (swish(x64 + h, 1.5) - swish(x64 - h, 1.5)) / (2 * h), rtol=1e-6, atol=1e-8)


def test_dropout_hash_restatement():
    """The hash is the kernel's, so what can be checked without it: wrap-around arithmetic (no NumPy overflow escapes to a wider
    type), the special values of p, the seed + seed_dev rule, and the keep rate and scale."""
    n = 70001
    for p in DROPOUT_P:
        k = dropout_keep(1234, None, n, p)
        assert k.dtype == np.float32 and k.shape == (n,)
        if p == 0:
            assert np.all(k == 1)
        elif p == 1:
            assert np.all(k == 0)
        else:
            s = np.float32(1) / (np.float32(1) - np.float32(p))
            assert set(np.unique(k).tolist()) == {0.0, float(s)}
            assert abs((k != 0).mean() - (1 - p)) < 4 * np.sqrt(p * (1 - p) / n)              # four standard deviations
    a = dropout_keep(7, 5, n, 0.5)
    assert np.array_equal(a, dropout_keep(12, None, n, 0.5)) and not np.array_equal(a, dropout_keep(13, None, n, 0.5))
    assert np.array_equal(dropout_keep(0xFFFFFFFF, 3, n, 0.5), dropout_keep(2, None, n, 0.5))  # the seed sum wraps
    assert np.array_equal(dropout_keep(7, None, n, 0.5)[:4099], dropout_keep(7, None, 4099, 0.5))   # a function of the index alone


def test_dispatch_restatement():
    assert [row_tier(c) for c in (1, 256, 257, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385)] == \
        ["64x1", "64x1", "64x2", "64x2", "64x4", "64x4", "256x4", "256x4", "256x8", "256x8", "1024x4", "1024x4", "looped"]
    assert row_variant(256) == "64x1-vec" and row_variant(256, 1) == "64x1-scalar" and row_variant(255) == "64x1-scalar"
    assert row_variant(256, 0, 257) == "64x1-scalar" and row_variant(256, 0, 260) == "64x1-vec"
    # every tier is reached in both variants by each family's table, and the looped kernels too
    tiers = ["64x1", "64x2", "64x4", "256x4", "256x8", "1024x4"]
    for table in ([row_variant(c, o) for c, o in SOFTMAX_CASES], [row_variant(t) for t in MASKED_TK],
                  [ce_kernel(*s).replace("-2blocks", "") for s in CE_SHAPES]):
        assert {f"{t}-{v}" for t in tiers for v in ("vec", "scalar")} <= set(table), table
    assert {row_variant(c, o) for c, o in RMS_CASES} >= {f"{t}-scalar" for t in tiers[1:]} | {"looped"}
    assert all(ce_kernel(*s) != "small" for s in CE_SHAPES + CE_MULTI_ROUND)
    assert all(ce_kernel(r - 1, c) == "small" for r, c in CE_SHAPES[:8] if (r - 1) * c <= 65536)   # the smallest that leave it
    assert [ce_kernel(*s).endswith("-2blocks") for s in CE_SHAPES[8::2]] == [True, True, True]


# ============================================================================================ C ABI: refusals before any launch
@pytest.fixture(scope="module")
def lib():
    import neunet_hip
    from neunet_hip import _lib
    try:
        neunet_hip.load_library()
    except (OSError, _lib.NeunetHipError) as exc:
        pytest.skip(f"the library does not load here: {exc}")
    return _lib


def status(lib, name, *args):
    """The entry's status code itself (call_hip_function turns it into an exception)."""
    return lib.load_hip_function(name)(*args)


def test_elementwise_argument_errors(lib):
    s = lambda name, *a: status(lib, name, *a)  # noqa: E731
    maps = {"nnhipReLUForward": lambda n, *p: s("nnhipReLUForward", *p, n, None), "nnhipReLUBackward": lambda n, *p: s("nnhipReLUBackward", *p, n, None),
            "nnhipSwishForward": lambda n, *p: s("nnhipSwishForward", *p, 1.0, n, None),
            "nnhipSwishBackward": lambda n, *p: s("nnhipSwishBackward", *p, 1.0, n, None),
            "nnhipGELUForward": lambda n, *p: s("nnhipGELUForward", *p, n, None), "nnhipGELUBackward": lambda n, *p: s("nnhipGELUBackward", *p, n, None),
            "nnhipAdd": lambda n, *p: s("nnhipAdd", *p, n, None), "nnhipMul": lambda n, *p: s("nnhipMul", *p, n, None),
            "nnhipScale": lambda n, *p: s("nnhipScale", *p, 2.0, n, None),
            "nnhipDropout": lambda n, *p: s("nnhipDropout", *p, n, 0.5, 1, None, None),
            "nnhipFusedSwishAndMul": lambda n, *p: s("nnhipFusedSwishAndMul", *p, 1.0, 4, n, None),
            "nnhipFusedSwishAndMulBackward": lambda n, *p: s("nnhipFusedSwishAndMulBackward", *p, 1.0, 4, n, None),
            "nnhipScaleRows": lambda n, *p: s("nnhipScaleRows", *p, n, 1, 1, None)}
    operands = {"nnhipReLUForward": 2, "nnhipReLUBackward": 3, "nnhipSwishForward": 2, "nnhipSwishBackward": 3, "nnhipGELUForward": 2,
                "nnhipGELUBackward": 3, "nnhipAdd": 3, "nnhipMul": 3, "nnhipScale": 1, "nnhipDropout": 2, "nnhipFusedSwishAndMul": 2,
                "nnhipFusedSwishAndMulBackward": 3, "nnhipScaleRows": 3}
    for name, f in maps.items():
        k = operands[name]
        assert f(-4, *[16] * k) == EINVAL, name                                              # a negative size
        assert f(0, *[None] * k) == 0, name                                                  # nothing to do: no pointer is looked at
        for i in range(k):
            for bad, want, word in ((None, EINVAL, "null"), (18, EALIGN, "misaligned"), (17, EALIGN, "misaligned")):
                p = [16] * k
                p[i] = bad
                assert f(8, *p) == want and word in lib.last_error() and name in lib.last_error(), (name, i, bad)
    for p in (-0.1, 1.5):
        assert s("nnhipDropout", 16, 16, 8, p, 1, None, None) == EINVAL
    for stride in (2, -1):
        assert s("nnhipScaleRows", 16, 16, 16, 2, 3, stride, None) == EINVAL
    for name, args in (("nnhipFusedSwishAndMul", (16, 16)), ("nnhipFusedSwishAndMulBackward", (16, 16, 16))):
        assert s(name, *args, 1.0, 4, 10, None) == EINVAL and "multiple of hidden" in lib.last_error()     # size % hidden != 0
        assert s(name, *args, 1.0, 0, 8, None) == EINVAL
    assert s("nnhipIncrementU32", None, 1, None) == EINVAL


def test_rowop_argument_errors(lib):
    s = lambda name, *a: status(lib, name, *a)  # noqa: E731
    for name, k in (("nnhipSoftmaxForward", 2), ("nnhipSoftmaxBackward", 3)):
        assert s(name, *[16] * k, -1, 4, 1, None) == EINVAL and s(name, *[16] * k, 4, -1, 1, None) == EINVAL
        assert s(name, *[16] * k, 4, 4, 0, None) == EINVAL and "stride" in lib.last_error()
        assert s(name, *[None] * k, 0, 4, 1, None) == 0
        for i in range(k):
            p = [16] * k
            p[i] = None
            assert s(name, *p, 4, 4, 1, None) == EINVAL and "null" in lib.last_error()
    #                                X   w   b     Y   std Xnorm rows cols eps
    assert s("nnhipRMSNormForward", 16, 16, None, 16, 16, None, -1, 4, EPS, None) == EINVAL
    assert s("nnhipRMSNormForward", 16, 16, None, 16, 16, None, 4, -1, EPS, None) == EINVAL
    assert s("nnhipRMSNormForward", None, None, None, None, None, None, 0, 4, EPS, None) == 0
    for i in (0, 1, 3, 4):
        p = [16, 16, None, 16, 16, None]
        p[i] = None
        assert s("nnhipRMSNormForward", *p, 4, 4, EPS, None) == EINVAL and "null" in lib.last_error()
    #                                   dY  X   w   std Xn    add   dX  dW  db
    assert s("nnhipRMSNormBackwardEx", 16, 16, 16, 16, None, None, 16, 16, None, -1, 4, None) == EINVAL
    for i in (0, 1, 2, 3, 6, 7):
        p = [16, 16, 16, 16, None, None, 16, 16, None]
        p[i] = None
        assert s("nnhipRMSNormBackwardEx", *p, 4, 4, None) == EINVAL and "null" in lib.last_error()
    for name, k in (("nnhipMaskedSoftmaxForwardEx", 2), ("nnhipMaskedSoftmaxBackwardEx", 3)):
        assert s(name, *[16] * k, None, None, -1, 2, 3, 4, 1.0, 0, None) == EINVAL

    def ce(logits=16, dlogits=16, loss_rows=16, lse=16, labels=16, lbytes=4, ld=8, rows=4, cols=8, red=b"m", loss_out=16):
        return s("nnhipCrossEntropyLossEx", logits, dlogits, loss_rows, lse, labels, lbytes, None, ld, -100, rows, cols, red, loss_out, None, None)
    assert ce(ld=7) == EINVAL and "bad sizes" in lib.last_error()                              # logits_stride < n_cols
    assert ce(rows=-1) == EINVAL and ce(cols=-1, ld=0) == EINVAL
    for lbytes in (3, 1, 0, 16):
        assert ce(lbytes=lbytes) == EINVAL and "int16, int32 or int64" in lib.last_error()
    assert ce(red=b"x") == EINVAL and "reduction" in lib.last_error()
    for red in (b"m", b"s"):
        assert ce(red=red, loss_out=None) == EINVAL and "need loss_out" in lib.last_error()
    for missing in ("logits", "loss_rows", "lse", "labels"):
        assert ce(**{missing: None}) == EINVAL and "null" in lib.last_error()
    assert ce(rows=0, red=b"n", loss_out=None, logits=None, labels=None) == 0


def test_embedding_argument_errors(lib):
    s = lambda name, *a: status(lib, name, *a)  # noqa: E731
    #                                 out W   ids pe    n  dim T  vocab scale
    fwd = lambda **k: s("nnhipEmbeddingForward", k.get("out", 16), k.get("W", 16), k.get("ids", 16), None, k.get("n", 4), k.get("dim", 8),  # noqa: E731
                        k.get("T", 4), k.get("vocab", 10), 1.0, None)
    bwd = lambda **k: s("nnhipEmbeddingBackward", k.get("dW", 16), k.get("g", 16), k.get("ids", 16), k.get("n", 4), k.get("dim", 8),  # noqa: E731
                        k.get("vocab", 10), 1.0, None)
    for f in (fwd, bwd):
        for bad in (dict(vocab=0), dict(vocab=-1), dict(n=-1), dict(dim=-1)):
            assert f(**bad) == EINVAL and "bad sizes" in lib.last_error(), bad
        assert f(dim=0, out=None, W=None, ids=None, dW=None, g=None) == 0
    assert fwd(T=0) == EINVAL
    assert fwd(n=0, out=None, W=None, ids=None) == 0
    for missing in ("out", "W", "ids"):
        assert fwd(**{missing: None}) == EINVAL and "null" in lib.last_error()
    for missing in ("dW", "g", "ids"):
        assert bwd(**{missing: None}) == EINVAL and "null" in lib.last_error()
    assert bwd(n=1 << 31) == EINVAL and "too many ids" in lib.last_error()
    assert s("nnhipNotEqualInt32", 16, 16, -1, 0, None) == EINVAL and s("nnhipNotEqualInt32", None, None, 0, 0, None) == 0
    assert s("nnhipNotEqualInt32", None, 16, 4, 0, None) == EINVAL and s("nnhipNotEqualInt32", 16, None, 4, 0, None) == EINVAL

