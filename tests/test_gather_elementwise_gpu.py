"""GPU: csrc/embedding.hip (the gather with its fused scale and positional term, the last-write-wins gradient, the pad mask) and
csrc/elementwise.hip (the float4 maps, SwiGLU, the counter-hash dropout) through the C ABI (include/neunet_hip.h), against
tests/rowops_ref.py.  tests/test_hip_parity.py keeps the reference's fixtures and the module-level cases.

Which call reaches which variant:

    embedding_fwd_kernel / embedding_bwd_kernel   a wave per row, four rows per block.  float4 lanes (a trip of the lane loop covers 256
                                                  columns) when D % 4 == 0 and W, out, pe (dW, grad) are 16-byte aligned; else one float
                                                  per lane (a trip covers 64 columns)
    embedding_last_kernel                         a thread per id, 256 per block: atomicMax of the position into last[row]
    map1_kernel / map2_kernel                     float4 body + scalar tail when every operand is 16-byte aligned (a block's span is
                                                  256 threads x 4 float4 = 4096 floats), else all scalar; ReLU, Swish, GELU, Scale and
                                                  Add, Mul and the three backwards are instances of the two
    swiglu_fwd_kernel / swiglu_bwd_kernel         float4 when h % 4 == 0 and every operand is aligned, else scalar
    dropout_hash_kernel                           float4 body + tail, or scalar: both hash the ELEMENT index, so both give one mask

`off1` starts every float operand four bytes into its allocation.  Every output lives between NaN fences, checked after each call.

Bounds.  Copies and single float32 operations (the gather with scale 1 and no pe, its gradient, ReLU, Add, Mul, Scale, ScaleRows,
dropout) are exact: bits are compared.  The gather with a scale or a positional term: each element within one float32 rounding per
operation of the float64 value, 2^-24 (|w s| + |w s + pe|) (the compiler may or may not contract the multiply-add).  Swish: the bounds
of test_swish_fast_sigmoid_accuracy_sweep (1e-6 + 2 ulp of the result; backward 1e-6 + 2 ulp of 1 + |beta f|).  SwiGLU: rtol = atol =
1e-5 (test_swiglu_vs_oracle).  GELU: rtol = atol = 1e-4 (test_gelu_gpt2_size_vs_float64).  One run's error / bound figures are in
EXPERIMENTS.md 5.21."""
import numpy as np
import pytest

from rowops_ref import (U24, dropout_keep, embedding_backward, embedding_forward, gelu, gelu_backward, relu_backward, relu_forward, swiglu,
                        swiglu_backward, swish, swish_backward)
from test_rowops_ref import DROPOUT_P, DROPOUT_SIZES, EMBEDDING_CASES, MAP_SIZES, SPECIALS, SWIGLU_CASES, embedding_inputs, map_inputs
from test_rowops_tiers_gpu import Buf, call, close_bound, dev, host, ratio

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, ref):
    """Bit-identical, a NaN of any payload counting as a NaN."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    nan = np.isnan(ref)
    return got.shape == ref.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(ref)[~nan])


OFFS = pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])


# ===================================================================================================== Embedding
def embedding_variant(D, off):
    return "vec" if D % 4 == 0 and off == 0 else "scalar"


@OFFS
@pytest.mark.parametrize("case", EMBEDDING_CASES, ids=lambda c: "V%d-D%d-n%d-T%d" % c)
def test_embedding_cases(hip, case, off):
    """Forward and backward with scale 1 and sqrt(D), with and without the positional table.  The ids repeat, run through both ends of
    the negative range, alias one row as k and k - V, and step outside the range on both sides (test_rowops_ref.embedding_ids)."""
    V, D, n, T = case
    W, ids, pe, g = embedding_inputs(V, D, n, T)
    w_d, pe_d, g_d, ids_d = Buf(W, off), Buf(pe, off), Buf(g, off), dev(ids, np.int32)
    tag = f"embedding V {V} D {D} n {n} T {T} {embedding_variant(D, off)}"
    for scale in (1.0, float(np.sqrt(D))):
        for with_pe in (False, True):
            out = Buf((n, D), off)
            call("nnhipEmbeddingForward", out.t, w_d.t, ids_d, pe_d.t if with_pe else None, n, D, T, V, scale)
            assert out.intact(), tag
            if scale == 1.0 and not with_pe:
                assert same(out.host(), embedding_forward(W, ids, dtype=np.float32)), tag + ": the gather is a row copy"
            else:
                ref = embedding_forward(W, ids, scale, pe if with_pe else None, T)
                ws = embedding_forward(W, ids, scale, None, T)
                bound = U24 * (np.abs(ws) + np.abs(ref))
                r = ratio(out.host(), ref, bound)
                print(f"\n[{tag} scale {scale:.3f} pe {with_pe}] error / bound: {r:.3f}")
                assert np.all(np.abs(out.host().astype(np.float64) - ref) <= bound), (tag, scale, with_pe, r)
        dW = Buf((V, D), off)                                            # NaN everywhere: untouched rows must come back 0
        call("nnhipEmbeddingBackward", dW.t, g_d.t, ids_d, n, D, V, scale)
        assert dW.intact(), tag
        if scale == 1.0:
            assert same(dW.host(), embedding_backward((V, D), ids, g, dtype=np.float32)), tag + ": the gradient is a row copy"
        else:
            ref = embedding_backward((V, D), ids, g, scale)
            assert np.all(np.abs(dW.host().astype(np.float64) - ref) <= U24 * np.abs(ref)), tag + ": one multiply"
            assert np.array_equal(dW.host() == 0, ref == 0)
    # no ids at all: the gradient is zero-filled, nothing else is read
    dW = Buf((V, D), off)
    call("nnhipEmbeddingBackward", dW.t, None, None, 0, D, V, 1.0)
    assert dW.intact() and np.all(dW.host() == 0)
    assert np.array_equal(host(ids_d), ids) and np.array_equal(w_d.host(), W) and np.array_equal(g_d.host(), g)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_not_equal_int32(hip, n):
    rng = np.random.default_rng(n)
    ids = rng.integers(-2, 3, n).astype(np.int32)
    out = torch.full((n + 2,), -7, device="cuda", dtype=torch.int32)
    call("nnhipNotEqualInt32", out[1:n + 1], dev(ids, np.int32), n, 0)
    got = host(out)
    assert got[0] == -7 and got[-1] == -7 and np.array_equal(got[1:-1], (ids != 0).astype(np.int32))


# ===================================================================================================== maps
def swish_bounds(x, beta):
    f = swish(x, beta)
    return (1e-6 + 2 * np.spacing(np.abs(f).astype(np.float32)).astype(np.float64),
            1e-6 + 2 * np.spacing((1.0 + np.abs(np.float64(np.float32(beta)) * f)).astype(np.float32)).astype(np.float64))


@OFFS
@pytest.mark.parametrize("n", MAP_SIZES)
def test_map_sizes(hip, n, off):
    """Every instance of map1_kernel / map2_kernel at sizes around the float4 body / scalar tail and the one-block span, aligned
    (float4 body) and four bytes off (all scalar)."""
    X, dY, U = map_inputs(n)
    x, dy, u = Buf(X, off), Buf(dY, off), Buf(U, off)
    new = lambda: Buf((n,), off)  # noqa: E731
    tag = f"maps n {n} {'off1' if off else 'aligned'}"

    # ---- exact ones
    y = new()
    call("nnhipReLUForward", y.t, x.t, n)
    assert y.intact() and same(y.host(), relu_forward(X)), tag + " ReLU forward"
    dx = new()
    call("nnhipReLUBackward", dx.t, dy.t, y.t, n)
    assert dx.intact() and same(dx.host(), relu_backward(dY, relu_forward(X))), tag + " ReLU backward"
    s, p = new(), new()
    call("nnhipAdd", s.t, x.t, u.t, n)
    call("nnhipMul", p.t, x.t, u.t, n)
    assert s.intact() and p.intact() and same(s.host(), X + U) and same(p.host(), X * U), tag + " Add / Mul"
    sc = Buf(X, off)
    call("nnhipScale", sc.t, 0.3, n)
    assert sc.intact() and same(sc.host(), np.float32(0.3) * X), tag + " Scale"
    for cols in (1, 7):
        rows = n
        M = np.random.default_rng(n + cols).standard_normal((rows, cols)).astype(np.float32)
        m = Buf(M, off)
        for stride, factors in ((0, U[:1]), (1, U)):
            f, o = Buf(factors, off), Buf((rows, cols), off)
            call("nnhipScaleRows", o.t, m.t, f.t, rows, cols, stride)
            assert o.intact() and same(o.host(), M * (factors[:, None] if stride else factors[0])), tag + f" ScaleRows cols {cols} stride {stride}"

    # ---- in place, as the package calls them: bit-identical to out of place
    a = Buf(X, off)
    call("nnhipAdd", a.t, a.t, u.t, n)                                   # tok = tok + pos
    assert a.intact() and torch.equal(a.t, s.t), tag + " Add(a, a, b)"
    a = Buf(U, off)
    call("nnhipAdd", a.t, x.t, a.t, n)
    assert a.intact() and torch.equal(a.t, s.t), tag + " Add(a, b, a)"
    a = Buf(X, off)
    call("nnhipMul", a.t, a.t, u.t, n)                                   # dattn = dattn * mask
    assert a.intact() and torch.equal(a.t, p.t), tag + " Mul(a, a, m)"

    # ---- Swish and GELU
    shares = {}
    for beta in (1.0, 1.5):
        f, dxs = new(), new()
        call("nnhipSwishForward", f.t, x.t, beta, n)
        call("nnhipSwishBackward", dxs.t, dy.t, x.t, beta, n)
        a = Buf(X, off)
        call("nnhipSwishBackward", a.t, dy.t, a.t, beta, n)              # dZ over Z
        assert f.intact() and dxs.intact() and a.intact() and torch.equal(a.t, dxs.t), tag + " Swish"
        bf, bb = swish_bounds(X, beta)
        fr, dr = swish(X, beta), swish_backward(X, dY, beta)
        # the sweep's backward bound is for dY = 1, where the final product is exact: with a dY it scales by |dY| and the product adds
        # its own rounding, 2^-24 |dx|
        bd = np.abs(dY) * bb + U24 * np.abs(dr)
        shares[f"swish({beta})"], shares[f"swish'({beta})"] = ratio(f.host(), fr, bf), ratio(dxs.host(), dr, bd)
        ones = Buf(np.ones(n, np.float32), off)
        d1 = new()
        call("nnhipSwishBackward", d1.t, ones.t, x.t, beta, n)
        shares[f"swish'({beta}) at dY = 1"] = ratio(d1.host(), swish_backward(X, 1.0, beta), bb)
        assert np.all(np.abs(f.host() - fr) <= bf), tag + f" Swish forward beta {beta}"
        assert np.all(np.abs(dxs.host() - dr) <= bd), tag + f" Swish backward beta {beta}"
        assert d1.intact() and np.all(np.abs(d1.host() - swish_backward(X, 1.0, beta)) <= bb), tag + f" Swish backward beta {beta}, dY = 1"
    ge, dge = new(), new()
    call("nnhipGELUForward", ge.t, x.t, n)
    call("nnhipGELUBackward", dge.t, dy.t, x.t, n)
    assert ge.intact() and dge.intact()
    shares["gelu"] = ratio(ge.host(), gelu(X), close_bound(gelu(X), 1e-4, 1e-4))
    shares["gelu'"] = ratio(dge.host(), gelu_backward(X, dY), close_bound(gelu_backward(X, dY), 1e-4, 1e-4))
    print(f"\n[{tag}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    np.testing.assert_allclose(ge.host(), gelu(X), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dge.host(), gelu_backward(X, dY), rtol=1e-4, atol=1e-4)
    assert np.array_equal(x.host(), X) and np.array_equal(dy.host(), dY) and np.array_equal(u.host(), U)


@OFFS
def test_map_special_values(hip, off):
    """+-0, +-inf, NaN, denormals and the largest magnitudes through ReLU, Add and Mul: 13 values are three float4 and a tail of one,
    or all scalar.  ReLU keeps a NaN (max(0, NaN) is NaN in NumPy and in the reference: a diverged activation must stay visible); the
    sign of a zero RESULT is not part of ReLU's definition (rowops_ref.relu_forward), so values are compared there, not sign bits."""
    X = SPECIALS
    n = X.size
    x, y = Buf(X, off), Buf((n,), off)
    call("nnhipReLUForward", y.t, x.t, n)
    got, ref = y.host(), relu_forward(X)
    assert y.intact()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"ReLU forward: NaN at {np.flatnonzero(np.isnan(got))}, expected at {np.flatnonzero(np.isnan(ref))}"
    assert np.array_equal(got, ref, equal_nan=True)
    # backward: `out` runs through the specials (a NaN or zero output is a dead unit), then dY does at live and dead units
    dY = np.arange(1, n + 1, dtype=np.float32)
    dx = Buf((n,), off)
    call("nnhipReLUBackward", dx.t, Buf(dY, off).t, x.t, n)
    assert dx.intact() and same(dx.host(), relu_backward(dY, X))
    live = np.where(np.arange(n) % 2 == 0, np.float32(1), np.float32(-1))
    call("nnhipReLUBackward", dx.t, x.t, Buf(live, off).t, n)
    assert dx.intact() and same(dx.host(), relu_backward(X, live))
    # Add and Mul against every rotation of the specials: inf - inf, 0 * inf, denormal sums and products, overflow
    for k in range(n):
        R = np.roll(X, k)
        r, s, p = Buf(R, off), Buf((n,), off), Buf((n,), off)
        call("nnhipAdd", s.t, x.t, r.t, n)
        call("nnhipMul", p.t, x.t, r.t, n)
        with np.errstate(all="ignore"):
            assert s.intact() and same(s.host(), X + R), f"Add, rotation {k}"
            assert p.intact() and same(p.host(), X * R), f"Mul, rotation {k}"


@pytest.mark.parametrize("h,rows,off", SWIGLU_CASES, ids=[f"h{h}-rows{r}-{'vec' if h % 4 == 0 and not o else 'scalar'}{'-off1' if o else ''}"
                                                          for h, r, o in SWIGLU_CASES])
def test_swiglu_cases(hip, h, rows, off):
    """in rows are [gate (h) | up (h)]; size counts OUTPUT elements.  Both halves of dIn are checked on their own."""
    rng = np.random.default_rng(h + rows)
    X = (rng.standard_normal((rows, 2 * h)) * 2).astype(np.float32)
    dY = rng.standard_normal((rows, h)).astype(np.float32)
    x, dy = Buf(X, off), Buf(dY, off)
    for beta in (1.0, 1.5):
        y, dx = Buf((rows, h), off), Buf((rows, 2 * h), off)
        call("nnhipFusedSwishAndMul", y.t, x.t, beta, h, rows * h)
        call("nnhipFusedSwishAndMulBackward", dx.t, dy.t, x.t, beta, h, rows * h)
        assert y.intact() and dx.intact()
        Yr, dXr = swiglu(X, beta), swiglu_backward(X, dY, beta)
        shares = [ratio(y.host(), Yr, close_bound(Yr, 1e-5, 1e-5)), ratio(dx.host()[:, :h], dXr[:, :h], close_bound(dXr[:, :h], 1e-5, 1e-5)),
                  ratio(dx.host()[:, h:], dXr[:, h:], close_bound(dXr[:, h:], 1e-5, 1e-5))]
        print(f"\n[swiglu h {h} rows {rows} off {off} beta {beta}] error / bound: Y {shares[0]:.3f}, d gate {shares[1]:.3f}, d up {shares[2]:.3f}")
        np.testing.assert_allclose(y.host(), Yr, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(dx.host()[:, :h], dXr[:, :h], rtol=1e-5, atol=1e-5, err_msg="d gate")
        np.testing.assert_allclose(dx.host()[:, h:], dXr[:, h:], rtol=1e-5, atol=1e-5, err_msg="d up")
    assert np.array_equal(x.host(), X)


# ===================================================================================================== dropout
def run_dropout(X, off, p, seed, seed_dev=None):
    x, y = Buf(X, off), Buf(X.shape, off)
    call("nnhipDropout", y.t, x.t, X.size, p, seed, seed_dev)
    assert y.intact()
    return y.host()


@pytest.mark.parametrize("p", DROPOUT_P)
@pytest.mark.parametrize("n", DROPOUT_SIZES)
def test_dropout_mask_is_the_restated_hash(hip, n, p):
    """The aligned call (float4 body, elements 4 i .. 4 i + 3 hashed by one thread) and the call four bytes off (all scalar) give the
    same bits, and both are in * dropout_keep(...): the mask element by element, not its statistics.  seed_dev = k with seed s is
    seed s + k."""
    X = np.random.default_rng(n).uniform(0.5, 2.0, n).astype(np.float32)
    word = dev(np.array([234], np.int32), np.int32)
    for seed, seed_dev, total in ((1234, None, 1234), (1000, word, 1234), (0xFFFFFFF0, word, 0xFFFFFFF0 + 234)):
        a, b = run_dropout(X, 0, p, seed, seed_dev), run_dropout(X, 1, p, seed, seed_dev)
        assert np.array_equal(bits(a), bits(b)), "the float4 and the scalar variant draw different masks"
        ref = X * dropout_keep(total, None, n, p)
        assert np.array_equal(bits(a), bits(ref)), f"{int((a != ref).sum())} of {n} elements differ from the restated hash"
        assert np.array_equal(ref, X * dropout_keep(seed, None if seed_dev is None else 234, n, p))
    if p == 0:
        assert np.array_equal(a, X)
    if p == 1:
        assert np.all(a == 0)


def test_dropout_seed_word_increment(hip):
    n, s, k = 4099, 77, 5
    X = np.random.default_rng(0).uniform(0.5, 2.0, n).astype(np.float32)
    word = dev(np.array([k], np.int32), np.int32)
    before = run_dropout(X, 0, 0.5, s, word)
    call("nnhipIncrementU32", word, 1)
    after = run_dropout(X, 0, 0.5, s, word)
    assert int(host(word)[0]) == k + 1
    assert np.array_equal(before, X * dropout_keep(s + k, None, n, 0.5)) and np.array_equal(after, X * dropout_keep(s + k + 1, None, n, 0.5))
    assert not np.array_equal(before, after)
