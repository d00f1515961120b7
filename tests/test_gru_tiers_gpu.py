"""GPU: the GRU / RNN recurrences (csrc/recurrent_gru.hip) at every kernel instance and tile pattern, for one and two directions, at long
T, over the activation grid and at the edges of the C ABI contract (include/neunet_hip.h, "nn.GRU, nn.RNN, nn.Bidirectional"), against
the float64 restatement (tests/gru_ref.py), plus properties that need no reference.  tests/test_gru_gpu.py keeps the fixtures.

Which hidden size reaches which kernel (host dispatch rec_run_fwd / rec_run_bwd; Hp = H rounded up to 16, a tile = 16 columns of every
gate, wave w of 8 owns tiles w, w + 8, w + 16, w + 24; NG = 3 for the GRU, 1 for the RNN):

    H      Hp    instance <NG, MAXT>   tiles   pattern
    1      16    <NG, 1>               1       one tile, 15 padded columns, 7 idle waves; k-loops of one chunk
    16     16    <NG, 1>               1       exact
    17     32    <NG, 1>               2       15 padded columns in the second tile
    50     64    <NG, 1>               4       the notebook's size; 14 padded columns; the backward's 16-wide weight chunks start here
    112    112   <NG, 1>               7       exact, 1 idle wave; backward k-loops with a 16-wide chunk and a tail of 4s
    128    128   <NG, 1>               8       exact, every wave one tile
    129    144   <NG, 2>               9       wave 0 owns two tiles, the others one; 15 padded columns
    144    144   <NG, 2>               9       exact (the activation grid's size)
    200    208   <NG, 2>               13      waves 0-4 two tiles; 8 padded columns
    256    256   <NG, 2>               16      exact, every wave two tiles
    257    272   <NG, 4>               17      wave 0 three tiles, the others two; 15 padded columns
    400    400   <NG, 4>               25      wave 0 four tiles
    512    512   <NG, 4>               32      exact, every wave four tiles; 99 KB of LDS

Inputs (gru_abi.make_inputs): per direction weights U(-w / sqrt(H), w / sqrt(H)), biases U(-0.3, 0.3); data and upstream gradients
U(-1, 1), seeded.  w = 3 (three times the layer's own initial range: the recurrent term is of order 1) wherever T <= 9.  The
activation grid (T = 12) and T = 256 use w = 1: unlike the LSTM's, these recurrences are not contracting at w = 3 -- a tanh RNN with
a recurrent gain of 3 / sqrt(3) is chaotic and a relu one grows without bound, so the float32 REFERENCE itself leaves float64 by many
times the bound (measured on the CPU: up to 2e4 x at T = 12 with a relu, 1e6 x at T = 256); at w = 1 it stays within 4 %.
Bound: every tensor, forward and backward, within assert_close_scaled(tol = 1e-4) of float64 -- bound_for() of
tests/test_lstm_tiers_gpu.py, unchanged: a tensor whose float32 REFERENCE alone uses more than a quarter of the bound gets max(bound,
4 x |ref32 - ref64|), provided that stays below 1 % of its rms; computed from the two restatements, never from the kernel.

How much of the bound rounding uses.  "ref32": gru_ref in float32 (the reference's own arithmetic) against float64, on the CPU: the
worst element's share of the bound over the forward tensors / dX / the parameter gradients.  "kernel": the same figure for the HIP
kernels, from a run of this module on an MI355X (every case prints its own shares before it asserts: run with -s).  Worst case of each
group, GRU and RNN, one and two directions together:

    case                                          rms(Y)      ref32: forward / dX / gradients    kernel: forward / dX / gradients
    tier matrix, B 33, T 9, in 24, H >= 16        0.23-0.79   9.1 % / 13.0 % / 8.8 % (RNN H 400)  9.3 % / 13.6 % / 9.9 % (RNN H 512)
    tier matrix, H = 1                            0.74-0.93   1.1 % / 6.3 % / 6.7 %               0.9 % / 4.6 % / 7.2 %
    batch edges B 1 / 15 / 16 / 17, H 50 / 144    0.28-0.70   5.2 % / 5.4 % / 5.0 %               4.2 % / 6.2 % / 6.4 %
    in_features 1 / 3, H 50 / 144                 0.20-0.61   5.0 % / 4.9 % / 5.2 %               5.2 % / 5.1 % / 4.8 %
    nine activation pairs (GRU), w = 1            0.14-0.51   1.1 % / 0.8 % / 2.7 %               1.1 % / 0.8 % / 3.0 %
    three activations (RNN), w = 1                0.16-0.50   1.0 % / 0.6 % / 1.3 %               1.1 % / 0.6 % / 1.2 %
    T 256, B 20, in 16, H 128 / 200, w = 1        0.19-0.23   1.9 % / 0.8 % / 3.2 %               1.8 % / 1.7 % / 3.1 %
    ABI cases, B 17, T 5 / 9, in 6, H 50          0.19-0.66   1.9 % / 2.9 % / 2.2 %               1.9 % / 4.0 % / 2.6 %

At these inputs no tensor needs bound_for()'s widening (every ref32 share is below 25 %), the single-element bias gradients at H = 1
included.  The kernels sit where the float32 reference sits; a structurally wrong element (wrong row, stale h, dropped tile, padding
leaking in, a direction read the wrong way round) is of the order of the rms, four orders above the bound.

That the tests bite was checked with two one-line mutants of recurrent_gru.hip (never committed), each run once against this module
and tests/test_gru_gpu.py:
    forward `hnext = hbuf[s < 40 ? (s & 1) ^ 1 : 0]` (stale h late in a sequence): the four test_long_sequence cases and nothing else
        (every other case has T <= 12);
    `jt < ntile` -> `jt < (ntile & ~1)` in the backward's carry product (the GRU's [dz | dr] W^T, the RNN's ds W_h^T: last tile dropped
        when the tile count is odd): 62 cases -- test_tier_matrix at the odd tile counts, every case at H = 144 / 200, and the fixtures
        with H = 16.

The whole module (109 cases) takes about 8 s on an MI355X."""
import numpy as np
import pytest

from gru_abi import FORWARD_OUT, NW, grad_names, make_inputs, reference, run_abi
from lstm_abi import padded
from test_hip_parity import assert_close_scaled, assert_within, rms_of
from test_lstm_tiers_gpu import bound_for, share

pytestmark = pytest.mark.gpu

KINDS = ["gru", "rnn"]


@pytest.fixture(scope="module", autouse=True)
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def pairs_of(kind, out, ref, tag, forward=None, dX=True, grads="all"):
    """(name, got, float64, float32) of every requested output; what was not requested must not have been written."""
    ndir, B, T, H = ref["Y"].shape
    names = grad_names(kind, ndir)
    r32 = ref["f32"]
    pairs = []
    for k in (FORWARD_OUT[kind] if forward is None else forward):
        if k == "gates":
            g = out["gates"].reshape(ndir, B, T, 3, padded(H))
            assert np.all(np.isfinite(g)), f"{tag}: non-finite value in the saved gates (padded columns included)"
            pairs.append(("gates", g[..., :H], ref["gates"], r32["gates"]))
        else:
            pairs.append((k, out[k], ref[k], r32[k]))
    if "dX" in out:
        if dX:
            pairs.append(("dX", out["dX"], ref["dX"], r32["dX"]))
        else:
            assert np.all(np.isnan(out["dX"])), f"{tag}: dX written although it was not passed"
        for i, n in enumerate(names):
            if grads == "all" or (grads is not None and divmod(i, NW[kind]) in grads):
                pairs.append((n, out["grads"][i], ref["grads"][i], r32["grads"][i]))
            else:
                assert np.all(np.isnan(out["grads"][i])), f"{tag}: {n} written although it was not passed"
    return pairs


def check(kind, out, ref, tag, **kw):
    """Every requested output against float64 within the bound."""
    pairs = pairs_of(kind, out, ref, tag, **kw)
    shares = {}
    for k, got, want, _ in pairs:
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert not np.any(np.isnan(got)), f"{tag}: NaN left in {k}"
        shares[k] = share(got, want)
    fwd = max([v for k, v in shares.items() if k in FORWARD_OUT[kind]] + [0.0])
    gr = max([v for k, v in shares.items() if k not in FORWARD_OUT[kind] and k != "dX"] + [0.0])
    print(f"\n[share of the 1e-4 bound] {tag}: forward {100 * fwd:.1f} %  dX {100 * shares.get('dX', 0.0):.1f} %  "
          f"worst gradient {100 * gr:.1f} %  rms(Y) {rms_of(ref['Y']):.3f}")
    for k, got, want, want32 in pairs:
        assert_within(got, want, bound_for(want, want32, f"{tag}: {k}"), f"{tag}: {k}")


def run_and_check(kind, seed, B, T, n_in, H, ndir=1, nl="tanh", rnl="sigmoid", dyl=True, state=False, tag=None, wide=3.0):
    d = make_inputs(kind, seed, B, T, n_in, H, ndir, state=state, wide=wide)
    dYl = d["dYl"] if dyl else None
    out = run_abi(kind, d["X"], d["params"], d["dY"], dYl, d.get("h0"), nl, rnl)
    ref = reference(kind, d["X"], d["params"], d["dY"], dYl, d.get("h0"), nl, rnl)
    check(kind, out, ref, tag or f"{kind} x{ndir} B {B} T {T} in {n_in} H {H} {nl}/{rnl}")
    return d, out, ref


# --------------------------------------------------------------------------------------------------------------- tier matrix
TIER_H = [1, 16, 17, 50, 112, 128, 129, 144, 200, 256, 257, 400, 512]


@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", TIER_H)
def test_tier_matrix(H, kind, ndir):
    """Every kernel instance and tile-occupancy pattern of the table above: B = 33 (two full 16-row workgroups and one with a single
    row), T = 9 (odd: both LDS h buffers end up as the source of the last step), dY and dYlast in ONE backward call, h0 given on the
    odd sizes."""
    run_and_check(kind, 1000 + H, 33, 9, 24, H, ndir, state=H % 2 == 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 15, 16, 17])
@pytest.mark.parametrize("H", [50, 144])
def test_batch_edges(H, B, kind):
    run_and_check(kind, 1500 + H + B, B, 9, 24, H, 2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_in", [1, 3])
@pytest.mark.parametrize("H", [50, 144])
def test_small_in_features(H, n_in, kind):
    """The whole-sequence GEMMs around the recurrence with K = in (projection), N = in (dX), M = in (dW_x) of 1 and 3."""
    run_and_check(kind, 3000 + H + n_in, 33, 9, n_in, H, 2)


# ----------------------------------------------------------------------------------------------------------- activation grid
@pytest.mark.parametrize("rnl", ["tanh", "sigmoid", "relu"])
@pytest.mark.parametrize("nl", ["tanh", "sigmoid", "relu"])
def test_gru_activation_grid(nl, rnl):
    """All nine pairs at H = 144: nine tiles, wave 0 owns two and the others one."""
    run_and_check("gru", 2000, 20, 12, 16, 144, 1, nl, rnl, wide=1.0)


@pytest.mark.parametrize("nl", ["tanh", "sigmoid", "relu"])
def test_rnn_activations(nl):
    run_and_check("rnn", 2001, 20, 12, 16, 144, 1, nl, nl, wide=1.0)


def test_gru_relu_derivative_at_zero():
    """relu' is 0 at x <= 0 (gru.py:399-401), and the kernels take it from the ACTIVATED value: pinned at pre-activations of exactly +0,
    -0, the smallest positive normal and a negative value.  H = 16, in = 1, T = 1, X = 1, h0 = 1, W_hz = W_hr = 0 and W_hh = diag(0.5),
    so the z and r pre-activations are W_x + b exactly and the candidate's is W_h + b_h + 0.5 r; nl = rnl = relu.  Per hidden unit:
       0..3   r = 0 (so c's pre-activation is W_h + b_h), z = 0.25, c: +0 / -0 (W_h = b_h = -0) / tiny / -0.5   -> dG_h is 0, 0, 0.75 hd, 0
       4      z = +0                       -> dG_z = 0 although hd (h0 - c) != 0
       5      z = tiny                     -> dG_z = hd (h0 - c)
       6      r = +0, c = 0.25             -> dG_r = 0 although (dc W_hh^T) h0 != 0
       7      r = tiny                     -> dG_r = (dc W_hh^T) h0
       8..15  controls, everything positive.
    With T = 1 and B rows of X = 1, db = dW_x = the sum over rows of dG: entries that are products with an exact zero are asserted to be
    exactly zero, everything against float64."""
    tiny = np.float32(np.finfo(np.float32).tiny)
    H, B = 16, 3
    z = np.full(H, 0.25, np.float32); r = np.full(H, 1.0, np.float32); c = np.full(H, 0.25, np.float32)
    r[0:4] = 0.0
    c[0:4] = [0.0, -0.0, tiny, -0.5]
    z[4], z[5], r[6], r[7] = 0.0, tiny, 0.0, tiny
    zero = np.zeros((H, H), np.float32)
    bias = [np.zeros(H, np.float32) for _ in range(3)]
    bias[2][1] = -0.0
    params = [[z[None].copy(), r[None].copy(), c[None].copy(), zero, zero, (0.5 * np.eye(H)).astype(np.float32), *bias]]
    X = np.ones((B, 1, 1), np.float32)
    h0 = np.ones((1, B, H), np.float32)
    dY = np.random.default_rng(7).uniform(0.5, 1.0, (1, B, 1, H)).astype(np.float32)
    out = run_abi("gru", X, params, dY, None, h0, "relu", "relu")
    ref = reference("gru", X, params, dY, None, h0, "relu", "relu")
    check("gru", out, ref, "gru relu'(0)")
    dbz, dbr, dbh = out["grads"][6], out["grads"][7], out["grads"][8]
    assert np.all(dbh[[0, 1, 3]] == 0) and dbh[2] > 0, dbh
    assert dbz[4] == 0 and dbz[5] != 0, dbz
    assert dbr[6] == 0 and dbr[7] != 0, dbr
    assert np.all(out["grads"][2][0, [0, 1, 3]] == 0) and out["grads"][0][0, 4] == 0 and out["grads"][1][0, 6] == 0


def test_rnn_relu_derivative_at_zero():
    """The same for the RNN (rnn.py:234-236): h = relu(W + b) with W_h = 0; units 0..3 at +0 / -0 / tiny / -0.5 -> ds is 0, 0, hd, 0."""
    tiny = np.float32(np.finfo(np.float32).tiny)
    H, B = 16, 3
    w = np.full(H, 0.25, np.float32)
    w[0:4] = [0.0, -0.0, tiny, -0.5]
    b = np.zeros(H, np.float32)
    b[1] = -0.0
    params = [[w[None].copy(), np.zeros((H, H), np.float32), b]]
    X = np.ones((B, 1, 1), np.float32)
    dY = np.random.default_rng(8).uniform(0.5, 1.0, (1, B, 1, H)).astype(np.float32)
    out = run_abi("rnn", X, params, dY, None, None, "relu")
    ref = reference("rnn", X, params, dY, None, None, "relu")
    check("rnn", out, ref, "rnn relu'(0)")
    db = out["grads"][2]
    assert np.all(db[[0, 1, 3]] == 0) and db[2] > 0 and np.all(db[4:] > 0), db


# ----------------------------------------------------------------------------------------------------------------- long T
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", [128, 200])
def test_long_sequence(H, kind):
    """T = 256 in both directions: a stale h or a swapped LDS buffer late in a sequence."""
    run_and_check(kind, 4000 + H, 20, 256, 16, H, 2, wide=1.0)


# ------------------------------------------------------------------------------------------------------------- ABI contract
@pytest.mark.parametrize("kind", KINDS)
def test_abi_null_bias_is_zero_bias(kind):
    d = make_inputs(kind, 5000, 17, 5, 6, 50, 2)
    n = NW[kind]
    nb = n // 3
    with_null = [p[:n - nb] + [None] * nb for p in d["params"]]
    with_zero = [p[:n - nb] + [np.zeros(50, np.float32)] * nb for p in d["params"]]
    a = run_abi(kind, d["X"], with_null, d["dY"], d["dYl"])
    b = run_abi(kind, d["X"], with_zero, d["dY"], d["dYl"])
    for k in FORWARD_OUT[kind] + ("dX",):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for x, y in zip(a["grads"], b["grads"]):
        np.testing.assert_array_equal(x, y)
    check(kind, a, reference(kind, d["X"], with_zero, d["dY"], d["dYl"]), f"{kind} NULL bias")


@pytest.mark.parametrize("kind", KINDS)
def test_abi_null_gradient_pointers_leave_buffers_unwritten(kind):
    d = make_inputs(kind, 5100, 17, 5, 6, 50, 2)
    ref = reference(kind, d["X"], d["params"], d["dY"], d["dYl"])
    n = NW[kind]
    some = {(0, 0), (1, n // 3), (1, n - 1)}
    out = run_abi(kind, d["X"], d["params"], d["dY"], d["dYl"], grads=some, want_dX=False)
    check(kind, out, ref, f"{kind} three gradients, no dX", dX=False, grads=some)
    out = run_abi(kind, d["X"], d["params"], d["dY"], d["dYl"], grads=None)
    check(kind, out, ref, f"{kind} grads = NULL", grads=None)
    out = run_abi(kind, d["X"], d["params"], d["dY"], d["dYl"], want_hT=False, backward=False)
    check(kind, out, ref, f"{kind} hT = NULL", forward=FORWARD_OUT[kind][:-1])


@pytest.mark.parametrize("kind", KINDS)
def test_abi_aliased_state(kind):
    """hT = h0 (the cycled contract): the state buffer holds the last state afterwards, the outputs are those of the plain call."""
    d = make_inputs(kind, 5200, 33, 9, 6, 144, 2, state=True)
    a = run_abi(kind, d["X"], d["params"], h0=d["h0"], backward=False)
    b = run_abi(kind, d["X"], d["params"], h0=d["h0"], alias_state=True, backward=False)
    for k in FORWARD_OUT[kind]:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", [50, 144])
def test_backward_is_linear_in_its_two_gradients(H, kind):
    """One backward with dY and dYlast equals the sum of a dY-only and a dYlast-only call (return_sequences="both" relies on it), for dX
    and every parameter gradient of both directions, within assert_close_scaled(1e-5) -- the sum of two rounded results against one
    rounded result, the bound of the LSTM's test of the same name; the one call is also held to float64; and dYlast = g equals a dY
    that is zero except at the last step, bit for bit."""
    B, T = 33, 9
    d = make_inputs(kind, 5300 + H, B, T, 24, H, 2)
    both = run_abi(kind, d["X"], d["params"], d["dY"], d["dYl"])
    only_all = run_abi(kind, d["X"], d["params"], d["dY"], None)
    only_last = run_abi(kind, d["X"], d["params"], None, d["dYl"])
    assert_close_scaled(only_all["dX"].astype(np.float64) + only_last["dX"], both["dX"], tol=1e-5, err_msg="dX")
    for n, a, b, c in zip(grad_names(kind, 2), only_all["grads"], only_last["grads"], both["grads"]):
        assert_close_scaled(a.astype(np.float64) + b, c, tol=1e-5, err_msg=n)
    check(kind, both, reference(kind, d["X"], d["params"], d["dY"], d["dYl"]), f"{kind} H {H} dY + dYlast in one call")
    check(kind, only_last, reference(kind, d["X"], d["params"], None, d["dYl"]), f"{kind} H {H} dYlast alone")
    z = np.zeros_like(d["dY"])
    z[:, :, T - 1] = d["dYl"]
    as_all = run_abi(kind, d["X"], d["params"], z, None)
    np.testing.assert_array_equal(as_all["dX"], only_last["dX"])
    for a, b in zip(as_all["grads"], only_last["grads"]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", [50, 144])
def test_directions_are_bit_identical_to_single_direction_calls(H, kind):
    """Direction 0 of an ndir = 2 call is bit-identical to the plain ndir = 1 call, and direction 1 to an ndir = 1 call on the
    time-flipped input with its output compared index for index (the reverse output is not flipped back); the saved tensors and dX
    are compared flipped back.  dX of the two-direction call is the sum of both contributions, so each direction's is isolated by
    giving the other a zero gradient (its contribution is then exactly zero)."""
    d = make_inputs(kind, 5400 + H, 33, 9, 24, H, 2, state=True)
    X, P, h0 = d["X"], d["params"], d["h0"]
    Xf = np.ascontiguousarray(X[:, ::-1])
    zero = np.zeros_like(d["dY"][:1])
    zl = np.zeros_like(d["dYl"][:1])
    two = run_abi(kind, X, P, d["dY"], d["dYl"], h0)
    for dd, Xd in ((0, X), (1, Xf)):
        one = run_abi(kind, Xd, [P[dd]], d["dY"][dd:dd + 1], d["dYl"][dd:dd + 1], h0[dd:dd + 1])
        flip = (lambda a: a[:, ::-1]) if dd else (lambda a: a)
        np.testing.assert_array_equal(two["Y"][dd], one["Y"][0], err_msg=f"Y[{dd}]")
        np.testing.assert_array_equal(two["hT"][dd], one["hT"][0], err_msg=f"hT[{dd}]")
        np.testing.assert_array_equal(two["hprev"][dd], flip(one["hprev"][0]), err_msg=f"hprev[{dd}]")
        if kind == "gru":
            np.testing.assert_array_equal(two["gates"][dd], flip(one["gates"][0]), err_msg=f"gates[{dd}]")
        dY2 = np.concatenate([d["dY"][:1], zero] if dd == 0 else [zero, d["dY"][1:]])
        dYl2 = np.concatenate([d["dYl"][:1], zl] if dd == 0 else [zl, d["dYl"][1:]])
        iso = run_abi(kind, X, P, dY2, dYl2, h0, grads=None)
        np.testing.assert_array_equal(iso["dX"], flip(one["dX"]), err_msg=f"dX of direction {dd}")
    # bit-identical reruns: no atomics anywhere
    again = run_abi(kind, X, P, d["dY"], d["dYl"], h0)
    for k in FORWARD_OUT[kind] + ("dX",):
        np.testing.assert_array_equal(again[k], two[k], err_msg=k)
    for a, b in zip(again["grads"], two["grads"]):
        np.testing.assert_array_equal(a, b)


def test_argument_refusals():
    """Refused before anything is launched: the outputs stay NaN."""
    from neunet_hip._lib import NeunetHipError
    d = make_inputs("gru", 5500, 2, 3, 4, 8)
    import torch
    from gru_abi import structs
    from lstm_abi import Fenced, dev
    from neunet_hip._lib import call_hip_function
    x = dev(d["X"])
    pd = [[dev(a) for a in d["params"][0]]]
    w, _ = structs("gru", pd)
    Y, g, hp = Fenced(1, 2, 3, 8), Fenced(1, 2, 3, 48), Fenced(1, 2, 3, 8)
    bad = [dict(ndir=3), dict(ndir=0), dict(H=513), dict(T=0), dict(nl=3)]
    for b in bad:
        a = dict(B=2, T=3, n_in=4, H=8, nl=0, rnl=1, ndir=1)
        a.update(b)
        with pytest.raises(NeunetHipError):
            call_hip_function("nnhipGRUForward", x, w, None, Y.view, g.view, hp.view, None, a["B"], a["T"], a["n_in"], a["H"], a["nl"], a["rnl"],
                              a["ndir"], 0)
    with pytest.raises(NeunetHipError):
        call_hip_function("nnhipGRUBackward", x, w, g.view, hp.view, None, None, None, None, 2, 3, 4, 8, 0, 1, 1, 0)
    torch.cuda.synchronize()
    assert Y.untouched() and g.untouched() and hp.untouched()
