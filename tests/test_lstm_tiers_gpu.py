"""GPU: the LSTM recurrences (csrc/recurrent.hip) at every kernel instance and tile pattern, at long T, over the activation grid and
at the edges of the C ABI contract (include/neunet_hip.h, "nn.LSTM"), against the float64 restatement (tests/lstm_ref.py), plus
properties that need no reference.  tests/test_lstm_gpu.py keeps the fixtures and the notebook sizes.

Which hidden size reaches which kernel (host dispatch at the end of recurrent.hip; Hp = H rounded up to 16, a tile = 16 columns of all
four gates, wave w of 8 owns tiles w, w + 8, w + 16, w + 24; add a row here when a tier is added):

    H      Hp    instance <RES, MAXT>     tiles   pattern
    1      16    <false, 1>               1       one tile, 15 padded columns, 7 idle waves
    5      16    <false, 1>               1       11 padded columns
    16     16    <false, 1>               1       exact
    17     32    <false, 1>               2       15 padded columns in the second tile
    100    112   <false, 1>               7       12 padded columns, 1 idle wave
    112    112   <false, 1>               7       exact, 1 idle wave
    127    128   <true, 1>  resident      8       1 padded column
    128    128   <true, 1>  resident      8       exact; <false, 1> with NNHIP_LSTM_RESIDENT=0 (own process: test_non_resident_twin)
    129    144   <false, 2>               9       wave 0 owns two tiles, the others one; 15 padded columns in wave 0's second tile
    130    144   <false, 2>               9       14 padded columns
    144    144   <false, 2>               9       exact (the activation grid's size)
    200    208   <false, 2>               13      waves 0-4 two tiles, 5-7 one; 8 padded columns
    255    256   <false, 2>               16      every wave two tiles, 1 padded column
    256    256   <false, 2>               16      exact
    257    272   <false, 4>               17      wave 0 three tiles, the others two; 15 padded columns; the backward loads the saved
                                                  values after the barrier (MAXT > 2)
    300    304   <false, 4>               19      waves 0-2 three tiles
    384    384   <false, 4>               24      every wave three tiles, exact
    400    400   <false, 4>               25      wave 0 four tiles
    500    512   <false, 4>               32      every wave four tiles, 12 padded columns
    511    512   <false, 4>               32      1 padded column
    512    512   <false, 4>               32      exact

Inputs (lstm_abi.make_inputs): weights U(-3 / sqrt(H), 3 / sqrt(H)), biases U(-0.3, 0.3), data and upstream gradients U(-1, 1), seeded.
Bound: every tensor, forward and backward, within the bound of assert_close_scaled(tol = 1e-4) of float64 -- 1e-4 of max(|ref|,
rms(ref)) per element, the project's "within 1e-4 fp32" for tensors that are not O(1) (test_hip_parity.py).  Every element is compared.

How much of that bound rounding uses.  "ref32": lstm_ref in float32 (the reference's own arithmetic) against float64, on the CPU: the
worst element's share of the bound, over the forward tensors (Y, gates, cell, hprev, hT, cT) / dX / the twelve gradients.  "kernel":
the same figure for the HIP kernels, from a run of this module on an MI355X (every case prints its own shares before it asserts:
run with -s).  Worst case of each group:

    case                                          rms(Y)       ref32: forward / dX / gradients    kernel: forward / dX / gradients
    tier matrix, B 33, T 9, in 24, H >= 5         0.11-0.29    2.9 % / 1.2 % / 3.0 %              8.2 % (H 511) / 2.3 % / 5.0 %
    tier matrix, H = 1                            0.35         0.9 % / 1.7 % / 161 % (db_f)       1.0 % / 2.3 % / 99.5 % (db_f)
    batch edges B 15 / 16 / 32 / 33, H 128 / 200  0.13-0.14    1.8 % / 0.8 % / 1.8 %              1.3 % / 1.2 % / 2.9 %
    in_features 1 / 3 / 5, H 50 / 200             0.10-0.13    1.6 % / 0.8 % / 1.9 %              1.2 % / 1.0 % / 2.7 %
    nine activation pairs, B 20, T 12, H 144      0.024-0.32   1.7 % / 1.2 % / 7.0 % (relu/relu)  1.7 % / 1.8 % / 6.8 % (sigmoid/relu)
    T 256, B 20, in 16, H 128 / 200               0.15 / 0.14  1.8 % / 1.2 % / 2.9 %              1.5 % / 1.8 % / 3.6 %
    T 1024, B 20, in 16, H 128 / 200              0.15 / 0.14  2.0 % / 1.2 % / 7.4 % (dW_hc)      1.6 % / 2.7 % / 5.3 %

Rounding in this contracting recurrence does not compound: T = 1024 looks like T = 9, for the reference and for the kernels, so one bound
serves every length, and a structurally wrong element (wrong row, stale h, dropped tile, padding leaking in) is of the order of the
rms, four orders above it.  The one tensor whose float32 REFERENCE is outside a quarter of the bound is the single-element db_f at
H = 1: a sum of 297 terms that cancels to 9e-4, so "1e-4 of max(|ref|, rms)" is relative to the cancelled value.  bound_for() gives such a
tensor max(project bound, 4 x max|ref32 - ref64|) -- computed from the two references, never from the kernel -- under the asserted
condition that this stays below 1 % of the tensor's rms (here 0.065 %).

That the tests bite was checked with one-line mutants of recurrent.hip (never committed), each run once against this module:
    forward `jt < ntile` -> `jt < (ntile & ~1)` (last tile dropped when the count is odd): test_tier_matrix at every odd tile count
        (H 1, 5, 16, 100, 112, 129, 130, 144, 200, 257, 300, 400) and every other test at H = 144 / 200 / 300, 48 in all;
    the same in the backward's `dG W_h^T` term: the same sizes of test_tier_matrix, 42 tests in all;
    `hnext = hbuf[t < 40 ? (t & 1) ^ 1 : 0]` (stale h late in a sequence): test_long_sequence (all four) and
        test_chunked_sequence_is_bit_identical -- nothing in tests/test_lstm_gpu.py (T <= 28);
    relu' `y >= 0`: test_relu_derivative_at_zero and the five activation pairs with a relu;
    dYlast dropped when dY is given too: test_tier_matrix (all sizes), test_backward_is_linear_in_its_two_gradients and every other
        test that passes both -- nothing in tests/test_lstm_gpu.py (two separate backward calls there);
    a NULL bias read as 1: test_abi_null_bias_is_zero_bias (all four) -- nothing else can express a NULL bias.

The whole module takes about 9 s on an MI355X; slowest: the child process of test_non_resident_twin 1.9 s, T = 1024 at H = 200 1.4 s
(the float64 and float32 BPTT on the CPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lstm_abi import ALL, FORWARD_OUT, GRADS, Fenced, dev, make_inputs, padded, run_abi, run_layer
from lstm_ref import ACT, lstm_backward, lstm_forward
from test_hip_parity import assert_close_scaled, assert_within, rms_of
from test_lstm import NAMES

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def reference_in(dtype, X, params, dY=None, dYl=None, h0=None, c0=None, nl="tanh", rnl="sigmoid"):
    Y, cache = lstm_forward(X, params, h0, c0, nl, rnl, dtype=dtype)
    gates = np.stack([np.stack([ACT[rnl](z[0]), ACT[rnl](z[1]), ACT[rnl](z[2]), ACT[nl](z[3])], 1) for z in cache["z"]], 1)
    ref = dict(Y=Y, gates=gates, cell=np.stack(cache["cs"], 1), hprev=np.stack(cache["hs"][:-1], 1), hT=cache["hs"][-1], cT=cache["cs"][-1])
    if dY is not None or dYl is not None:
        ref["dX"], ref["grads"] = lstm_backward(cache, dY, dYl)
    return ref


def reference(*args, **kw):
    """The float64 restatement, laid out like the C ABI's outputs (gates (B, T, 4, H), activated), with the float32 restatement of the
    same inputs under "f32": what the reference's own rounding does to each tensor (see bound_for)."""
    ref = reference_in(np.float64, *args, **kw)
    ref["f32"] = reference_in(np.float32, *args, **kw)
    return ref


def bound_for(ref64, ref32, what):
    """The project's bound, TOL * max(|ref|, rms(ref)) per element -- unless the float32 REFERENCE alone uses more than a quarter of it
    (a tensor that is one heavily cancelled sum, e.g. the single-element bias gradient at H = 1): then max(that, 4 x max|ref32 -
    ref64|), provided this is still below 1 % of the tensor's rms.  Computed from the two references only, never from the kernel."""
    ref64 = np.asarray(ref64, np.float64)
    bound = TOL * np.maximum(np.abs(ref64), rms_of(ref64)) + 1e-30
    if share(ref32, ref64) > 0.25:
        wide = 4.0 * float(np.max(np.abs(np.asarray(ref32, np.float64) - ref64)))
        assert wide < 0.01 * rms_of(ref64), f"{what}: the float32 reference is {wide / 4:.2e} off float64, rms {rms_of(ref64):.2e}: change the inputs"
        print(f"\n[bound widened from the reference's own float32 error] {what}: 4 x {wide / 4:.2e} = {100 * wide / rms_of(ref64):.3f} % of the rms")
        bound = np.maximum(bound, wide)
    return bound


def share(got, ref):
    """Worst element's |got - ref| as a fraction of the assert_close_scaled(TOL) bound."""
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (TOL * np.maximum(np.abs(ref), rms_of(ref)) + 1e-30)))


def check(out, ref, H, tag, forward=FORWARD_OUT, dX=True, grads=ALL):
    """Every requested output against float64 within the bound; whatever was not requested must not have been written."""
    Hp = padded(H)
    B, T = ref["Y"].shape[:2]
    shares = {}
    pairs = []
    r32 = ref["f32"]
    for k in forward:
        if k == "gates":
            g = out["gates"].reshape(B, T, 4, Hp)
            assert np.all(np.isfinite(g)), f"{tag}: non-finite value in the saved gates (padded columns included)"
            pairs.append(("gates", g[..., :H], ref["gates"], r32["gates"]))
        else:
            pairs.append((k, out[k], ref[k], r32[k]))
    if "dX" in out:
        if dX:
            pairs.append(("dX", out["dX"], ref["dX"], r32["dX"]))
        else:
            assert np.all(np.isnan(out["dX"])), f"{tag}: dX written although it was not passed"
        for i in range(12):
            if grads is not None and i in grads:
                pairs.append((GRADS[i], out["grads"][i], ref["grads"][i], r32["grads"][i]))
            else:
                assert np.all(np.isnan(out["grads"][i])), f"{tag}: {GRADS[i]} ({NAMES[i]}) written although it was not passed"
    for k, got, want, _ in pairs:
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert not np.any(np.isnan(got)), f"{tag}: NaN left in {k}"
        shares[k] = share(got, want)
    fwd = max([v for k, v in shares.items() if k in FORWARD_OUT] + [0.0])
    gr = max([v for k, v in shares.items() if k in GRADS] + [0.0])
    print(f"\n[share of the 1e-4 bound] {tag}: forward {100 * fwd:.1f} %  dX {100 * shares.get('dX', 0.0):.1f} %  "
          f"worst gradient {100 * gr:.1f} %  rms(Y) {rms_of(ref['Y']):.3f}")
    for k, got, want, want32 in pairs:
        assert_within(got, want, bound_for(want, want32, f"{tag}: {k}"), f"{tag}: {k}")


def run_and_check(seed, B, T, n_in, H, nl="tanh", rnl="sigmoid", dyl=True, state=False, tag=None):
    d = make_inputs(seed, B, T, n_in, H, state=state)
    dYl = d["dYl"] if dyl else None
    out = run_abi(d["X"], d["params"], d["dY"], dYl, d.get("h0"), d.get("c0"), nl, rnl)
    ref = reference(d["X"], d["params"], d["dY"], dYl, d.get("h0"), d.get("c0"), nl, rnl)
    check(out, ref, H, tag or f"B {B} T {T} in {n_in} H {H} {nl}/{rnl}")
    return d, out, ref


# --------------------------------------------------------------------------------------------------------------- tier matrix
TIER_H = [1, 5, 16, 17, 100, 112, 127, 128, 129, 130, 144, 200, 255, 256, 257, 300, 384, 400, 500, 511, 512]


@pytest.mark.parametrize("H", TIER_H)
def test_tier_matrix(H):
    """Every kernel instance and tile-occupancy pattern of the table above: B = 33 (two full 16-row workgroups and one with a single
    row), T = 9 (odd: both LDS h buffers end up as the source of the last step), dY and dYlast in ONE backward call, h0 and c0 given
    on the odd sizes."""
    run_and_check(1000 + H, 33, 9, 24, H, state=H % 2 == 1)


@pytest.mark.parametrize("B", [15, 16, 32, 33])
@pytest.mark.parametrize("H", [128, 200])
def test_batch_edges(B, H):
    run_and_check(1500 + H + B, B, 9, 24, H)


@pytest.mark.parametrize("n_in", [1, 3, 5])
@pytest.mark.parametrize("H", [50, 200])
def test_small_in_features(n_in, H):
    """The whole-sequence GEMMs around the recurrence with K = in (projection), N = in (dX), M = in (dW_x) of 1, 3, 5: row pitches
    that are not multiples of 4 floats."""
    run_and_check(3000 + H + n_in, 33, 9, n_in, H)


def test_non_resident_twin(tmp_path):
    """Hp = 128 with NNHIP_LSTM_RESIDENT=0: lstm_fwd_kernel<false, 1> / lstm_bwd_kernel<false, 1> with all eight waves busy.  The
    library reads the variable once per process, so a fresh child process (tests/lstm_abi.py) runs it; this process runs the same
    inputs on the resident instance.  Both are held to float64 with the same bound; the two sum in different orders, so nothing is
    claimed between them."""
    seed, B, T, n_in, H = 1128, 33, 9, 24, 128
    assert os.environ.get("NNHIP_LSTM_RESIDENT", "1") != "0", "this test needs the default (resident) dispatch in the parent"
    path = str(tmp_path / "nonresident.npz")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "lstm_abi.py"), path, str(seed), str(B),
                        str(T), str(n_in), str(H)], env={**os.environ, "NNHIP_LSTM_RESIDENT": "0"}, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    f = dict(np.load(path, allow_pickle=False))
    assert str(f["resident_env"]) == "0"
    child = {k: f[k] for k in FORWARD_OUT + ("dX",)}
    child["grads"] = [f[n] for n in GRADS]
    d = make_inputs(seed, B, T, n_in, H)
    ref = reference(d["X"], d["params"], d["dY"], d["dYl"])
    check(child, ref, H, "H 128 non-resident (child process)")
    out = run_abi(d["X"], d["params"], d["dY"], d["dYl"])
    check(out, ref, H, "H 128 resident")


# ----------------------------------------------------------------------------------------------------------- activation grid
@pytest.mark.parametrize("rnl", ["tanh", "sigmoid", "relu"])
@pytest.mark.parametrize("nl", ["tanh", "sigmoid", "relu"])
def test_activation_grid(nl, rnl):
    """All nine pairs at H = 144: nine tiles, wave 0 owns two and the others one."""
    run_and_check(2000, 20, 12, 16, 144, nl, rnl)


def test_relu_derivative_at_zero():
    """relu' is 0 at x <= 0 (lstm.py:457), and the kernels take it from the ACTIVATED value: pinned at pre-activations of exactly
    +0, -0, the smallest positive normal, and a negative value.  H = 16, in = 1, T = 1, X = 1 and no h0, so a pre-activation is W_x + b
    exactly; nl = rnl = relu.  Per hidden unit (f, i, o, g are pre-activations):
       0..3   f = i = o = 1, c0 = 0.5, g = +0 / -0 (W_c = b_c = -0) / tiny / -0.5      -> dG_c is 0, 0, dY, 0
       4      f = i = o = 1, c0 = -0.25, g = 0.25: c_1 = -0.25 + 0.25 = +0 exactly      -> dc = 0: dG_f = dG_i = dG_c = 0
       5      c0 = 0, g = tiny: c_1 = tiny                                             -> relu'(c_1) = 1: dG_c = dY
       6      c0 = -0.5, g = 0.25: c_1 = -0.25                                         -> dc = 0
       7      control: c0 = 0.5, g = 0.25, everything positive
       8      f = +0 (c0 = 0.5, g = 0.25)                                              -> dG_f = 0 although dc c0 != 0
       9      i = +0                                                                   -> dG_i = 0 although dc g != 0
       10     o = +0                                                                   -> dG_o = 0 although dh relu(c_1) != 0
       11     o = tiny                                                                 -> dG_o = dY relu(c_1)
    (c_1 = -0 cannot be reached observably: f c0 + i g rounds to +0 unless both products are -0, and then every gradient through it is 0
    whatever the derivative.)  With T = 1 and B rows of X = 1, db = sum over rows of dG and dW_x = the same sum: entries that are
    products with an exact zero are asserted to be exactly zero, the others against float64."""
    tiny = np.float32(np.finfo(np.float32).tiny)
    H, B = 16, 3
    nz = np.float32(-0.0)
    f = np.ones(H, np.float32); i = np.ones(H, np.float32); o = np.ones(H, np.float32)
    g = np.full(H, 0.25, np.float32); c0 = np.full(H, 0.5, np.float32)
    g[0:4] = [0.0, nz, tiny, -0.5]
    c0[4], c0[5], c0[6] = -0.25, 0.0, -0.5
    g[5] = tiny
    f[8], i[9], o[10], o[11] = 0.0, 0.0, 0.0, tiny
    bias = [np.zeros(H, np.float32) for _ in range(4)]
    bias[3][1] = nz
    params = [v.reshape(1, H).copy() for v in (f, i, o, g)] + [np.full((H, H), 0.125, np.float32) for _ in range(4)] + bias
    rng = np.random.default_rng(7)
    X = np.ones((B, 1, 1), np.float32)
    dY = rng.uniform(0.25, 1.0, (B, 1, H)).astype(np.float32)          # one sign: a sum of non-zero terms cannot cancel to zero
    c0B = np.tile(c0, (B, 1))
    out = run_abi(X, params, dY, None, None, c0B, "relu", "relu")
    ref = reference(X, params, dY, None, None, c0B, "relu", "relu")
    assert out["cell"][:, 1, 4].tolist() == [0.0] * B and np.all(out["cell"][:, 1, 5] == tiny) and np.all(out["gates"][:, 0, 3 * H + 2] == tiny)
    check(out, ref, H, "relu at zero")
    db = {n: out["grads"][8 + k] for k, n in enumerate("fioc")}
    dw = {n: out["grads"][k][0] for k, n in enumerate("fioc")}
    zero = {"c": [0, 1, 3, 4, 6], "f": [4, 6, 8], "i": [4, 6, 9], "o": [10]}
    for n, units in zero.items():
        for u in units:
            assert db[n][u] == 0.0 and dw[n][u] == 0.0, f"relu' must be 0 here: gate {n}, unit {u}: db {db[n][u]!r}, dW_x {dw[n][u]!r}"
    one = {"c": [2, 5, 7], "f": [7], "i": [7], "o": [11, 7]}
    for n, units in one.items():
        for u in units:
            assert db[n][u] > 0.1, f"relu' must be 1 here: gate {n}, unit {u}: db {db[n][u]!r}"
    s = dY[:, 0].astype(np.float64).sum(0)
    np.testing.assert_allclose([db["c"][2], db["c"][5]], [s[2], s[5]], rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------ long sequences
@pytest.mark.parametrize("T", [256, 1024])
@pytest.mark.parametrize("H", [128, 200])
def test_long_sequence(T, H):
    """A per-step defect (a stale LDS h buffer on odd / even steps, a wrong c carry in padded lanes) compounds over T; rounding does
    not (module docstring), so the bound is the one of T = 9."""
    run_and_check(4000 + T + H, 20, T, 16, H, dyl=False)


# ------------------------------------------------------------------------------------------ properties that need no reference
def forward_only(X, params, h0=None, c0=None, **kw):
    return run_abi(X, params, h0=h0, c0=c0, backward=False, **kw)


def gemm_families():
    """Launches so far per GEMM kernel family (classic 128 x 128, persistent, small-problem, split-bf16)."""
    from neunet_hip._lib import call_hip_function
    return np.array([int(call_hip_function("nnhipGemmLaunchCount", k)) for k in range(4)])


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("H", [128, 300])
def test_chunked_sequence_is_bit_identical(H, alias):
    """One call over T = 64 equals two calls over T = 32 chained hT -> h0, cT -> c0, bit for bit in Y, hT, cT (and the saved cell
    states): same recurrence instance, same per-step arithmetic, only where the state sits between steps 31 and 32 differs (LDS and
    registers against global memory).  alias: the chained calls pass hT == h0 and cT == c0, the cycled-state contract.

    The premise is that the projection P = X W_x + b is the same for a row whatever M = B T is, and that holds only within one GEMM
    kernel family.  Found with this test at (B, in) = (20, 16), H = 128: the T = 32 projection (640 x 512, K = 16: 320 tiles of 32 x 32)
    takes the small-problem kernel, the T = 64 one (640 tiles, over gemm_small_wanted's limit of 512) the classic 128 x 128 kernel,
    whose k-sums round differently; Y then differs from step 0 on, by at most 1.6e-7, and the recurrence is not involved (at H = 300
    both projections were classic and everything was bit-identical).  So in = 80 here: K > 64 and more than eight 128 x 128 tiles put
    all three projections on the classic kernel, which the launch counters confirm before anything is compared."""
    B, T, n_in = 20, 64, 80
    d = make_inputs(5000 + H, B, T, n_in, H, state=True)
    fam = [gemm_families()]
    whole = forward_only(d["X"], d["params"], d["h0"], d["c0"])
    fam.append(gemm_families())
    a = forward_only(d["X"][:, :32], d["params"], d["h0"], d["c0"], alias_state=alias)
    fam.append(gemm_families())
    b = forward_only(d["X"][:, 32:], d["params"], a["hT"], a["cT"], alias_state=alias)
    fam.append(gemm_families())
    used = [tuple(y - x) for x, y in zip(fam, fam[1:])]
    assert used[0] == used[1] == used[2] and sum(used[0]) == 1, f"the three projections ran on different GEMM kernels: {used}"
    np.testing.assert_array_equal(np.concatenate([a["Y"], b["Y"]], 1), whole["Y"])
    np.testing.assert_array_equal(b["hT"], whole["hT"])
    np.testing.assert_array_equal(b["cT"], whole["cT"])
    np.testing.assert_array_equal(b["cell"][:, 0], a["cT"])
    np.testing.assert_array_equal(b["hprev"][:, 0], a["hT"])
    np.testing.assert_array_equal(np.concatenate([a["cell"], b["cell"][:, 1:]], 1), whole["cell"])
    np.testing.assert_array_equal(np.concatenate([a["hprev"], b["hprev"]], 1), whole["hprev"])


@pytest.mark.parametrize("H", [128, 200])
def test_batch_rows_are_independent(H):
    """Batch rows never meet (recurrent.hip: one workgroup per 16 rows, no communication).  The same 33 rows permuted give the permuted
    outputs bit for bit (the projection GEMM has the same M, so the same instance, and a row's k-sum order does not depend on where
    the row sits); rows 0, 15 and 32 run alone as B = 1 equal their rows of the B = 33 run within 1e-6 absolute (another M may select
    another GEMM instance: 1e-6 is about 8 ulp at |h| <= 1, five orders below a wrong row)."""
    B, T, n_in = 33, 9, 24
    d = make_inputs(6000 + H, B, T, n_in, H, state=True)
    base = forward_only(d["X"], d["params"], d["h0"], d["c0"])
    perm = np.random.default_rng(1).permutation(B)
    assert np.any(perm // 16 != np.arange(B) // 16)                      # rows change workgroup
    p = forward_only(d["X"][perm], d["params"], d["h0"][perm], d["c0"][perm])
    for k in ("Y", "cell", "hprev", "hT", "cT"):
        np.testing.assert_array_equal(p[k], base[k][perm], err_msg=k)
    for r in (0, 15, 32):
        one = forward_only(d["X"][r:r + 1], d["params"], d["h0"][r:r + 1], d["c0"][r:r + 1])
        for k in ("Y", "cell", "hprev", "hT", "cT"):
            np.testing.assert_allclose(one[k][0], base[k][r], rtol=0, atol=1e-6, err_msg=f"{k} row {r}")


def test_padding_is_inert():
    """H = 100 and H = 112 with the weights zero-extended share Hp = 112 and the kernel instance: the first 100 units are bit-identical
    and the twelve extra units (zero weights, zero bias, nl = tanh: g = tanh(0) = 0, c stays 0) output exactly 0."""
    B, T, n_in, H, H2 = 33, 9, 24, 100, 112
    d = make_inputs(7000, B, T, n_in, H)
    ext = [np.zeros((n_in, H2), np.float32) for _ in range(4)] + [np.zeros((H2, H2), np.float32) for _ in range(4)] + \
          [np.zeros(H2, np.float32) for _ in range(4)]
    for e, a in zip(ext, d["params"]):
        e[tuple(slice(0, n) for n in a.shape)] = a
    small = forward_only(d["X"], d["params"])
    big = forward_only(d["X"], ext)
    np.testing.assert_array_equal(big["Y"][:, :, :H], small["Y"])
    np.testing.assert_array_equal(big["cell"][:, :, :H], small["cell"])
    assert not np.any(big["Y"][:, :, H:]) and not np.any(big["cell"][:, :, H:]) and not np.any(big["hT"][:, H:])


@pytest.mark.parametrize("H", [128, 200, 300])
def test_backward_is_linear_in_its_two_gradients(H):
    """One backward with dY and dYlast equals the sum of a dY-only and a dYlast-only call (return_sequences="both" relies on it) within
    assert_close_scaled(1e-5) (the sum of two rounded results against one rounded result); and dYlast = g equals a dY that is zero
    except dY[:, T-1] = g, bit for bit."""
    B, T, n_in = 33, 9, 24
    d = make_inputs(8000 + H, B, T, n_in, H)
    both = run_abi(d["X"], d["params"], d["dY"], d["dYl"])
    only_all = run_abi(d["X"], d["params"], d["dY"], None)
    only_last = run_abi(d["X"], d["params"], None, d["dYl"])
    assert_close_scaled(only_all["dX"].astype(np.float64) + only_last["dX"], both["dX"], tol=1e-5, err_msg="dX")
    for i in range(12):
        assert_close_scaled(only_all["grads"][i].astype(np.float64) + only_last["grads"][i], both["grads"][i], tol=1e-5, err_msg=GRADS[i])
    ref = reference(d["X"], d["params"], None, d["dYl"])
    check(only_last, ref, H, f"dYlast alone, H {H}")
    z = np.zeros_like(d["dY"])
    z[:, T - 1] = d["dYl"]
    as_all = run_abi(d["X"], d["params"], z, None)
    np.testing.assert_array_equal(as_all["dX"], only_last["dX"])
    for i in range(12):
        np.testing.assert_array_equal(as_all["grads"][i], only_last["grads"][i], err_msg=GRADS[i])


# ------------------------------------------------------------------------------------------------------------ C ABI contract
ABI_SHAPE = dict(B=17, T=6, n_in=10)


def abi_inputs(H, seed=9000):
    return make_inputs(seed + H, ABI_SHAPE["B"], ABI_SHAPE["T"], ABI_SHAPE["n_in"], H, state=True)


@pytest.mark.parametrize("H", [50, 200])
@pytest.mark.parametrize("null_bias", [(0, 1, 2, 3), (2,)])
def test_abi_null_bias_is_zero_bias(H, null_bias):
    d = abi_inputs(H)
    params = [None if i - 8 in null_bias else a for i, a in enumerate(d["params"])]
    out = run_abi(d["X"], params, d["dY"], d["dYl"], d["h0"], d["c0"])
    ref = reference(d["X"], params, d["dY"], d["dYl"], d["h0"], d["c0"])
    check(out, ref, H, f"b NULL for gates {null_bias}, H {H}")


@pytest.mark.parametrize("H", [50, 200])
@pytest.mark.parametrize("given", ["h0", "c0"])
def test_abi_one_initial_state(H, given):
    d = abi_inputs(H)
    h0, c0 = (d["h0"], None) if given == "h0" else (None, d["c0"])
    out = run_abi(d["X"], d["params"], d["dY"], d["dYl"], h0, c0)
    check(out, reference(d["X"], d["params"], d["dY"], d["dYl"], h0, c0), H, f"{given} alone, H {H}")


@pytest.mark.parametrize("H", [50, 200])
def test_abi_null_outputs(H):
    """hT / cT NULL; dX NULL; grads NULL (only dX written); a grads struct with only dwh[2] and db[0] set (those right, every other
    gradient buffer and all the guard words around the two still NaN)."""
    d = abi_inputs(H)
    ref = reference(d["X"], d["params"], d["dY"], d["dYl"], d["h0"], d["c0"])
    args = (d["X"], d["params"], d["dY"], d["dYl"], d["h0"], d["c0"])
    out = run_abi(*args, want_hT=False, want_cT=False, want_dX=False)
    assert out["hT"] is None and out["cT"] is None
    check(out, ref, H, f"hT, cT, dX NULL, H {H}", forward=("Y", "gates", "cell", "hprev"), dX=False)
    out = run_abi(*args, want_hT=True, want_cT=False, grads=None)
    check(out, ref, H, f"cT NULL, grads NULL, H {H}", forward=("Y", "gates", "cell", "hprev", "hT"), grads=None)
    out = run_abi(*args, want_hT=False, want_cT=True, grads=(6, 8))
    check(out, ref, H, f"hT NULL, grads = dwh[2], db[0], H {H}", forward=("Y", "gates", "cell", "hprev", "cT"), grads=(6, 8))


@pytest.mark.parametrize("H", [200, 300])
def test_abi_aliased_state(H):
    """hT == h0 and cT == c0 where a wave owns several tiles: every workgroup must have read its rows of h0 / c0 before any thread
    overwrites them."""
    d = abi_inputs(H)
    out = run_abi(d["X"], d["params"], d["dY"], d["dYl"], d["h0"], d["c0"], alias_state=True)
    check(out, reference(d["X"], d["params"], d["dY"], d["dYl"], d["h0"], d["c0"]), H, f"aliased state, H {H}")


def test_abi_refusals():
    """Argument errors are host-side checks that return before any launch: the documented status, a message, every output still NaN,
    the device error word still clear."""
    import ctypes
    import torch
    from neunet_hip import _lib
    EINVAL, EALIGN = -1, -2
    B, T, n_in, H = 17, 6, 10, 50
    d = make_inputs(9500, B, T, n_in, H, state=True)
    x, pd = dev(d["X"]), [dev(a) for a in d["params"]]
    dY, dYl, h0, c0 = dev(d["dY"]), dev(d["dYl"]), dev(d["h0"]), dev(d["c0"])
    Hp = padded(512)                                            # buffers large enough for whatever H a refused call names
    outs = dict(Y=Fenced(B, T, 513), gates=Fenced(B, T, 4 * (Hp + 16)), cell=Fenced(B, T + 1, 513), hprev=Fenced(B, T, 513), hT=Fenced(B, 513),
                cT=Fenced(B, 513), dX=Fenced(B, T, n_in), **{n: Fenced(513, 513) for n in GRADS})
    # saved state for the backward refusals: a real forward
    saved = {}
    run_abi(d["X"], d["params"], None, None, d["h0"], d["c0"], backward=False, raw=saved)

    def weights(shift=None):
        w = _lib.LSTMWeights()
        for g in range(4):
            w.wx[g], w.wh[g], w.b[g] = pd[g].data_ptr(), pd[4 + g].data_ptr(), pd[8 + g].data_ptr()
        if shift:
            getattr(w, shift[0])[shift[1]] += 2
        return w

    def grads_struct(shift=None):
        g = _lib.LSTMGrads()
        for i, n in enumerate(GRADS):
            (g.dwx, g.dwh, g.db)[i // 4][i % 4] = outs[n].view.data_ptr() + (2 if shift == n else 0)
        return g

    def ptr(t, off=0):
        return None if t is None else ctypes.c_void_p(t.data_ptr() + off)

    fwd = _lib.load_hip_function("nnhipLSTMForward")
    bwd = _lib.load_hip_function("nnhipLSTMBackward")
    st = _lib.get_current_stream_ptr()

    def forward(B=B, T=T, n_in=n_in, H=H, nl=0, rnl=1, w=None, off=None):
        o = lambda name, t: ptr(t, 2 if off == name else 0)
        w = w or weights()
        return fwd(o("X", x), ctypes.byref(w), o("h0", h0), o("c0", c0), o("Y", outs["Y"].view), o("gates", outs["gates"].view),
                   o("cell", outs["cell"].view), o("hprev", outs["hprev"].view), o("hT", outs["hT"].view), o("cT", outs["cT"].view), B, T, n_in,
                   H, nl, rnl, st)

    def backward(B=B, T=T, n_in=n_in, H=H, nl=0, rnl=1, w=None, off=None, dy=dY, dyl=dYl, g=None):
        o = lambda name, t: ptr(t, 2 if off == name else 0)
        w = w or weights()
        g = g or grads_struct()
        return bwd(o("X", x), ctypes.byref(w), o("gates", saved["gates"].view), o("cell", saved["cell"].view), o("hprev", saved["hprev"].view),
                   o("dY", dy), o("dYlast", dyl), o("dX", outs["dX"].view), ctypes.byref(g), B, T, n_in, H, nl, rnl, st)

    cases = [("forward hidden 513", lambda: forward(H=513), EINVAL), ("forward T 0", lambda: forward(T=0), EINVAL),
             ("forward B 0", lambda: forward(B=0), EINVAL), ("forward in 0", lambda: forward(n_in=0), EINVAL),
             ("forward nonlinearity 3", lambda: forward(nl=3), EINVAL), ("forward recurrent nonlinearity 3", lambda: forward(rnl=3), EINVAL),
             ("forward nonlinearity -1", lambda: forward(nl=-1), EINVAL),
             ("backward hidden 513", lambda: backward(H=513), EINVAL), ("backward T 0", lambda: backward(T=0), EINVAL),
             ("backward B 0", lambda: backward(B=0), EINVAL), ("backward nonlinearity 3", lambda: backward(nl=3), EINVAL),
             ("backward dY and dYlast NULL", lambda: backward(dy=None, dyl=None), EINVAL)]
    cases += [(f"forward {n} + 2 bytes", (lambda n=n: forward(off=n)), EALIGN) for n in ("X", "h0", "c0", "Y", "gates", "cell", "hprev", "hT", "cT")]
    cases += [(f"backward {n} + 2 bytes", (lambda n=n: backward(off=n)), EALIGN) for n in ("X", "gates", "cell", "hprev", "dY", "dYlast", "dX")]
    cases += [("forward wh[1] + 2 bytes", lambda: forward(w=weights(("wh", 1))), EALIGN), ("forward b[3] + 2 bytes", lambda: forward(w=weights(("b", 3))), EALIGN),
              ("backward wx[0] + 2 bytes", lambda: backward(w=weights(("wx", 0))), EALIGN),
              ("backward dwh[2] + 2 bytes", lambda: backward(g=grads_struct("dwh2")), EALIGN),
              ("backward db[0] + 2 bytes", lambda: backward(g=grads_struct("db0")), EALIGN)]
    saved_before = {k: saved[k].host() for k in ("gates", "cell", "hprev")}
    for name, call, status in cases:
        rc = call()
        assert rc == status, f"{name}: status {rc}, expected {status} ({_lib.last_error()})"
        assert _lib.last_error(), f"{name}: no error message"
    torch.cuda.synchronize()
    for n, o in outs.items():
        assert o.untouched(), f"a refused call wrote to {n}"
    for k, v in saved_before.items():
        np.testing.assert_array_equal(saved[k].host(), v)
    _lib.call_hip_function("nnhipDeviceError")


# -------------------------------------------------------------------------------------------------------------- Python layer
def test_layer_matches_abi_and_float64():
    """nn.LSTM (return_sequences "both": two backward passes that add up) against float64 and, in the forward, bit for bit against the
    C ABI call it makes."""
    B, T, n_in, H = 33, 9, 24, 200
    d = make_inputs(9700, B, T, n_in, H)
    lay = run_layer(d["X"], d["params"], d["dY"], d["dYl"])
    ref = reference(d["X"], d["params"], d["dY"], d["dYl"])
    abi = run_abi(d["X"], d["params"], backward=False)
    np.testing.assert_array_equal(lay["Y"], abi["Y"])
    np.testing.assert_array_equal(lay["hT"], abi["hT"])
    assert_close_scaled(lay["Y"], ref["Y"], tol=TOL, err_msg="Y")
    assert_close_scaled(lay["dX"], ref["dX"], tol=TOL, err_msg="dX")
    for i in range(12):
        assert_close_scaled(lay["grads"][i], ref["grads"][i].reshape(lay["grads"][i].shape), tol=TOL, err_msg=NAMES[i])


def test_layer_input_without_grad():
    """X with requires_grad=False: the backward passes dX = NULL; x.grad stays None and the parameter gradients are right."""
    B, T, n_in, H = 17, 6, 10, 200
    d = make_inputs(9701, B, T, n_in, H)
    lay = run_layer(d["X"], d["params"], d["dY"], None, x_requires_grad=False)
    assert lay["x"].grad is None and lay["dX"] is None
    ref = reference(d["X"], d["params"], d["dY"], None)
    assert_close_scaled(lay["Y"], ref["Y"], tol=TOL, err_msg="Y")
    for i in range(12):
        assert_close_scaled(lay["grads"][i], ref["grads"][i].reshape(lay["grads"][i].shape), tol=TOL, err_msg=NAMES[i])


def test_layer_non_contiguous_input_and_gradient(hip):
    """X a transposed view of a (T, B, in) array, the upstream gradient a view of a (B, T, 2H) array."""
    import torch
    import neunet_hip.nn as nn
    B, T, n_in, H = 17, 6, 10, 200
    d = make_inputs(9702, B, T, n_in, H)
    m = nn.LSTM(n_in, H, return_sequences=True)
    for p, a in zip(m.parameters(), d["params"]):
        p.data.copy_(dev(a))
    xt = dev(d["X"].transpose(1, 0, 2)).transpose(0, 1)
    assert not xt.is_contiguous() and tuple(xt.shape) == (B, T, n_in)
    x = hip.Tensor(xt, device="cuda", _nocopy=True)             # wrapped as it is: the constructor would copy it contiguous
    assert not x.data.is_contiguous()
    Y = m(x)
    wide = torch.zeros((B, T, 2 * H), dtype=torch.float32, device="cuda")
    wide[:, :, ::2] = dev(d["dY"])
    gview = wide[:, :, ::2]
    assert not gview.is_contiguous()
    # Tensor.backward() copies the seed it is given contiguous; a strided gradient reaches a grad_fn from a consumer op's apply_grad,
    # which keeps it by reference: do what the tape walk does with such a node (autograd.py: v.grad_fn(*v.args, grad=v.grad))
    Y.apply_grad(gview)
    assert not Y.grad.is_contiguous()
    Y.grad_fn(*Y.args, grad=Y.grad)
    torch.cuda.synchronize()
    ref = reference(d["X"], d["params"], d["dY"], None)
    assert_close_scaled(Y.data.cpu().numpy(), ref["Y"], tol=TOL, err_msg="Y")
    assert tuple(x.grad.shape) == (B, T, n_in)
    assert_close_scaled(x.grad.cpu().numpy(), ref["dX"], tol=TOL, err_msg="dX")
    for i, p in enumerate(m.parameters()):
        assert_close_scaled(p.grad.cpu().numpy(), ref["grads"][i].reshape(p.grad.shape), tol=TOL, err_msg=NAMES[i])


def test_layer_cycled_states_over_three_calls(hip):
    """cycled_states=True at H = 200: three calls over consecutive pieces of a sequence equal one float64 pass over the whole."""
    import neunet_hip.nn as nn
    B, T, n_in, H = 17, 18, 10, 200
    d = make_inputs(9703, B, T, n_in, H)
    m = nn.LSTM(n_in, H, return_sequences="both", cycled_states=True)
    for p, a in zip(m.parameters(), d["params"]):
        p.data.copy_(dev(a))
    Yr, cache = lstm_forward(d["X"], d["params"])
    for k, (a, b) in enumerate([(0, 5), (5, 12), (12, 18)]):
        Y, last = m(hip.Tensor(d["X"][:, a:b], device="cuda", requires_grad=False))
        assert_close_scaled(Y.data.cpu().numpy(), Yr[:, a:b], tol=TOL, err_msg=f"Y of call {k}")
        assert_close_scaled(last.data.cpu().numpy().reshape(B, H), Yr[:, b - 1], tol=TOL, err_msg=f"last of call {k}")
        assert_close_scaled(m.hprev.cpu().numpy(), cache["hs"][b], tol=TOL, err_msg=f"carried h after call {k}")
        assert_close_scaled(m.cprev.cpu().numpy(), cache["cs"][b], tol=TOL, err_msg=f"carried c after call {k}")
