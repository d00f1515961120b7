"""CPU: tests/fused_step_ref.py against what the project already trusts.

  * reach: the case tables of tests/test_fused_step_gpu.py run every instance of the three one-launch step kernels -- the route
    functions restate the host's choice, and the tables are held to the list of instances here;
  * the float64 restatements equal oracle/neunet_oracle.py evaluated in float64 on the shapes tests/test_hip_parity.py uses;
  * the float32 oracle, on every table case, sits well inside the bounds the kernels are held to (each test prints the largest share).

Largest share of a bound the float32 oracle uses (this file, one run): MLP backward 0.084; Linear + CrossEntropy 0.087 (logits; loss
and dlogits 0.014); BatchNorm head 0.165 (dz; Y 0.050, save_inv 0.057, pred 0.032, running_var 0.104).  The offset-channel case (a
channel with mean 100 and standard deviation 0.01): the float32 two-pass BatchNorm is 1.6e-3 from float64 in Y (rms 0.93) -- the kernel
is allowed 4 x that, 0.69 % of the rms."""
import numpy as np
import pytest

import fused_step_ref as F
from oracle import neunet_oracle as O
from rowops_ref import cross_entropy
from test_gemm_tiers_gpu import dot_bound_of, ratio
from test_rowops_tiers_gpu import close_bound, scaled_bound


# ==================================================================================================== reach
def test_tables_reach_every_mlp_instance():
    seen = {}
    for rows, in1, hid, out2 in F.MLP_CASES:
        fits, nw, u, tail, n = F.mlp_route(rows, in1, hid, out2)
        assert fits, (rows, in1, hid, out2)
        seen.setdefault((nw, u), set()).add((rows, tail))
    assert sorted(seen) == [(4, 1), (4, 8), (8, 1), (8, 8)]
    for inst, rows in F.MLP_INSTANCE_ROWS.items():
        assert {r for r, _ in seen[inst]} == set(rows), inst
    # the staging tail loop runs exactly where 16 rows > 4 BS: never in the one-group instances, always in the eight-group ones -- no
    # instance has both
    assert {t for _, t in seen[(4, 1)]} == {False} and {t for _, t in seen[(8, 1)]} == {False}
    assert {t for _, t in seen[(4, 8)]} == {True} and {t for _, t in seen[(8, 8)]} == {True}
    assert F.mlp_route(64, 16, 16, 16)[3] is False and F.mlp_route(65, 16, 16, 16)[3] is True
    assert F.mlp_route(128, 16, 16, 16)[3] is False and F.mlp_route(129, 16, 16, 16)[3] is True
    # every row count with an exact and a ragged geometry; hid, in1, out2 of the issue's lists all used
    for r in F.MLP_ROWS:
        assert {(r,) + F.G_EXACT, (r,) + F.G_RAGGED} <= set(F.MLP_CASES)
    assert {c[1] for c in F.MLP_CASES} == {1, 15, 16, 17, 90} and {c[2] for c in F.MLP_CASES} == {1, 16, 17, 50}
    assert {c[3] for c in F.MLP_CASES} == {1, 7, 15, 16}
    # the old tests' shapes: two instances only
    assert {F.mlp_route(r, 16, 16, 1)[1:3] for r in (5, 32, 37, 256)} == {(4, 1), (8, 8)}


def test_adam_shapes_reach_the_arrival_board_edges():
    for shape, n, inst in zip(F.MLP_ADAM_SHAPES, F.MLP_ADAM_N, F.MLP_ADAM_INSTANCE):
        fits, nw, u, _, blocks = F.mlp_route(*shape, with_adam=True)
        assert fits and blocks == n and (nw, u) == inst, shape
        want = F.board_wants(n)
        assert sum(want) == n and max(want) - min(want) <= 1
    assert F.board_wants(2) == [1, 1] + [0] * 26 and F.board_wants(27)[-1] == 0 and F.board_wants(28) == [1] * 28
    assert F.board_wants(29)[:2] == [2, 1] and F.board_wants(57)[:2] == [3, 2]
    assert [F.MLP_ADAM_N[i] for i in F.MLP_ADAM_SEQUENCE] == [57, 2, 28, 57]
    # ragged: the `omine` / `bmine` clamps are false somewhere
    assert any(s[1] % 16 and s[2] % 16 for s in F.MLP_ADAM_SHAPES)
    assert {a[0] for a in F.ADAM_AXES} == {0, 1} and {a[1] for a in F.ADAM_AXES} == {0.0, 1e-2} and {a[2] for a in F.ADAM_AXES} == {0, 1, 7}
    assert any(a[3] == 0.5 and a[4] is None for a in F.ADAM_AXES) and any(a[3] == 0.5 and a[4] for a in F.ADAM_AXES)


def test_fits_grid_straddles_every_limit():
    got = [F.mlp_route(*c)[0] for c in F.MLP_FITS_GRID]
    assert got == [True, False, True, False, True, False, True, True, False, True, False, True, True, False, True, False]


def test_tables_reach_every_linear_ce_instance():
    seen = set()
    for rows, K, classes, ox, ow in F.LINCE_CASES:
        assert F.lince_fits(rows, K, classes)
        vec, nw, one, nblk = F.lince_route(rows, K, classes, not (ox or ow))
        seen.add((vec, nw, one))
    assert seen == {(v, nw, one) for v in (False, True) for nw in (4, 8) for one in (False, True)}
    assert F.lince_route(1, 64, 1)[1:3] == (4, True) and F.lince_route(1, 65, 1)[1:3] == (4, False)
    assert F.lince_route(1, 112, 1)[1:3] == (4, False) and F.lince_route(1, 113, 1)[1:3] == (8, True)
    assert F.lince_route(1, 128, 1)[1:3] == (8, True) and F.lince_route(1, 129, 1)[1:3] == (8, False)
    # a K % 4 == 0 operand 4 bytes off: the scalar instance, with one k-group (64) and with several (132)
    assert F.lince_route(33, 64, 17, False)[:3] == (False, 4, True) and F.lince_route(17, 132, 31, False)[:3] == (False, 8, False)
    for K in F.LINCE_K:
        mine = [c for c in F.LINCE_CASES if c[1] == K]
        assert len({c[0] for c in mine}) >= 2 and len({c[2] for c in mine}) >= 2, K
    assert {c[0] for c in F.LINCE_CASES} >= set(F.LINCE_ROWS) and {c[2] for c in F.LINCE_CASES} >= set(F.LINCE_CLASSES)
    assert [F.lince_route(r, 64, 10)[3] for r in F.LINCE_SEQUENCE] == [2, 1, 16, 2]
    assert {(r, w) for r, w, _ in F.LINCE_RUNS} == {(r, w) for r in "nms" for w in (False, True)}
    assert {(r, i) for r, _, i in F.LINCE_RUNS} == {(r, i) for r in "nms" for i in (False, True)}


def test_tables_reach_every_bn_head_path():
    routes = [F.bnhead_route(*c[:5]) for c in F.BN_CASES + [F.BN_OFFSET_CASE]]
    assert all(r[0] for r in routes)
    nblk, rounds = {r[1] for r in routes}, {r[2] for r in routes}
    assert {1, 2, 256} <= nblk and any(2 < n < 256 for n in nblk) and 1 in rounds and any(r >= 2 for r in rounds)
    assert {(c[1], c[2]) for c in F.BN_CASES} >= {(16, 1), (2, 2), (4, 3), (4, 5), (2, 6), (16, 49), (4, 127), (4, 341), (4, 511), (16, 128)}
    # channel boundaries inside one aligned float4: three at HW = 1, one at HW = 2, 3, 5, 6 (at HW >= 2 no four consecutive k hold two)
    assert [F.float4_channel_crossings(C, HW) for C, HW in ((16, 1), (2, 2), (4, 3), (4, 5), (2, 6))] == [3, 1, 1, 1, 1]
    assert {c[0] for c in F.BN_CASES} >= {1, 16, 17, 32, 33, 300, 4096} and {c[3] for c in F.BN_CASES} >= {1, 15, 16}
    assert {c[4] for c in F.BN_CASES} == {1, 16, 31, 32, 33, 256, 257, 1024}
    assert {c[5] for c in F.BN_CASES} == {c[6] for c in F.BN_CASES} == {c[7] for c in F.BN_CASES} == {True, False}
    assert max(c[0] * c[1] * c[2] for c in F.BN_CASES) <= 300 * 784                # nothing larger than the old test's operand
    assert F.bnhead_route(32, 16, 128, 16, 256)[2] == 1 and F.bnhead_route(257, 2, 2, 1, 257)[2] == 2


# ==================================================================================================== pinned to the oracle
def oracle_mlp(X1, H, W2, dO):
    """The O.linear_backward / O.relu_backward chain of test_mlp_chain_backward_one_launch, in the dtype of its arguments."""
    dh, dW2, db2 = O.linear_backward(H, W2, np.zeros((1, W2.shape[0]), W2.dtype), dO)
    dz = O.relu_backward(H, dh)
    _, dW1, db1 = O.linear_backward(X1, np.zeros((H.shape[1], X1.shape[1]), X1.dtype), np.zeros((1, H.shape[1]), X1.dtype), dz)
    return dict(dW2=dW2, db2=db2.reshape(-1), dW1=dW1, db1=db1.reshape(-1))


@pytest.mark.parametrize("shape", [(32, 784, 128, 10), (37, 50, 33, 7), (256, 300, 64, 16), (5, 16, 16, 1)])
def test_mlp_restatement_is_the_oracle_chain(shape):
    d = [a.astype(np.float64) for a in F.mlp_inputs(*shape)]
    ref, want = F.mlp_backward64(*d), oracle_mlp(*d)
    for k in want:
        np.testing.assert_allclose(ref[k], want[k], rtol=1e-12, atol=1e-12, err_msg=k)


def test_mlp_restatement_masks_as_the_reference_does():
    """activations.py:44-45, `grad * (f_x > 0)`: NaN, -0 and +0 in H are closed; a closed mask over an infinite gradient gives NaN."""
    H = np.array([[np.nan, -0.0, 0.0, 1e-38, 2.0, 0.0]], np.float32)
    W2 = np.array([[1, 1, 1, 1, 1, np.inf]], np.float32)
    ref = F.mlp_backward64(np.ones((1, 1), np.float32), H, W2, np.full((1, 1), 3.0, np.float32))
    want = O.relu_backward(H.astype(np.float64), O.linear_backward(H.astype(np.float64), W2.astype(np.float64), None, np.full((1, 1), 3.0))[0])
    np.testing.assert_array_equal(ref["dZ"], want)
    np.testing.assert_array_equal(ref["dZ"][0, :5], [0, 0, 0, 3, 3])
    assert np.isnan(ref["dZ"][0, 5])


@pytest.mark.parametrize("rows,K,classes,red", [(32, 128, 10, "mean"), (200, 784, 10, "sum"), (256, 2048, 32, "none"), (7, 50, 3, "mean")])
def test_linear_ce_restatement_is_the_oracle_chain(rows, K, classes, red):
    X, W, b, cw, _ = F.lince_inputs(rows, K, classes)
    y = np.random.default_rng(rows).integers(0, classes, rows)
    y[::5] = 0                                                                  # the old test's in-range ignore_index
    X, W, b, cw = (a.astype(np.float64) for a in (X, W, b, cw))
    z, _ = F.logits64(X, W, b)
    np.testing.assert_allclose(z, O.linear_forward(X, W, b[None, :]), rtol=1e-12, atol=1e-12)
    for weight in (None, cw):
        loss_rows, _, loss, dl, _ = cross_entropy(z, y, weight, 0, red)
        want_loss, want_grad = O.cross_entropy_forward_backward(z, y, weight, 0, red)
        np.testing.assert_allclose(loss, want_loss, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(dl, want_grad, rtol=1e-12, atol=1e-14)


def oracle_bn_chain(d, dtype):
    """batchnorm2d.py:84-100 -> linear.py:48-58 -> activations.py:19-28 -> losses.py:9-22 through the oracle, in `dtype`."""
    X, T, W = (np.asarray(d[k], dtype) for k in ("X", "T", "W"))
    B, C, HW = X.shape
    opt = lambda a: None if a is None else np.asarray(a, dtype)[None, :]        # noqa: E731
    Y, cache, rm, rv = O.batchnorm2d_forward(X[..., None], opt(d["g"]), opt(d["be"]), np.full((1, C), F.BN_RM0, dtype),
                                               np.full((1, C), F.BN_RV0, dtype), dtype(F.BN_EPS), dtype(F.BN_MOMENTUM), True)
    z = O.linear_forward(Y.reshape(B, -1), W, opt(d["b"]))
    pred = O.sigmoid_forward(z)
    loss, dpred = O.mse_forward_backward(pred, T)
    return dict(Y=Y.reshape(B, C, HW), inv=np.asarray(cache[1]).reshape(-1), z=z, pred=pred, dz=O.sigmoid_backward(pred, dpred), loss=loss,
                rm=np.asarray(rm).reshape(-1), rv=np.asarray(rv).reshape(-1))


@pytest.mark.parametrize("c", [(256, 16, 49, 10, 196, True, True, True), (37, 5, 12, 3, 4, True, True, True), (16, 3, 64, 16, 1024, False, True, True),
                               (2, 2, 2, 1, 1, True, True, True), (300, 16, 4, 7, 25, True, True, True)], ids=F.bn_id)
def test_bn_head_restatement_is_the_oracle_chain(c):
    d = F.bn_inputs(c)
    ref, want = F.bnhead64(d), oracle_bn_chain(d, np.float64)
    for k in want:
        np.testing.assert_allclose(ref[k], want[k], rtol=1e-9, atol=1e-12, err_msg=k)
    # the (mean, M2) pairs the kernel is fed describe the same statistics
    st = d["stats"].astype(np.float64)
    np.testing.assert_allclose(st[:, :, 0].mean(0), ref["mean"], rtol=1e-6, atol=1e-6)


# ==================================================================================================== the float32 oracle inside the bounds
def test_float32_oracle_sits_inside_the_mlp_bounds():
    worst = 0.0
    for shape in F.MLP_CASES + F.MLP_ADAM_SHAPES:
        d = F.mlp_inputs(*shape)
        ref = F.mlp_backward64(*d)
        bound, got = F.mlp_bounds(*d, ref), oracle_mlp(*d)
        worst = max([worst] + [ratio(got[k], ref[k], bound[k]) for k in got])
    print(f"float32 oracle, MLP backward: largest share of a bound {worst:.3f}")
    assert worst < 0.5


def test_float32_oracle_sits_inside_the_linear_ce_bounds():
    worst = dict(logits=0.0, ce=0.0)
    for rows, K, classes, _, _ in F.LINCE_CASES:
        X, W, b, cw, y = F.lince_inputs(rows, K, classes)
        z64, mag = F.logits64(X, W, b)
        z32 = O.linear_forward(X, W, b[None, :])
        assert z32.dtype == np.float32
        worst["logits"] = max(worst["logits"], ratio(z32, z64, dot_bound_of(mag, z64)))
        ign = F.lince_ignore(classes)
        for red, weighted, _ in F.LINCE_RUNS:
            if classes == 1 and red == "m":
                continue                                                        # (every label ignored: 0 / 0 in the oracle's mean)
            live = (y != ign) & (y >= 0) & (y < classes)
            yo = np.where(live, y, ign)                                         # the oracle indexes with every label: inert ones -> ignored
            loss_rows, _, loss, dl, _ = cross_entropy(z32, y, cw if weighted else None, ign, red)
            got_loss, got_grad = O.cross_entropy_forward_backward(z32, yo, cw if weighted else None, ign, {"n": "none", "m": "mean", "s": "sum"}[red])
            worst["ce"] = max(worst["ce"], ratio(got_loss, loss, close_bound(loss, 1e-5, 1e-5)), ratio(got_grad, dl, scaled_bound(dl)))
    print(f"float32 oracle, Linear + CrossEntropy: largest share of a bound: logits {worst['logits']:.3f}, loss / dlogits {worst['ce']:.3f}")
    assert max(worst.values()) < 0.5


def test_float32_oracle_sits_inside_the_bn_head_bounds():
    worst = {}
    for c in F.BN_CASES:
        d = F.bn_inputs(c)
        ref = F.bnhead64(d)
        bound, got = F.bnhead_bounds(d, ref), oracle_bn_chain(d, np.float32)
        for k in got:
            if k != "z":
                worst[k] = max(worst.get(k, 0.0), ratio(got[k], ref[k], bound[k]))
    print("float32 oracle, BatchNorm head: largest share of a bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) < 0.5


def test_offset_channel_allowance():
    """The case whose float32 reference loses digits: what the two-pass float32 BatchNorm is off by, times 4 (the kernel merges (mean, M2)
    pairs in another order, and a Chan merge is not two-pass), stays below 1 % of the rms."""
    dy, rms = F.bn_offset_allowance()
    print(f"offset channel: float32 two-pass |Y - Y64| {dy:.3e} (rms {rms:.3f}); allowed 4 x = {400 * dy / rms:.3f} % of the rms")
    assert 0 < 4 * dy < 0.01 * rms
    d = F.bn_inputs(F.BN_OFFSET_CASE, offset_channel=True)
    assert abs(d["X"][:, 1].mean() - 100) < 0.01 and 0.005 < d["X"][:, 1].std() < 0.02
