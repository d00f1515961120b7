"""CPU: the LSTM layer's contract (parameters, seeded initial values, argument errors) and the float64 restatement the GPU tests
use (tests/lstm_ref.py), both checked against fixtures recorded from the reference (tools/gen_golden.py: gen_lstm)."""
import numpy as np
import pytest

from lstm_ref import lstm_backward, lstm_forward

CASES = ["lstm_h50_b17", "lstm_t28", "lstm_t1_b1", "lstm_2d", "lstm_state", "lstm_cycled", "lstm_relu", "lstm_relu_rec"]
NAMES = ["weight_f", "weight_i", "weight_o", "weight_c", "weight_hf", "weight_hi", "weight_ho", "weight_hc",
         "bias_f", "bias_i", "bias_o", "bias_c"]


def replay_reference(f, dtype=np.float64):
    """Run a fixture case through the restatement (float64, or the reference's own float32): returns ({key: output}, dX per call,
    the twelve gradients)."""
    B, T, n_in, H, calls = (int(v) for v in f["cfg"])
    nl, rnl = str(f["modes"][0]), str(f["modes"][1])
    params = [f[f"p{i}"] for i in range(12)]
    h0, c0 = f.get("h0"), f.get("c0")
    outs, dXs, grads = {}, [], [np.zeros(np.shape(a)) for a in params]
    for c in range(calls):
        X = f[f"X{c}"]
        X3 = X[None] if B < 0 else X
        Y, cache = lstm_forward(X3, params, h0, c0, nl, rnl, dtype=dtype)
        keys = sorted(k for k in f if k.startswith(f"Y{c}_"))
        dX = np.zeros(X3.shape)
        for k in keys:
            idx = k.split("_")[1]
            dY = f[f"dY{c}_{idx}"]
            if f[k].shape[1] == 1 and (len(keys) == 2 and idx == "1" or f["modes"][2] in ("last", "False")):
                outs[k] = Y[:, -1:]
                dx, g = lstm_backward(cache, dY_last=dY.reshape(dY.shape[0], -1))
            else:
                outs[k] = Y
                dx, g = lstm_backward(cache, dY_all=dY)
            dX += dx
            grads = [a + b for a, b in zip(grads, g)]
        dXs.append(dX.reshape(X.shape))
        if calls > 1:                                            # cycled_states: the next call starts from the last state
            h0, c0 = cache["hs"][-1], cache["cs"][-1]
    return outs, dXs, grads


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_fixture(golden, name):
    f = golden(name)
    outs, dXs, grads = replay_reference(f)
    for k, v in outs.items():
        np.testing.assert_allclose(v, f[k], rtol=1e-5, atol=1e-6, err_msg=k)
    for c, dX in enumerate(dXs):
        np.testing.assert_allclose(dX, f[f"dX{c}"], rtol=1e-4, atol=1e-6, err_msg=f"dX{c}")
    for i, g in enumerate(grads):
        np.testing.assert_allclose(g.reshape(f[f"g{i}"].shape), f[f"g{i}"], rtol=1e-4, atol=1e-5, err_msg=NAMES[i])


def test_float32_mode_matches_reference_fixture(golden):
    """lstm_ref's dtype=np.float32 mode is the reference's own arithmetic (float32 arrays, float32 exp / tanh): it reproduces the
    recorded T = 28 case to the tolerances above, every array it touches is float32, and it differs from the float64 mode -- so the
    "share of the bound the reference alone uses" figures of tests/test_lstm_tiers_gpu.py are pinned to the reference, not to our
    reading of it."""
    f = golden("lstm_t28")
    outs, dXs, grads = replay_reference(f, dtype=np.float32)
    for k, v in outs.items():
        assert v.dtype == np.float32
        np.testing.assert_allclose(v, f[k], rtol=1e-5, atol=1e-6, err_msg=k)
    for c, dX in enumerate(dXs):
        np.testing.assert_allclose(dX, f[f"dX{c}"], rtol=1e-4, atol=1e-6, err_msg=f"dX{c}")
    for i, g in enumerate(grads):
        np.testing.assert_allclose(g.reshape(f[f"g{i}"].shape), f[f"g{i}"], rtol=1e-4, atol=1e-5, err_msg=NAMES[i])
    B, T, n_in, H, _ = (int(v) for v in f["cfg"])
    params = [f[f"p{i}"] for i in range(12)]
    Y32, cache = lstm_forward(f["X0"], params, dtype=np.float32)
    dX32, g32 = lstm_backward(cache, dY_all=np.ones((B, T, H), np.float32))
    for a in [Y32, dX32, *g32, *cache["hs"], *cache["cs"], *(z for zs in cache["z"] for z in zs)]:
        assert a.dtype == np.float32
    Y64, _ = lstm_forward(f["X0"], params)
    assert Y64.dtype == np.float64 and np.any(Y64 != Y32) and np.abs(Y64 - Y32).max() < 1e-5
    # a None bias is a zero bias
    Yz, _ = lstm_forward(f["X0"], params[:8] + [None, params[9], None, None])
    Yz2, _ = lstm_forward(f["X0"], params[:8] + [np.zeros(H), params[9], np.zeros(H), np.zeros(H)])
    np.testing.assert_array_equal(Yz, Yz2)


def test_lstm_parameters_match_reference(golden):
    """neunet_hip.nn.LSTM draws its weights from the global np.random in the reference's order and dtype: with the fixture's seed
    it starts from exactly the reference's initial weights (biases are zeros; the fixture randomised them afterwards)."""
    import neunet_hip.nn as nn
    f = golden("lstm_h50_b17")
    np.random.seed(112)                                          # tools/gen_golden.py: gen_lstm's seed_layers(112)
    m = nn.LSTM(10, 50, device="cpu")
    ps = m.parameters()
    assert [n for n in NAMES] == [k for k, v in m.__dict__.items() if v.__class__.__name__ == "Parameter"]
    assert len(ps) == 12
    for i, p in enumerate(ps):
        assert p.data.dtype == np.float32
        if i < 8:
            np.testing.assert_array_equal(p.data, f[f"p{i}"], err_msg=NAMES[i])
        else:
            assert p.data.shape == (50,) and not np.any(p.data)
    assert list(m.state_dict()) == NAMES


def test_lstm_argument_errors():
    import neunet_hip.nn as nn
    with pytest.raises(ValueError, match="lstm.py:318"):
        nn.LSTM(4, 8, bias=False, device="cpu")
    with pytest.raises(ValueError, match="nonlinearity"):
        nn.LSTM(4, 8, nonlinearity="gelu", device="cpu")
    with pytest.raises(ValueError, match="nonlinearity"):
        nn.LSTM(4, 8, recurrent_nonlinearity="softsign", device="cpu")
    with pytest.raises(ValueError, match="return_sequences"):
        nn.LSTM(4, 8, return_sequences="first", device="cpu")
