"""CPU: the GRU / RNN / Bidirectional layers' contract (parameters, their order, seeded initial values, argument errors, the ctypes
mirrors of the ABI-220 structs) and the float64 restatement the GPU tests use (tests/gru_ref.py), checked against fixtures recorded
from the reference (tools/gen_golden.py: gen_gru, gen_rnn, gen_bidirectional)."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_abi import lib  # noqa: F401 -- the fixture that loads (and if need be builds) the library
from gru_ref import gru_backward, gru_forward, merge_backward, merge_forward, rnn_backward, rnn_forward

GRU_CASES = ["gru_h50_b17", "gru_t1_b1", "gru_2d", "gru_state", "gru_cycled", "gru_relu", "gru_relu_rec"]
RNN_CASES = ["rnn_h50_b17", "rnn_t1_b1", "rnn_relu", "rnn_cycled"]
BI_CASES = ["bi_gru_sum", "bi_gru_concat", "bi_gru_mul", "bi_gru_avg", "bi_gru_last", "bi_rnn_sum", "bi_gru_both"]
GRU_NAMES = ["weight_z", "weight_r", "weight_h", "weight_hz", "weight_hr", "weight_hh", "bias_z", "bias_r", "bias_h"]
RNN_NAMES = ["weight", "weight_h", "bias"]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "neunet_hip.h")


def parse_rs(v):
    return {"True": True, "False": False}.get(str(v), str(v))


def wants_last(rs, k, n_outs):
    """Is output k of a layer with this return_sequences the last state (else the whole sequence)?"""
    return k == 1 if n_outs == 2 else rs in ("last", False)


def run_ref(kind, X, params, h0, nl, rnl, dtype, reverse=False):
    if kind == "gru":
        return gru_forward(X, params, h0, nl, rnl, dtype=dtype, reverse=reverse)
    return rnn_forward(X, params, h0, nl, dtype=dtype, reverse=reverse)


def back_ref(kind, cache, dY_all=None, dY_last=None):
    return (gru_backward if kind == "gru" else rnn_backward)(cache, dY_all, dY_last)


def replay_layer(f, kind, dtype=np.float64):
    """A single-layer fixture through the restatement: ({key: output}, dX per call, the parameter gradients)."""
    B, T, n_in, H, calls = (int(v) for v in f["cfg"])
    nl, rnl, rs = str(f["modes"][0]), str(f["modes"][1]), parse_rs(f["modes"][2])
    n = 9 if kind == "gru" else 3
    params = [f[f"p{i}"] for i in range(n)]
    h0 = f.get("h0")
    outs, dXs, grads = {}, [], [np.zeros(np.shape(a)) for a in params]
    for c in range(calls):
        X = f[f"X{c}"]
        X3 = X[None] if B < 0 else X
        Y, cache = run_ref(kind, X3, params, h0, nl, rnl, dtype)
        keys = sorted(k for k in f if k.startswith(f"Y{c}_"))
        dX = np.zeros(X3.shape)
        for k in keys:
            idx = int(k.split("_")[1])
            dY = f[f"dY{c}_{idx}"]
            if wants_last(rs, idx, len(keys)):
                outs[k] = Y[:, -1:]
                dx, g = back_ref(kind, cache, dY_last=dY.reshape(dY.shape[0], -1))
            else:
                outs[k] = Y
                dx, g = back_ref(kind, cache, dY_all=dY)
            dX += dx
            grads = [a + b for a, b in zip(grads, g)]
        dXs.append(dX.reshape(X.shape))
        if calls > 1:                                            # cycled_states: the next call starts from the last state
            h0 = cache["hs"][-1]
    return outs, dXs, grads


def replay_bidirectional(f, dtype=np.float64):
    """A Bidirectional fixture: the direct layer on X, the reverse layer on X read backwards (outputs in step order), merged."""
    kind, merge, rs = str(f["modes"][0]).lower(), str(f["modes"][1]), parse_rs(f["modes"][2])
    n = 9 if kind == "gru" else 3
    pd, pr = [f[f"p{i}"] for i in range(n)], [f[f"p{n + i}"] for i in range(n)]
    X = f["X0"]
    YD, cD = run_ref(kind, X, pd, None, "tanh", "sigmoid", dtype)
    YR, cR = run_ref(kind, X, pr, None, "tanh", "sigmoid", dtype, reverse=True)
    keys = sorted(k for k in f if k.startswith("Y0_"))
    outs, dX, grads = {}, np.zeros(X.shape), [np.zeros(np.shape(a)) for a in pd + pr]
    for k in keys:
        idx = int(k.split("_")[1])
        last = wants_last(rs, idx, len(keys))
        D, R = (YD[:, -1:], YR[:, -1:]) if last else (YD, YR)
        outs[k] = merge_forward(D, R, merge)
        if f"dY0_{idx}" not in f:
            continue
        dD, dR = merge_backward(f[f"dY0_{idx}"].astype(dtype), D, R, merge)
        if last:
            (dxd, gd), (dxr, gr) = back_ref(kind, cD, dY_last=dD[:, 0]), back_ref(kind, cR, dY_last=dR[:, 0])
        else:
            (dxd, gd), (dxr, gr) = back_ref(kind, cD, dY_all=dD), back_ref(kind, cR, dY_all=dR)
        dX += dxd + dxr
        grads = [a + b for a, b in zip(grads, gd + gr)]
    return outs, dX, grads


def check_against_fixture(f, outs, dXs, grads, names):
    for k, v in outs.items():
        np.testing.assert_allclose(v, f[k], rtol=1e-5, atol=1e-6, err_msg=k)
    for c, dX in enumerate(dXs):
        np.testing.assert_allclose(dX, f[f"dX{c}"], rtol=1e-4, atol=1e-6, err_msg=f"dX{c}")
    for i, g in enumerate(grads):
        np.testing.assert_allclose(g.reshape(f[f"g{i}"].shape), f[f"g{i}"], rtol=1e-4, atol=1e-5, err_msg=names[i % len(names)])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", GRU_CASES + RNN_CASES)
def test_restatement_matches_reference_fixture(golden, name, dtype):
    f = golden(name)
    kind = name[:3]
    outs, dXs, grads = replay_layer(f, kind, dtype)
    assert all(v.dtype == dtype for v in outs.values())
    check_against_fixture(f, outs, dXs, grads, GRU_NAMES if kind == "gru" else RNN_NAMES)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", BI_CASES)
def test_bidirectional_restatement_matches_reference_fixture(golden, name, dtype):
    f = golden(name)
    outs, dX, grads = replay_bidirectional(f, dtype)
    assert len(outs) == (2 if name == "bi_gru_both" else 1)
    if name == "bi_gru_both":                                    # forward only: the reference's backward raises
        assert "dX0" not in f
        for k, v in outs.items():
            np.testing.assert_allclose(v, f[k], rtol=1e-5, atol=1e-6, err_msg=k)
        return
    check_against_fixture(f, outs, [dX], grads, GRU_NAMES if "gru" in name else RNN_NAMES)


def test_float32_mode_is_float32_throughout(golden):
    f = golden("gru_h50_b17")
    params = [f[f"p{i}"] for i in range(9)]
    Y32, cache = gru_forward(f["X0"], params, dtype=np.float32)
    dX32, g32 = gru_backward(cache, dY_all=np.ones(Y32.shape, np.float32), dY_last=np.ones(Y32[:, 0].shape, np.float32))
    for a in [Y32, dX32, *g32, *cache["hs"], *cache["z"], *cache["r"], *cache["c"], *(u for us in cache["pre"] for u in us)]:
        assert a.dtype == np.float32
    Y64, _ = gru_forward(f["X0"], params)
    assert Y64.dtype == np.float64 and np.any(Y64 != Y32) and np.abs(Y64 - Y32).max() < 1e-5
    R32, cache = rnn_forward(f["X0"], [params[0], params[3], params[6]], dtype=np.float32)
    dR32, gr32 = rnn_backward(cache, dY_all=np.ones(R32.shape, np.float32))
    for a in [R32, dR32, *gr32, *cache["hs"], *cache["pre"]]:
        assert a.dtype == np.float32
    # a None bias is a zero bias
    Yz, _ = gru_forward(f["X0"], params[:6] + [None, params[7], None])
    Yz2, _ = gru_forward(f["X0"], params[:6] + [np.zeros(50), params[7], np.zeros(50)])
    np.testing.assert_array_equal(Yz, Yz2)


def test_reverse_flag_is_the_layer_on_the_flipped_input(golden):
    f = golden("gru_h50_b17")
    params = [f[f"p{i}"] for i in range(9)]
    X, dY = f["X0"], f["dY0_0"]
    Yr, cr = gru_forward(X, params, reverse=True)
    Yf, cf = gru_forward(X[:, ::-1], params)
    np.testing.assert_array_equal(Yr, Yf)
    dXr, gr = gru_backward(cr, dY_all=dY)
    dXf, gf = gru_backward(cf, dY_all=dY)
    np.testing.assert_array_equal(dXr, dXf[:, ::-1])
    for a, b in zip(gr, gf):
        np.testing.assert_array_equal(a, b)


def param_names(m):
    return [k for k, v in m.__dict__.items() if v.__class__.__name__ == "Parameter"]


def test_gru_parameters_match_reference(golden):
    """nn.GRU draws its weights from the global np.random in the reference's order and dtype: with the fixture's seed it starts from
    exactly the reference's initial weights (biases are zeros; the fixture randomised them afterwards)."""
    import neunet_hip.nn as nn
    f = golden("gru_h50_b17")
    np.random.seed(120)                                          # tools/gen_golden.py: gen_gru's seed_layers(120)
    m = nn.GRU(10, 50, device="cpu")
    ps = m.parameters()
    assert param_names(m) == GRU_NAMES and list(m.state_dict()) == GRU_NAMES and len(ps) == 9
    for i, p in enumerate(ps):
        assert p.data.dtype == np.float32
        if i < 6:
            np.testing.assert_array_equal(p.data, f[f"p{i}"], err_msg=GRU_NAMES[i])
        else:
            assert p.data.shape == (50,) and not np.any(p.data)


def test_rnn_parameters_match_reference(golden):
    import neunet_hip.nn as nn
    f = golden("rnn_h50_b17")
    np.random.seed(121)                                          # gen_rnn's seed_layers(121)
    m = nn.RNN(10, 50, device="cpu")
    ps = m.parameters()
    assert param_names(m) == RNN_NAMES and list(m.state_dict()) == RNN_NAMES and len(ps) == 3
    np.testing.assert_array_equal(ps[0].data, f["p0"])
    np.testing.assert_array_equal(ps[1].data, f["p1"])
    assert ps[2].data.shape == (50,) and not np.any(ps[2].data) and all(p.data.dtype == np.float32 for p in ps)


def test_bidirectional_parameters(golden):
    """The reverse layer owns distinct Parameter objects with the direct layer's initial values, nothing more is drawn from the
    generator, parameters() is direct then reverse, and the state_dict keys carry direct_layer / reverse_layer."""
    import neunet_hip.nn as nn
    f = golden("bi_gru_sum")
    np.random.seed(122)                                          # gen_bidirectional's seed_layers(122): bi_gru_sum is its first case
    m = nn.Bidirectional(nn.GRU(7, 20, return_sequences="all", device="cpu"), merge_mode="sum", device="cpu")
    after = np.random.uniform()
    np.random.seed(122)
    nn.GRU(7, 20, device="cpu")
    assert np.random.uniform() == after, "Bidirectional drew from the global generator"
    ps = m.parameters()
    assert len(ps) == 18 and len({id(p) for p in ps}) == 18
    assert ps[:9] == m.direct_layer.parameters() and ps[9:] == m.reverse_layer.parameters()
    for i in range(9):
        assert ps[i] is not ps[9 + i] and ps[i].data is not ps[9 + i].data
        np.testing.assert_array_equal(ps[i].data, ps[9 + i].data)
        if i < 6:
            np.testing.assert_array_equal(ps[i].data, f[f"p{i}"], err_msg=GRU_NAMES[i])
    assert list(m.state_dict()) == ["direct_layer." + n for n in GRU_NAMES] + ["reverse_layer." + n for n in GRU_NAMES]
    assert m.return_sequences == "all" and m.merge_mode == "sum"
    assert nn.Bidirectional(nn.RNN(4, 8, device="cpu"), device="cpu").merge_mode == "sum"       # the default


def test_seqcls_initial_parameters_match_reference(golden):
    """The notebook's model, built in the reference's order with the fixture's seed, starts from the reference's initial values."""
    import neunet_hip.nn as nn
    f = {**golden("seqcls_step_0"), **golden("seqcls_step_1")}
    np.random.seed(123)
    model = nn.Sequential(nn.Embedding(40, 10, device="cpu"),
                          nn.Bidirectional(nn.GRU(10, 50, return_sequences=True, device="cpu"), merge_mode="sum", device="cpu"),
                          nn.Bidirectional(nn.RNN(50, 50, return_sequences=True, bias=True, device="cpu"), device="cpu"),
                          nn.Bidirectional(nn.GRU(50, 50, return_sequences=False, device="cpu"), device="cpu"),
                          nn.Linear(50, 1, device="cpu"), nn.Sigmoid())
    ps = model.parameters()
    assert len(ps) == int(f["n_params"]) == 45
    for i, p in enumerate(ps):
        np.testing.assert_array_equal(np.asarray(p.data), f[f"p{i}"], err_msg=str(i))


def test_argument_errors():
    import neunet_hip.nn as nn
    with pytest.raises(ValueError, match=r"gru.py:274-280"):
        nn.GRU(4, 8, bias=False, device="cpu")
    with pytest.raises(ValueError, match=r"rnn.py:152-158"):
        nn.RNN(4, 8, bias=False, device="cpu")
    for bad in (dict(nonlinearity="gelu"), dict(recurrent_nonlinearity="softsign")):
        with pytest.raises(ValueError, match="nonlinearity"):
            nn.GRU(4, 8, device="cpu", **bad)
    with pytest.raises(ValueError, match="nonlinearity"):
        nn.RNN(4, 8, nonlinearity="gelu", device="cpu")
    for cls in (nn.GRU, nn.RNN):
        with pytest.raises(ValueError, match="return_sequences"):
            cls(4, 8, return_sequences="first", device="cpu")
        with pytest.raises(ValueError, match="512"):
            cls(4, 513, device="cpu")
        for rs in ("both", "all", "last", True, False):
            assert cls(4, 8, return_sequences=rs, device="cpu").return_sequences is rs
    with pytest.raises(NotImplementedError, match="reverse mode"):
        nn.Bidirectional(nn.LSTM(4, 8, device="cpu"), device="cpu")
    with pytest.raises(ValueError, match="LSTM, GRU or RNN"):
        nn.Bidirectional(nn.Linear(4, 8, device="cpu"), device="cpu")
    with pytest.raises(ValueError, match="merge_mode"):
        nn.Bidirectional(nn.GRU(4, 8, device="cpu"), merge_mode="max", device="cpu")
    with pytest.raises(TypeError, match="tensor"):
        nn.GRU(4, 8, device="cpu")(np.zeros((2, 3, 4), np.float32))


def header_struct(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    assert m, f"struct {name} not found in include/neunet_hip.h"
    fields = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        g = re.fullmatch(r"(?:const\s+)?float\s*\*\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?", decl)
        assert g, f"struct {name}: member {decl!r} is not a float pointer (array)"
        fields.append((g.group(1), int(g.group(2) or 0)))
    return fields


@pytest.mark.parametrize("cname,pyname,order,length,args", [
    ("nnhipGRUWeights", "GRUWeights", ["wx", "wh", "b"], 3, [("nnhipGRUForward", 1), ("nnhipGRUBackward", 1)]),
    ("nnhipGRUGrads", "GRUGrads", ["dwx", "dwh", "db"], 3, [("nnhipGRUBackward", 7)]),
    ("nnhipRNNWeights", "RNNWeights", ["wx", "wh", "b"], 0, [("nnhipRNNForward", 1), ("nnhipRNNBackward", 1)]),
    ("nnhipRNNGrads", "RNNGrads", ["dwx", "dwh", "db"], 0, [("nnhipRNNBackward", 7)])])
def test_structs_match_header(cname, pyname, order, length, args):
    """The ctypes mirrors have the header's members in the header's order, pointers (or arrays of three) without padding, and the
    signature table passes them where the header does."""
    from neunet_hip import _lib
    cls = getattr(_lib, pyname)
    assert header_struct(cname) == [(n, length) for n in order]
    assert [n for n, _ in cls._fields_] == order
    psz, k = ctypes.sizeof(ctypes.c_void_p), max(length, 1)
    for idx, (n, t) in enumerate(cls._fields_):
        if length:
            assert t._type_ is ctypes.c_void_p and t._length_ == length, n
        else:
            assert t is ctypes.c_void_p, n
        assert getattr(cls, n).offset == idx * k * psz and getattr(cls, n).size == k * psz, n
    assert ctypes.sizeof(cls) == 3 * k * psz
    for fn, pos in args:
        assert _lib._SIGNATURES[fn][1][pos] is ctypes.POINTER(cls), (fn, pos)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for fn, pos in args:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % fn, text, flags=re.S).group(1).split(",")
        assert cname in decl[pos], (fn, pos, decl[pos])
    assert [int(re.search(r"#define\s+NNHIP_MERGE_%s\s+(\d+)" % m.upper(), text).group(1)) for m in ("concat", "sum", "mul", "avg")] == \
        [0, 1, 2, 3]


def test_version_is_220(lib):
    from neunet_hip import _lib
    assert _lib.load_hip_function("nnhipVersion")() >= 220
