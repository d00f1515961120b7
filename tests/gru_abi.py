"""Helpers of tests/test_gru_tiers_gpu.py: seeded GRU / RNN inputs for one or two directions, one call of nnhipGRUForward /
nnhipGRUBackward (or the RNN pair) through the C ABI with every output buffer pre-filled with NaN and fenced by NaN guard words, and
the float64 / float32 restatement (tests/gru_ref.py) laid out like the C ABI's outputs."""
import numpy as np

from gru_ref import gru_backward, gru_forward, rnn_backward, rnn_forward
from lstm_abi import NL, Fenced, dev, padded

NW = {"gru": 9, "rnn": 3}                                   # parameters per direction, reference order
FORWARD_OUT = {"gru": ("Y", "gates", "hprev", "hT"), "rnn": ("Y", "hprev", "hT")}


def grad_names(kind, ndir):
    base = ("dwz", "dwr", "dwh", "dwhz", "dwhr", "dwhh", "dbz", "dbr", "dbh") if kind == "gru" else ("dw", "dwh", "db")
    return [f"{n}[{d}]" for d in range(ndir) for n in base]


def make_inputs(kind, seed, B, T, n_in, H, ndir=1, state=False, wide=3.0):
    """Per direction: weights U(-wide / sqrt(H), wide / sqrt(H)) (three times the layer's own initial range, so that the recurrent term
    is of order 1 and a wrong recurrence moves the outputs by about their rms), biases U(-0.3, 0.3); data and gradients U(-1, 1)."""
    rng = np.random.default_rng(seed)
    s = wide / np.sqrt(H)
    ng = NW[kind] // 3
    params = [[rng.uniform(-s, s, (n_in, H)) for _ in range(ng)] + [rng.uniform(-s, s, (H, H)) for _ in range(ng)] +
              [rng.uniform(-0.3, 0.3, H) for _ in range(ng)] for _ in range(ndir)]
    d = dict(params=[[a.astype(np.float32) for a in p] for p in params],
             X=rng.uniform(-1, 1, (B, T, n_in)).astype(np.float32),
             dY=rng.uniform(-1, 1, (ndir, B, T, H)).astype(np.float32),
             dYl=rng.uniform(-1, 1, (ndir, B, H)).astype(np.float32))
    if state:
        d["h0"] = rng.uniform(-1, 1, (ndir, B, H)).astype(np.float32)
    return d


def structs(kind, pd, grad_ptrs=None):
    """The ctypes weight (and gradient) struct arrays for per-direction lists of device tensors (None: a NULL member)."""
    from neunet_hip._lib import GRUGrads, GRUWeights, RNNGrads, RNNWeights
    W, G = (GRUWeights, GRUGrads) if kind == "gru" else (RNNWeights, RNNGrads)
    ndir = len(pd)
    w = (W * ndir)()
    g = (G * ndir)() if grad_ptrs is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    for d in range(ndir):
        if kind == "gru":
            for k in range(3):
                w[d].wx[k], w[d].wh[k], w[d].b[k] = ptr(pd[d][k]), ptr(pd[d][3 + k]), ptr(pd[d][6 + k])
                if g is not None:
                    g[d].dwx[k], g[d].dwh[k], g[d].db[k] = grad_ptrs[d][k], grad_ptrs[d][3 + k], grad_ptrs[d][6 + k]
        else:
            w[d].wx, w[d].wh, w[d].b = ptr(pd[d][0]), ptr(pd[d][1]), ptr(pd[d][2])
            if g is not None:
                g[d].dwx, g[d].dwh, g[d].db = grad_ptrs[d]
    return w, g


def run_abi(kind, X, params, dY=None, dYl=None, h0=None, nl="tanh", rnl="sigmoid", want_hT=True, alias_state=False, want_dX=True,
            grads="all", backward=True):
    """One forward (+ one backward) through the C ABI.  params: one list per direction (a None bias: b = NULL).  alias_state: hT = h0
    (the cycled contract).  grads: "all", None (grads = NULL) or a set of (direction, index) pairs to pass.  Returns {name: array}: Y
    [ndir, B, T, H], gates (GRU) [ndir, B, T, 3Hp], hprev, hT, dX, grads (one array per direction and parameter, NaN where not passed)."""
    import torch
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    ndir, n = len(params), NW[kind]
    B, T, n_in = X.shape
    H = params[0][n // 3].shape[0]
    Hp = padded(H)
    st = get_current_stream_ptr()
    x = dev(X)
    pd = [[None if a is None else dev(a) for a in p] for p in params]
    w, _ = structs(kind, pd)
    h0d = None if h0 is None else dev(h0)
    f = dict(Y=Fenced(ndir, B, T, H), hprev=Fenced(ndir, B, T, H), hT=Fenced(ndir, B, H) if want_hT and not alias_state else None)
    if kind == "gru":
        f["gates"] = Fenced(ndir, B, T, 3 * Hp)
    hTd = h0d if alias_state else (f["hT"] and f["hT"].view)
    if kind == "gru":
        call_hip_function("nnhipGRUForward", x, w, h0d, f["Y"].view, f["gates"].view, f["hprev"].view, hTd, B, T, n_in, H, NL[nl], NL[rnl],
                          ndir, st)
    else:
        call_hip_function("nnhipRNNForward", x, w, h0d, f["Y"].view, f["hprev"].view, hTd, B, T, n_in, H, NL[nl], ndir, st)
    torch.cuda.synchronize()
    out = {k: (None if v is None else v.host()) for k, v in f.items()}
    if alias_state:
        out["hT"] = h0d.cpu().numpy()
    fences = [v for v in f.values() if v is not None]
    if backward:
        fdX = Fenced(B, T, n_in)
        fg = [[Fenced(*np.shape(params[d][i] if params[d][i] is not None else np.zeros(H))) for i in range(n)] for d in range(ndir)]
        g = None
        if grads is not None:
            ptrs = [[fg[d][i].view.data_ptr() if grads == "all" or (d, i) in grads else None for i in range(n)] for d in range(ndir)]
            _, g = structs(kind, pd, ptrs)
        dYd, dYld = None if dY is None else dev(dY), None if dYl is None else dev(dYl)
        if kind == "gru":
            call_hip_function("nnhipGRUBackward", x, w, f["gates"].view, f["hprev"].view, dYd, dYld, fdX.view if want_dX else None, g, B, T,
                              n_in, H, NL[nl], NL[rnl], ndir, st)
        else:
            call_hip_function("nnhipRNNBackward", x, w, f["Y"].view, f["hprev"].view, dYd, dYld, fdX.view if want_dX else None, g, B, T,
                              n_in, H, NL[nl], ndir, st)
        torch.cuda.synchronize()
        out["dX"] = fdX.host()
        out["grads"] = [b.host() for per in fg for b in per]
        fences += [fdX] + [b for per in fg for b in per]
        for k in FORWARD_OUT[kind][:-1]:                         # the backward must not touch what the forward saved
            np.testing.assert_array_equal(f[k].host(), out[k], err_msg=f"{k} changed by the backward")
    for v in fences:
        assert v.guards_intact(), "a kernel wrote outside an output buffer"
    call_hip_function("nnhipDeviceError")                        # raises if a kernel raised the device error word
    return out


def reference_in(dtype, kind, X, params, dY=None, dYl=None, h0=None, nl="tanh", rnl="sigmoid"):
    """The restatement laid out like the C ABI's outputs: a leading direction axis; Y in step order; gates (ndir, B, T, 3, H) and
    hprev in INPUT-time order; dX the sum over the directions; grads flat (direction-major)."""
    ndir = len(params)
    Ys, gates, hprevs, hTs, grads = [], [], [], [], []
    dX = None
    for d in range(ndir):
        h0d = None if h0 is None else h0[d]
        if kind == "gru":
            Y, cache = gru_forward(X, params[d], h0d, nl, rnl, dtype=dtype, reverse=d == 1)
            g = np.stack([np.stack([cache["z"][t], cache["r"][t], cache["c"][t]], 1) for t in range(len(cache["z"]))], 1)
            gates.append(g[:, ::-1] if d else g)
        else:
            Y, cache = rnn_forward(X, params[d], h0d, nl, dtype=dtype, reverse=d == 1)
        hp = np.stack(cache["hs"][:-1], 1)
        Ys.append(Y)
        hprevs.append(hp[:, ::-1] if d else hp)
        hTs.append(cache["hs"][-1])
        if dY is not None or dYl is not None:
            bw = gru_backward if kind == "gru" else rnn_backward
            dx, g = bw(cache, None if dY is None else dY[d], None if dYl is None else dYl[d])
            dX = dx if dX is None else dX + dx
            grads += g
    ref = dict(Y=np.stack(Ys), hprev=np.stack(hprevs), hT=np.stack(hTs))
    if kind == "gru":
        ref["gates"] = np.stack(gates)
    if dX is not None:
        ref["dX"], ref["grads"] = dX, grads
    return ref


def reference(*args, **kw):
    """The float64 restatement with the float32 restatement of the same inputs under "f32" (what the reference's own rounding does)."""
    ref = reference_in(np.float64, *args, **kw)
    ref["f32"] = reference_in(np.float32, *args, **kw)
    return ref
