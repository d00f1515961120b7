"""Helpers of tests/test_lstm_tiers_gpu.py: seeded LSTM inputs, one call of nnhipLSTMForward / nnhipLSTMBackward through the C ABI
with every output buffer pre-filled with NaN and fenced by NaN guard words, and the same configuration through nn.LSTM.

Run as a script it is the fresh-process twin the environment-variable test needs (the library reads NNHIP_LSTM_RESIDENT once per
process):   python tests/lstm_abi.py OUT.npz SEED B T IN H   runs forward + backward through the C ABI and saves every output."""
import ctypes
import os
import sys

import numpy as np

NL = {"tanh": 0, "sigmoid": 1, "relu": 2}                   # include/neunet_hip.h: NNHIP_LSTM_TANH / _SIGMOID / _RELU
GUARD = 64                                                   # floats of NaN before and after every output buffer
FORWARD_OUT = ("Y", "gates", "cell", "hprev", "hT", "cT")
GRADS = ("dwx0", "dwx1", "dwx2", "dwx3", "dwh0", "dwh1", "dwh2", "dwh3", "db0", "db1", "db2", "db3")
ALL = tuple(range(12))


def make_inputs(seed, B, T, n_in, H, state=False, wide=3.0):
    """Weights U(-wide / sqrt(H), wide / sqrt(H)) (three times the layer's own initial range, so that the recurrent term h W_h is of
    order 1 and a wrong recurrence moves the outputs by about their rms), biases U(-0.3, 0.3), data and gradients U(-1, 1)."""
    rng = np.random.default_rng(seed)
    s = wide / np.sqrt(H)
    params = [rng.uniform(-s, s, (n_in, H)) for _ in range(4)] + [rng.uniform(-s, s, (H, H)) for _ in range(4)] + \
             [rng.uniform(-0.3, 0.3, H) for _ in range(4)]
    d = dict(params=[a.astype(np.float32) for a in params],
             X=rng.uniform(-1, 1, (B, T, n_in)).astype(np.float32),
             dY=rng.uniform(-1, 1, (B, T, H)).astype(np.float32),
             dYl=rng.uniform(-1, 1, (B, H)).astype(np.float32))
    if state:
        d["h0"] = rng.uniform(-1, 1, (B, H)).astype(np.float32)
        d["c0"] = rng.uniform(-1, 1, (B, H)).astype(np.float32)
    return d


class Fenced:
    """A NaN-filled device buffer of `shape` with GUARD NaN floats on either side."""

    def __init__(self, *shape):
        import torch
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.view = self.whole[GUARD:GUARD + n].view(*shape)

    def host(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        import torch
        return bool(torch.isnan(self.whole[:GUARD]).all()) and bool(torch.isnan(self.whole[-GUARD:]).all())

    def untouched(self):
        import torch
        return bool(torch.isnan(self.whole).all())


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def padded(H):
    return (H + 15) // 16 * 16


def run_abi(X, params, dY=None, dYl=None, h0=None, c0=None, nl="tanh", rnl="sigmoid", want_hT=True, want_cT=True, alias_state=False,
            want_dX=True, grads=ALL, backward=True, raw=None):
    """One forward (+ one backward) through the C ABI.  params[8 + g] None: b[g] = NULL.  alias_state: hT = h0 and cT = c0 (the cycled
    contract; both given).  grads: indices (reference parameter order) of the nnhipLSTMGrads members to set, or None for grads =
    NULL.  Returns {name: array or None}: the forward outputs, dX, grads (twelve arrays, all-NaN where not requested)."""
    import torch
    from neunet_hip._lib import LSTMGrads, LSTMWeights, call_hip_function, get_current_stream_ptr
    B, T, n_in = X.shape
    H = params[4].shape[0]
    Hp = padded(H)
    st = get_current_stream_ptr()
    x = dev(X)
    pd = [None if a is None else dev(a) for a in params]
    w = LSTMWeights()
    for g in range(4):
        w.wx[g] = pd[g].data_ptr()
        w.wh[g] = pd[4 + g].data_ptr()
        w.b[g] = None if pd[8 + g] is None else pd[8 + g].data_ptr()
    h0d = None if h0 is None else dev(h0)
    c0d = None if c0 is None else dev(c0)
    f = dict(Y=Fenced(B, T, H), gates=Fenced(B, T, 4 * Hp), cell=Fenced(B, T + 1, H), hprev=Fenced(B, T, H),
             hT=Fenced(B, H) if want_hT and not alias_state else None, cT=Fenced(B, H) if want_cT and not alias_state else None)
    hTd, cTd = (h0d, c0d) if alias_state else (f["hT"] and f["hT"].view, f["cT"] and f["cT"].view)
    call_hip_function("nnhipLSTMForward", x, ctypes.byref(w), h0d, c0d, f["Y"].view, f["gates"].view, f["cell"].view, f["hprev"].view,
                      hTd, cTd, B, T, n_in, H, NL[nl], NL[rnl], st)
    torch.cuda.synchronize()
    out = {k: (None if v is None else v.host()) for k, v in f.items()}
    if alias_state:
        out["hT"], out["cT"] = h0d.cpu().numpy(), c0d.cpu().numpy()
    fences = [v for v in f.values() if v is not None]
    if backward:
        fdX = Fenced(B, T, n_in)
        fg = [Fenced(*np.shape(params[i] if params[i] is not None else np.zeros(H))) for i in range(12)]
        g = None
        if grads is not None:
            g = LSTMGrads()
            for i in grads:
                (g.dwx, g.dwh, g.db)[i // 4][i % 4] = fg[i].view.data_ptr()
        call_hip_function("nnhipLSTMBackward", x, ctypes.byref(w), f["gates"].view, f["cell"].view, f["hprev"].view,
                          None if dY is None else dev(dY), None if dYl is None else dev(dYl), fdX.view if want_dX else None,
                          None if g is None else ctypes.byref(g), B, T, n_in, H, NL[nl], NL[rnl], st)
        torch.cuda.synchronize()
        out["dX"] = fdX.host()
        out["grads"] = [b.host() for b in fg]
        fences += [fdX] + fg
        # the backward must not touch what the forward saved
        for k in ("gates", "cell", "hprev"):
            np.testing.assert_array_equal(f[k].host(), out[k], err_msg=f"{k} changed by the backward")
    for v in fences:
        assert v.guards_intact(), "a kernel wrote outside an output buffer"
    call_hip_function("nnhipDeviceError")                      # raises if a kernel raised the device error word
    if raw is not None:
        raw.update(f)
    return out


def run_layer(X, params, dY=None, dYl=None, nl="tanh", rnl="sigmoid", x_requires_grad=True, **kw):
    """The same through nn.LSTM (return_sequences "both"): Y, last, dX (None without x.grad), the twelve gradients."""
    import torch
    import neunet_hip
    import neunet_hip.nn as nn
    B, T, n_in = X.shape
    H = params[4].shape[0]
    m = nn.LSTM(n_in, H, nonlinearity=nl, recurrent_nonlinearity=rnl, **kw)
    for p, a in zip(m.parameters(), params):
        p.data.copy_(dev(a))
    x = neunet_hip.Tensor(X, device="cuda", requires_grad=x_requires_grad)
    Y, last = m(x)
    if dY is not None:
        Y.backward(dev(dY))
    if dYl is not None:
        last.backward(dev(dYl.reshape(B, 1, H)))
    torch.cuda.synchronize()
    return dict(Y=Y.data.cpu().numpy(), hT=last.data.cpu().numpy().reshape(B, H), dX=None if x.grad is None else x.grad.cpu().numpy(),
                grads=[None if p.grad is None else p.grad.cpu().numpy() for p in m.parameters()], x=x, layer=m)


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "numpy-nn-model_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    out_path, seed, B, T, n_in, H = argv[0], *(int(v) for v in argv[1:6])
    import neunet_hip
    neunet_hip.load_library()
    d = make_inputs(seed, B, T, n_in, H)
    out = run_abi(d["X"], d["params"], d["dY"], d["dYl"])
    grads = out.pop("grads")
    np.savez(out_path, resident_env=os.environ.get("NNHIP_LSTM_RESIDENT", ""), **out, **{n: a for n, a in zip(GRADS, grads)})
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
