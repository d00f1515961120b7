"""HIPLSTM, HIPGRU, HIPRNN, HIPBidirectional -- the recurrent layers on the one-launch recurrence kernels (csrc/recurrent.hip, ABI 211;
csrc/recurrent_gru.hip, ABI 220; net-new: the reference has no CUDA recurrences).  One set of helpers and one base class serve the
three layers; a layer adds its parameters and whatever of its checks differs.
CPU semantics: neunet/nn/layers/lstm.py -- parameters :187-247, forward :254-408, backward (BPTT) :16-143, nonlinearities :412-460;
gru.py, rnn.py and bidirectional.py as cited below.

A layer's forward is the input projection P = X W_x + b (one GEMM over all B*T rows and every gate) followed by ONE launch that
runs every timestep; the backward is one launch for the recurrence followed by whole-sequence GEMMs for dX and the parameter
gradients.  Whatever T is, a layer costs a fixed handful of launches."""
import copy
from typing import Union

import numpy as np

from ..._lib import GRUGrads, GRUWeights, LSTMGrads, LSTMWeights, RNNGrads, RNNWeights
from ...autograd import Tensor
from ..modules import Module
from ..parameter import Parameter
from .linear import _finish_param, _grad_out
from .utils import call_hip_function, get_current_stream_ptr, require_device_f32

NONLINEARITIES = {"tanh": 0, "sigmoid": 1, "relu": 2}     # include/neunet_hip.h: NNHIP_LSTM_TANH / _SIGMOID / _RELU
MAX_HIDDEN = 512


def _padded(h):
    return (h + 15) // 16 * 16


def _array(v):
    if v is None:
        return None
    return v.data if isinstance(v, Tensor) else v


MERGE_MODES = {"concat": 0, "sum": 1, "mul": 2, "avg": 3}  # include/neunet_hip.h: NNHIP_MERGE_*
_RS = ("both", "all", "last", True, False)
_STRUCTS = {"lstm": (LSTMWeights, LSTMGrads, 4), "gru": (GRUWeights, GRUGrads, 3), "rnn": (RNNWeights, RNNGrads, 1)}   # + gate count


def _check_return_sequences(rs):
    if not any(rs is v or (isinstance(v, str) and rs == v) for v in _RS):
        raise ValueError(f"return_sequences must be 'both', 'all', 'last', True or False, got {rs!r}")


def _rec_structs(layers, outs=None):
    """The ndir weight structs of `layers` (one layer, or the direct and the reverse layer of a Bidirectional) and, with `outs` (one
    list of gradient buffers per layer), the gradient structs."""
    W, G, ng = _STRUCTS[layers[0]._kind]
    w, g = (W * len(layers))(), (G * len(layers))() if outs is not None else None
    for d, layer in enumerate(layers):
        ps = layer._params()
        if ng > 1:                                          # wx[ng] | wh[ng] | b[ng], the order of _params()
            for k in range(ng):
                w[d].wx[k], w[d].wh[k], w[d].b[k] = (ps[k].data.data_ptr(), ps[ng + k].data.data_ptr(), ps[2 * ng + k].data.data_ptr())
                if outs is not None:
                    g[d].dwx[k], g[d].dwh[k], g[d].db[k] = (outs[d][k].data_ptr(), outs[d][ng + k].data_ptr(), outs[d][2 * ng + k].data_ptr())
        else:
            w[d].wx, w[d].wh, w[d].b = (p.data.data_ptr() for p in ps)
            if outs is not None:
                g[d].dwx, g[d].dwh, g[d].db = (o.data_ptr() for o in outs[d])
    return w, g


def _rec_forward(layers, X, h0, hT, c0=None, cT=None):
    """One projection + ONE recurrence launch for the len(layers) directions.  h0: [ndir, B, H] or None; hT: [ndir, B, H], receives the
    last state (it may be h0 itself); c0 / cT: the LSTM's cell state likewise.  Returns (x, Y [ndir, B, T, H], saved)."""
    import torch
    first = layers[0]
    x = X.data if X.data.is_contiguous() else X.data.contiguous()
    if X.ndim == 2:                                         # lstm.py:262-263 / gru.py:230-231 / rnn.py:130-131: a single sequence is batch 1
        x = x.reshape(1, *x.shape)
    B, T, n_in = x.shape
    H, ndir = first.hidden_size, len(layers)
    Y = torch.empty((ndir, B, T, H), dtype=torch.float32, device="cuda")
    hprev_s = torch.empty((ndir, B, T, H), dtype=torch.float32, device="cuda")
    w, _ = _rec_structs(layers)
    nl = NONLINEARITIES[first.nonlinearity]
    saved = dict(X=x, Y=Y, hprev=hprev_s, B=B, T=T, H=H, nl=nl, layers=layers, **{"in": n_in})
    if first._kind != "rnn":
        rnl = NONLINEARITIES[first.recurrent_nonlinearity]
        gates = torch.empty((ndir, B, T, _STRUCTS[first._kind][2] * _padded(H)), dtype=torch.float32, device="cuda")
        saved.update(gates=gates, rnl=rnl)
    if first._kind == "lstm":
        cell = torch.empty((B, T + 1, H), dtype=torch.float32, device="cuda")
        saved.update(cell=cell)
        call_hip_function("nnhipLSTMForward", x, w, h0, c0, Y, gates, cell, hprev_s, hT, cT, B, T, n_in, H, nl, rnl, get_current_stream_ptr())
    elif first._kind == "gru":
        call_hip_function("nnhipGRUForward", x, w, h0, Y, gates, hprev_s, hT, B, T, n_in, H, nl, rnl, ndir, get_current_stream_ptr())
    else:
        call_hip_function("nnhipRNNForward", x, w, h0, Y, hprev_s, hT, B, T, n_in, H, nl, ndir, get_current_stream_ptr())
    return x, Y, saved


def _rec_backward(saved, X, dY, dYlast):
    """ONE recurrence launch backward for every direction, then the whole-sequence GEMMs.  dY [ndir, B, T, H] / dYlast [ndir, B, H]."""
    s = saved
    layers = s["layers"]
    B, T, n_in, H, ndir = s["B"], s["T"], s["in"], s["H"], len(layers)
    dX = X.xp.empty((B, T, n_in), dtype=np.float32) if X.requires_grad else None
    outs = [[_grad_out(p, p.data) for p in layer._params()] for layer in layers]
    w, g = _rec_structs(layers, outs)
    if layers[0]._kind == "lstm":
        call_hip_function("nnhipLSTMBackward", s["X"], w, s["gates"], s["cell"], s["hprev"], dY, dYlast, dX, g, B, T, n_in, H, s["nl"], s["rnl"],
                          get_current_stream_ptr())
    elif layers[0]._kind == "gru":
        call_hip_function("nnhipGRUBackward", s["X"], w, s["gates"], s["hprev"], dY, dYlast, dX, g, B, T, n_in, H, s["nl"], s["rnl"], ndir,
                          get_current_stream_ptr())
    else:
        call_hip_function("nnhipRNNBackward", s["X"], w, s["Y"], s["hprev"], dY, dYlast, dX, g, B, T, n_in, H, s["nl"], ndir,
                          get_current_stream_ptr())
    if dX is not None:
        X.apply_grad(dX.reshape(X.shape))
    for layer, o in zip(layers, outs):
        for p, buf in zip(layer._params(), o):
            _finish_param(p, buf)


class _HIPRecurrentTensor(Tensor):
    """One output of HIPLSTM / HIPGRU / HIPRNN.  `which` is "all" (the gradient of every h_t) or "last" (the gradient of the last h
    alone); each output has its own BPTT grad_fn, as in the reference (lstm.py:400-408, gru.py:344-352, rnn.py:179-187) -- with
    return_sequences="both" the two passes add up in X and the parameters because the gradient is linear."""

    def __init__(self, data, args, device, saved, which):
        super().__init__(data, args, saved["layers"][0]._kind, device=device, _nocopy=True)

        def grad_fn(X, *params, grad):
            grad = grad if grad.is_contiguous() else grad.contiguous()
            _rec_backward(saved, X, *((grad, None) if which == "all" else (None, grad)))

        self.grad_fn = grad_fn


class _HIPRecurrent(Module):
    """What HIPLSTM, HIPGRU and HIPRNN share: the input checks, the state handling and the single-direction call."""
    _kind = ""
    _states = ("hprev",)                                    # the carried states, in the order _run takes them

    def _check(self, X):
        if not isinstance(X, Tensor):
            raise TypeError("Input must be a tensor")
        if X.device != self.device:
            raise ValueError("Tensors must be on the same device")
        require_device_f32(X)
        if X.ndim not in (2, 3):
            raise ValueError(f"{type(self).__name__} expects a (batch, timesteps, input_size) or (timesteps, input_size) input")
        B = 1 if X.ndim == 2 else X.shape[0]
        if self.input_size != X.shape[-1]:
            raise ValueError("input_size must be equal to input shape[2]")
        return B

    def _sequences(self):
        rs = self.return_sequences
        return "all" if rs == "all" or rs is True else "last" if rs == "last" or rs is False else "both"

    def _run(self, X, *given):
        import torch
        B, H = self._check(X), self.hidden_size
        if not self.cycled_states:
            for name, v in zip(self._states, given):
                setattr(self, name, _array(v))
        for name in self._states:
            state = getattr(self, name)
            if state is not None and tuple(state.shape) != (B, H):
                raise ValueError(f"{name} shape must be equal to (batch_size, 1, hidden_size)")
            if self.cycled_states and state is None:
                setattr(self, name, torch.zeros((B, H), dtype=torch.float32, device="cuda"))
        states = [getattr(self, name) for name in self._states]
        first = [None if s is None else s.contiguous().to(torch.float32) for s in states]
        last = torch.empty((B, 1, H), dtype=torch.float32, device="cuda")
        # cycled: the kernel reads the state buffers and writes the new state into the same buffers (each element by its owner thread)
        final = states if self.cycled_states else [last, None]
        x, Y, saved = _rec_forward([self], X, *(s for pair in zip(first, final) for s in pair))     # h0, hT (, c0, cT)
        if self.cycled_states:
            last.copy_(self.hprev.reshape(B, 1, H))
        args = (X, *self._params())
        outs = {"all": Y.reshape(B, x.shape[1], H), "last": last}
        which = self._sequences()
        if which == "both":
            return tuple(_HIPRecurrentTensor(outs[k], args, self.device, saved, k) for k in ("all", "last"))
        return _HIPRecurrentTensor(outs[which], args, self.device, saved, which)


def _uniform_param(stdv, shape):
    return Parameter(Tensor(np.random.uniform(-stdv, stdv, shape), dtype=np.float32))


class HIPLSTM(_HIPRecurrent):
    """neunet.nn.LSTM (lstm.py:168-252) on nnhipLSTMForward / nnhipLSTMBackward.  Differences from the reference, both deliberate:
      * bias=False raises: the reference's `a + b + bias if bias is not None else +0` (lstm.py:313-319) parses as
        `(a + b + bias) if ... else 0`, so without a bias every pre-activation is 0 and the layer outputs zeros whatever the input;
      * with cycled_states the carried (h, c) live in module-owned device buffers that the kernel itself rewrites, so a replayed
        hipGraph carries them from replay to replay exactly as eager calls do.  Their shape is (batch, hidden)."""
    _kind = "lstm"
    _states = ("hprev", "cprev")

    def __init__(self, input_size: int, hidden_size: int, nonlinearity: str = "tanh", recurrent_nonlinearity: str = "sigmoid",
                 return_sequences: Union[str, bool] = "both", bias: bool = True, cycled_states: bool = False, device="cuda"):
        super().__init__()
        for name in (nonlinearity, recurrent_nonlinearity):
            if name not in NONLINEARITIES:
                raise ValueError(f"unknown nonlinearity {name!r}: one of {sorted(NONLINEARITIES)} (lstm.py:460)")
        if not bias:
            raise ValueError("LSTM(bias=False) is not supported: in the reference it outputs zeros whatever the input "
                             "(neunet/nn/layers/lstm.py:318 -- the conditional expression drops the whole pre-activation)")
        if return_sequences not in _RS:                        # by ==, not _check_return_sequences' identity: 1 / 0 pass as True / False
            raise ValueError(f"return_sequences must be 'both', 'all', 'last', True or False, got {return_sequences!r}")
        self.input_size, self.hidden_size = input_size, hidden_size
        self.nonlinearity, self.recurrent_nonlinearity = nonlinearity, recurrent_nonlinearity
        self.return_sequences, self.cycled_states = return_sequences, cycled_states
        stdv = 1.0 / np.sqrt(hidden_size)
        # drawn from the global generator in the reference's order and dtype (float64 draws, stored as float32; lstm.py:187-242)
        for gate in "fioc":
            setattr(self, f"weight_{gate}", _uniform_param(stdv, (input_size, hidden_size)))
        for gate in "fioc":
            setattr(self, f"weight_h{gate}", _uniform_param(stdv, (hidden_size, hidden_size)))
        for gate in "fioc":
            setattr(self, f"bias_{gate}", Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32)))
        self.cprev = None
        self.hprev = None
        self.to(device)

    def _params(self):
        return [self.weight_f, self.weight_i, self.weight_o, self.weight_c, self.weight_hf, self.weight_hi, self.weight_ho,
                self.weight_hc, self.bias_f, self.bias_i, self.bias_o, self.bias_c]

    def _check(self, X):
        B = super()._check(X)
        if self.hidden_size > MAX_HIDDEN:                       # at the call, not at construction as for GRU / RNN
            raise ValueError(f"hidden_size {self.hidden_size} > {MAX_HIDDEN} is not supported by the HIP recurrence kernels")
        return B

    def _sequences(self):
        rs = self.return_sequences                              # by ==, as the constructor's check
        return "all" if rs in ("all", True) else "last" if rs in ("last", False) else "both"

    def forward(self, X: Tensor, hprev=None, cprev=None):
        return self._run(X, hprev, cprev)

    def __call__(self, X, hprev=None, cprev=None):
        return self.forward(X, hprev, cprev)


class HIPGRU(_HIPRecurrent):
    """neunet.nn.GRU (gru.py:127-355) on nnhipGRUForward / nnhipGRUBackward.  Differences from the reference, all deliberate:
      * bias=False raises: `a + b + bias if bias is not None else 0` (gru.py:274-280) parses as `(a + b + bias) if ... else 0`, so
        without a bias every pre-activation is 0 and the layer ignores its input;
      * with cycled_states the carried h lives in a module-owned device buffer (batch, hidden) that the kernel itself rewrites, so a
        replayed hipGraph carries it from replay to replay exactly as eager calls do;
      * cprev is accepted and shape-checked but otherwise unused: in the reference it only fills cell_states[:, -1], which nothing reads."""
    _kind = "gru"

    def __init__(self, input_size: int, hidden_size: int, nonlinearity: str = "tanh", recurrent_nonlinearity: str = "sigmoid",
                 return_sequences: Union[str, bool] = "both", bias: bool = True, cycled_states: bool = False, device="cuda"):
        super().__init__()
        for name in (nonlinearity, recurrent_nonlinearity):
            if name not in NONLINEARITIES:
                raise ValueError(f"unknown nonlinearity {name!r}: one of {sorted(NONLINEARITIES)} (gru.py:404)")
        if not bias:
            raise ValueError("GRU(bias=False) is not supported: in the reference every pre-activation is then 0 whatever the input "
                             "(neunet/nn/layers/gru.py:274-280 -- the conditional expression drops the whole sum)")
        if hidden_size > MAX_HIDDEN:
            raise ValueError(f"hidden_size {hidden_size} > {MAX_HIDDEN} is not supported by the HIP recurrence kernels")
        _check_return_sequences(return_sequences)
        self.input_size, self.hidden_size = input_size, hidden_size
        self.nonlinearity, self.recurrent_nonlinearity = nonlinearity, recurrent_nonlinearity
        self.return_sequences, self.cycled_states = return_sequences, cycled_states
        stdv = 1.0 / np.sqrt(hidden_size)
        # drawn from the global generator in the reference's order and dtype (float64 draws, stored as float32; gru.py:169-215)
        self.weight_z = _uniform_param(stdv, (input_size, hidden_size))
        self.weight_r = _uniform_param(stdv, (input_size, hidden_size))
        self.weight_h = _uniform_param(stdv, (input_size, hidden_size))
        self.weight_hz = _uniform_param(stdv, (hidden_size, hidden_size))
        self.weight_hr = _uniform_param(stdv, (hidden_size, hidden_size))
        self.weight_hh = _uniform_param(stdv, (hidden_size, hidden_size))
        self.bias_z = Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32))
        self.bias_r = Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32))
        self.bias_h = Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32))
        self.cprev = None
        self.hprev = None
        self.to(device)

    def _params(self):
        return [self.weight_z, self.weight_r, self.weight_h, self.weight_hz, self.weight_hr, self.weight_hh, self.bias_z, self.bias_r,
                self.bias_h]

    def forward(self, X: Tensor, hprev=None, cprev=None):
        B = self._check(X)
        c = _array(cprev)
        if c is not None and tuple(c.shape) != (B, self.hidden_size):
            raise ValueError("cprev shape must be equal to (batch_size, 1, hidden_size)")
        return self._run(X, hprev)

    def __call__(self, X, hprev=None, cprev=None):
        return self.forward(X, hprev, cprev)


class HIPRNN(_HIPRecurrent):
    """neunet.nn.RNN (rnn.py:68-190) on nnhipRNNForward / nnhipRNNBackward; argument order as the reference's.  bias=False raises for
    the reason given at HIPGRU (rnn.py:152-158); cycled states as there."""
    _kind = "rnn"

    def __init__(self, input_size: int, hidden_size: int, nonlinearity: str = "tanh", bias: bool = True, cycled_states: bool = False,
                 return_sequences: Union[str, bool] = "both", device="cuda"):
        super().__init__()
        if nonlinearity not in NONLINEARITIES:
            raise ValueError(f"unknown nonlinearity {nonlinearity!r}: one of {sorted(NONLINEARITIES)} (rnn.py:239)")
        if not bias:
            raise ValueError("RNN(bias=False) is not supported: in the reference every pre-activation is then 0 whatever the input "
                             "(neunet/nn/layers/rnn.py:152-158 -- the conditional expression drops the whole sum)")
        if hidden_size > MAX_HIDDEN:
            raise ValueError(f"hidden_size {hidden_size} > {MAX_HIDDEN} is not supported by the HIP recurrence kernels")
        _check_return_sequences(return_sequences)
        self.input_size, self.hidden_size = input_size, hidden_size
        self.nonlinearity = nonlinearity
        self.cycled_states, self.return_sequences = cycled_states, return_sequences
        stdv = 1.0 / np.sqrt(hidden_size)
        self.weight = _uniform_param(stdv, (input_size, hidden_size))             # rnn.py:99-114
        self.weight_h = _uniform_param(stdv, (hidden_size, hidden_size))
        self.bias = Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32))
        self.hprev = None
        self.to(device)

    def _params(self):
        return [self.weight, self.weight_h, self.bias]

    def forward(self, X: Tensor, hprev=None):
        return self._run(X, hprev)

    def __call__(self, X, hprev=None):
        return self.forward(X, hprev)


class _HIPBidirectionalTensor(Tensor):
    """One merged output of HIPBidirectional.  Its grad_fn is the merge's backward (one launch, bidirectional.py:16-23) followed by the
    ndir = 2 recurrence backward: ONE launch for both directions, and X receives one accumulated gradient."""

    def __init__(self, data, args, device, saved, which, mode, D, R):
        super().__init__(data, args, "bidirectional" + saved["layers"][0]._kind, device=device, _nocopy=True)

        def grad_fn(X, *params, grad):
            import torch
            grad = grad if grad.is_contiguous() else grad.contiguous()
            B, T, H = saved["B"], saved["T"], saved["H"]
            rows = B * T if which == "all" else B
            d = torch.empty((2, rows, H), dtype=torch.float32, device="cuda")
            call_hip_function("nnhipBidirectionalMergeBackward", grad, D, R, d[0], d[1], rows, H, mode, get_current_stream_ptr())
            _rec_backward(saved, X, *((d, None) if which == "all" else (None, d)))

        self.grad_fn = grad_fn


class HIPBidirectional(Module):
    """neunet.nn.Bidirectional (bidirectional.py:31-86) over nn.GRU or nn.RNN: both directions run through the ndir = 2 entries -- ONE
    recurrence launch forward and ONE backward -- and the merge is one elementwise launch each way.  The reverse direction reads the
    input backwards and its output is NOT flipped back before the merge (bidirectional.py:55-56); no flipped copy of X is made.
    The reverse layer owns distinct parameters with the direct layer's values (the reference's copy.copy followed by Module.to(), which
    re-creates every Parameter); nothing more is drawn from the generator.  parameters(): the direct layer's, then the reverse layer's.
    Deviations from the reference:
      * return_sequences="both": the reference's backward raises (four saved arguments against a three-argument grad_fn,
        bidirectional.py:62-73); here each of the two outputs routes its gradient to its own pair of layer outputs;
      * nn.LSTM raises NotImplementedError: the ABI-211 LSTM entries have no reverse mode (a follow-up);
      * with a cycled_states layer the two carried states live in one module-owned [2, batch, hidden] buffer (each layer's hprev is
        its half), rewritten by the kernel."""

    def __init__(self, layer, merge_mode: str = "sum", device="cuda"):
        super().__init__()
        if isinstance(layer, HIPLSTM):
            raise NotImplementedError("Bidirectional(LSTM) is not supported yet: the LSTM entries (nnhipLSTMForward / Backward, ABI 211) "
                                      "have no reverse mode; nn.GRU and nn.RNN run both directions in one launch")
        if not isinstance(layer, (HIPGRU, HIPRNN)):
            raise ValueError("Bidirectional layer can only be used with LSTM, GRU or RNN layers")
        if merge_mode not in MERGE_MODES:
            raise ValueError(f"unknown merge_mode {merge_mode!r}: one of {sorted(MERGE_MODES)}")
        self.direct_layer = layer
        self.reverse_layer = copy.copy(layer)
        for name, item in list(layer.__dict__.items()):
            if item.__class__.__name__ == "Parameter":
                self.reverse_layer.__dict__[name] = item.to(item.device)          # Parameter.to always copies
        self.merge_mode = merge_mode
        self.return_sequences = layer.return_sequences
        self._state = None
        self.to(device)

    def forward(self, X: Tensor):
        import torch
        d, r = self.direct_layer, self.reverse_layer
        B, H = d._check(X), d.hidden_size
        h0 = None
        last = torch.empty((2, B, H), dtype=torch.float32, device="cuda")
        if d.cycled_states:
            if self._state is None or tuple(self._state.shape) != (2, B, H):
                self._state = torch.zeros((2, B, H), dtype=torch.float32, device="cuda")
                d.hprev, r.hprev = self._state[0], self._state[1]
            h0 = self._state
        x, Y, saved = _rec_forward([d, r], X, h0, h0 if d.cycled_states else last)
        if d.cycled_states:
            last.copy_(self._state)
        T = x.shape[1]
        mode = MERGE_MODES[self.merge_mode]
        width = 2 * H if self.merge_mode == "concat" else H
        args = (X, *d._params(), *r._params())

        def merged(which):
            src, rows, shape = (Y, B * T, (B, T, width)) if which == "all" else (last, B, (B, 1, width))
            out = torch.empty(shape, dtype=torch.float32, device="cuda")
            call_hip_function("nnhipBidirectionalMergeForward", src[0], src[1], out, rows, H, mode, get_current_stream_ptr())
            return _HIPBidirectionalTensor(out, args, self.device, saved, which, mode, src[0], src[1])

        rs = self.return_sequences
        if isinstance(rs, str) and rs == "both":
            return merged("all"), merged("last")
        return merged("all" if (rs == "all" or rs is True) else "last")
