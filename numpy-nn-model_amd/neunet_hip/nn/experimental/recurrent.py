"""HIPLSTM -- nn.LSTM on the one-launch recurrence kernels (csrc/recurrent.hip, ABI 211; net-new: the reference has no CUDA LSTM).
CPU semantics: neunet/nn/layers/lstm.py -- parameters :187-247, forward :254-408, backward (BPTT) :16-143, nonlinearities :412-460.

A layer's forward is the input projection P = X W_x + b (one GEMM over all B*T rows and the four gates) followed by ONE launch that
runs every timestep; the backward is one launch for the recurrence followed by whole-sequence GEMMs for dX and the twelve parameter
gradients.  Whatever T is, a layer costs a fixed handful of launches."""
import ctypes
from typing import Union

import numpy as np

from ..._lib import LSTMGrads, LSTMWeights
from ...autograd import Tensor
from ..modules import Module
from ..parameter import Parameter
from .linear import _finish_param, _grad_out
from .utils import call_hip_function, get_current_stream_ptr, require_device_f32

NONLINEARITIES = {"tanh": 0, "sigmoid": 1, "relu": 2}     # include/neunet_hip.h: NNHIP_LSTM_TANH / _SIGMOID / _RELU
MAX_HIDDEN = 512


def _padded(h):
    return (h + 15) // 16 * 16


def _weights_struct(params):
    w = LSTMWeights()
    for g in range(4):
        w.wx[g] = params[g].data.data_ptr()
        w.wh[g] = params[4 + g].data.data_ptr()
        w.b[g] = params[8 + g].data.data_ptr()
    return w


def _array(v):
    if v is None:
        return None
    return v.data if isinstance(v, Tensor) else v


class _HIPLSTMTensor(Tensor):
    """One output of HIPLSTM.  `which` is "all" (the gradient of every h_t) or "last" (the gradient of h_{T-1} alone); each output has
    its own BPTT grad_fn, as in the reference (lstm.py:400-408) -- with return_sequences="both" the two passes add up in X and the
    parameters because the gradient is linear."""

    def __init__(self, data, args, device, saved, which):
        super().__init__(data, args, "lstm", device=device, _nocopy=True)

        def grad_fn(X, *params, grad):
            s = saved
            B, T, n_in, H = s["B"], s["T"], s["in"], s["H"]
            grad = grad if grad.is_contiguous() else grad.contiguous()
            dY, dYlast = (grad, None) if which == "all" else (None, grad)
            dX = X.xp.empty((B, T, n_in), dtype=np.float32) if X.requires_grad else None
            outs = [_grad_out(p, p.data) for p in params]
            g = LSTMGrads()
            for k in range(4):
                g.dwx[k] = outs[k].data_ptr()
                g.dwh[k] = outs[4 + k].data_ptr()
                g.db[k] = outs[8 + k].data_ptr()
            call_hip_function("nnhipLSTMBackward", s["X"], ctypes.byref(_weights_struct(params)), s["gates"], s["cell"], s["hprev"],
                              dY, dYlast, dX, ctypes.byref(g), B, T, n_in, H, s["nl"], s["rnl"], get_current_stream_ptr())
            if dX is not None:
                X.apply_grad(dX.reshape(X.shape))
            for p, o in zip(params, outs):
                _finish_param(p, o)

        self.grad_fn = grad_fn


class HIPLSTM(Module):
    """neunet.nn.LSTM (lstm.py:168-252).  Differences from the reference, both deliberate:
      * bias=False raises: the reference's `a + b + bias if bias is not None else +0` (lstm.py:313-319) parses as
        `(a + b + bias) if ... else 0`, so without a bias every pre-activation is 0 and the layer outputs zeros whatever the input;
      * with cycled_states the carried (h, c) live in module-owned device buffers that the kernel itself rewrites, so a replayed
        hipGraph carries them from replay to replay exactly as eager calls do.  Their shape is (batch, hidden)."""

    def __init__(self, input_size: int, hidden_size: int, nonlinearity: str = "tanh", recurrent_nonlinearity: str = "sigmoid",
                 return_sequences: Union[str, bool] = "both", bias: bool = True, cycled_states: bool = False, device="cuda"):
        super().__init__()
        for name in (nonlinearity, recurrent_nonlinearity):
            if name not in NONLINEARITIES:
                raise ValueError(f"unknown nonlinearity {name!r}: one of {sorted(NONLINEARITIES)} (lstm.py:460)")
        if not bias:
            raise ValueError("LSTM(bias=False) is not supported: in the reference it outputs zeros whatever the input "
                             "(neunet/nn/layers/lstm.py:318 -- the conditional expression drops the whole pre-activation)")
        if return_sequences not in ("both", "all", "last", True, False):
            raise ValueError(f"return_sequences must be 'both', 'all', 'last', True or False, got {return_sequences!r}")
        self.input_size, self.hidden_size = input_size, hidden_size
        self.nonlinearity, self.recurrent_nonlinearity = nonlinearity, recurrent_nonlinearity
        self.return_sequences, self.cycled_states = return_sequences, cycled_states
        stdv = 1.0 / np.sqrt(hidden_size)
        # drawn from the global generator in the reference's order and dtype (float64 draws, stored as float32; lstm.py:187-242)
        self.weight_f = Parameter(Tensor(np.random.uniform(-stdv, stdv, (input_size, hidden_size)), dtype=np.float32))
        self.weight_i = Parameter(Tensor(np.random.uniform(-stdv, stdv, (input_size, hidden_size)), dtype=np.float32))
        self.weight_o = Parameter(Tensor(np.random.uniform(-stdv, stdv, (input_size, hidden_size)), dtype=np.float32))
        self.weight_c = Parameter(Tensor(np.random.uniform(-stdv, stdv, (input_size, hidden_size)), dtype=np.float32))
        self.weight_hf = Parameter(Tensor(np.random.uniform(-stdv, stdv, (hidden_size, hidden_size)), dtype=np.float32))
        self.weight_hi = Parameter(Tensor(np.random.uniform(-stdv, stdv, (hidden_size, hidden_size)), dtype=np.float32))
        self.weight_ho = Parameter(Tensor(np.random.uniform(-stdv, stdv, (hidden_size, hidden_size)), dtype=np.float32))
        self.weight_hc = Parameter(Tensor(np.random.uniform(-stdv, stdv, (hidden_size, hidden_size)), dtype=np.float32))
        self.bias_f = Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32))
        self.bias_i = Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32))
        self.bias_o = Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32))
        self.bias_c = Parameter(Tensor(np.zeros(hidden_size), dtype=np.float32))
        self.cprev = None
        self.hprev = None
        self.to(device)

    def _params(self):
        return [self.weight_f, self.weight_i, self.weight_o, self.weight_c, self.weight_hf, self.weight_hi, self.weight_ho,
                self.weight_hc, self.bias_f, self.bias_i, self.bias_o, self.bias_c]

    def forward(self, X: Tensor, hprev=None, cprev=None):
        import torch
        if not isinstance(X, Tensor):
            raise TypeError("Input must be a tensor")
        if X.device != self.device:
            raise ValueError("Tensors must be on the same device")
        require_device_f32(X)
        if X.ndim not in (2, 3):
            raise ValueError("LSTM expects a (batch, timesteps, input_size) or (timesteps, input_size) input")
        if self.hidden_size > MAX_HIDDEN:
            raise ValueError(f"hidden_size {self.hidden_size} > {MAX_HIDDEN} is not supported by the HIP recurrence kernels")
        x = X.data if X.data.is_contiguous() else X.data.contiguous()
        if X.ndim == 2:                                         # lstm.py:262-263: a single sequence is batch 1
            x = x.reshape(1, *x.shape)
        B, T, n_in = x.shape
        H = self.hidden_size
        if not self.cycled_states:
            self.hprev, self.cprev = _array(hprev), _array(cprev)
        if self.hprev is not None and tuple(self.hprev.shape) != (B, H):
            raise ValueError("hprev shape must be equal to (batch_size, 1, hidden_size)")
        if self.cprev is not None and tuple(self.cprev.shape) != (B, H):
            raise ValueError("cprev shape must be equal to (batch_size, 1, hidden_size)")
        if self.input_size != n_in:
            raise ValueError("input_size must be equal to input shape[2]")
        if self.cycled_states:
            if self.hprev is None:
                self.hprev = torch.zeros((B, H), dtype=torch.float32, device="cuda")
            if self.cprev is None:
                self.cprev = torch.zeros((B, H), dtype=torch.float32, device="cuda")
        h0 = None if self.hprev is None else self.hprev.contiguous().to(torch.float32)
        c0 = None if self.cprev is None else self.cprev.contiguous().to(torch.float32)
        Hp = _padded(H)
        Y = torch.empty((B, T, H), dtype=torch.float32, device="cuda")
        gates = torch.empty((B, T, 4 * Hp), dtype=torch.float32, device="cuda")
        cell = torch.empty((B, T + 1, H), dtype=torch.float32, device="cuda")
        hprev_s = torch.empty((B, T, H), dtype=torch.float32, device="cuda")
        last = torch.empty((B, 1, H), dtype=torch.float32, device="cuda")
        # cycled: the kernel reads the state buffers and writes the new state into the same buffers (each element by its owner thread)
        hT = self.hprev if self.cycled_states else last
        cT = self.cprev if self.cycled_states else None
        params = self._params()
        nl, rnl = NONLINEARITIES[self.nonlinearity], NONLINEARITIES[self.recurrent_nonlinearity]
        call_hip_function("nnhipLSTMForward", x, ctypes.byref(_weights_struct(params)), h0, c0, Y, gates, cell, hprev_s, hT, cT,
                          B, T, n_in, H, nl, rnl, get_current_stream_ptr())
        if self.cycled_states:
            last.copy_(self.hprev.reshape(B, 1, H))
        saved = dict(X=x, gates=gates, cell=cell, hprev=hprev_s, B=B, T=T, H=H, nl=nl, rnl=rnl, **{"in": n_in})
        args = (X, *params)
        rs = self.return_sequences
        if rs in ("all", True) and rs is not False:
            return _HIPLSTMTensor(Y, args, self.device, saved, "all")
        if rs in ("last", False):
            return _HIPLSTMTensor(last, args, self.device, saved, "last")
        return _HIPLSTMTensor(Y, args, self.device, saved, "all"), _HIPLSTMTensor(last, args, self.device, saved, "last")

    def __call__(self, X, hprev=None, cprev=None):
        return self.forward(X, hprev, cprev)
