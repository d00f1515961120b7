"""Helpers of tests/test_conv_tiers_gpu.py, and its fresh-process twin: the library reads every NNHIP_CONV_* developer switch once per
process (a `static const` in csrc/conv2d.hip / csrc/conv_mfma.hip), so a switch can only be tested from an interpreter started under it.

run_case(): one table case of tests/conv_ref.py through the C ABI -- nnhipConv2dForward with and without bias, nnhipConv2dBackward with
all three outputs, then dX only, dW only, db only -- every output in a NaN-filled, NaN-fenced buffer, compared with float64.

python tests/conv_child.py [DUMP.npz]   runs child_cases() under whatever the environment says and prints ONE JSON object: the switches it
saw and, per case, the worst error / bound ratio and a sha256 digest of every output, and whatever invariant (fences, NaN left,
separately requested outputs not bit-identical to the joint call) it found broken.  DUMP.npz: every case's dX is saved there too.

python tests/conv_child.py --fused-off   fused_off_main(): the three switches that are no part of the dispatch table."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "numpy-nn-model_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from conv_ref import (ENV, ConvDesc, child_cases, conv2d_backward64, conv2d_forward64, dgrad_abs_sum, dot_rule, forward_abs_sum,  # noqa: E402
                      make_inputs)
from lstm_abi import GUARD, Fenced, dev  # noqa: E402

TENSORS = ("O", "O_nobias", "dX", "dW", "db")


class FencedAt(Fenced):
    """Fenced, with the view `off` floats past a 16-byte boundary (off = 1: 4-byte but not 16-byte aligned)."""

    def __init__(self, shape, off=0):
        import torch
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD + off,), float("nan"), dtype=torch.float32, device="cuda")
        self.view = self.whole[GUARD + off:GUARD + off + n].view(*shape)
        self.lo, self.n = GUARD + off, n
        assert self.view.data_ptr() % 16 == 4 * (off % 4)

    def guards_intact(self):
        import torch
        return bool(torch.isnan(self.whole[:self.lo]).all()) and bool(torch.isnan(self.whole[self.lo + self.n:]).all())


def dev_at(a, off=0):
    """A device copy of `a` whose first element sits `off` floats past a 16-byte boundary."""
    import torch
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.zeros(a.size + off, dtype=torch.float32, device="cuda")
    v = buf[off:off + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def cdesc(d):
    from neunet_hip._lib import Conv2dDesc
    return ctypes.byref(Conv2dDesc(**{k: getattr(d, k) for k in ConvDesc.FIELDS}))


def cpool(p):
    from neunet_hip._lib import Pool2dDesc
    from vision_ref import PoolDesc
    return ctypes.byref(Pool2dDesc(**{k: getattr(p, k) for k in PoolDesc.FIELDS}))


NO_STREAM = ("nnhipDeviceError", "nnhipConv2dWeightGradPooledOk", "nnhipConv2dLeakyMaxPoolForwardOk", "nnhipConv2dLeakyMaxPoolStatsBlocks")


def call(name, *args, stream=None):
    """One C ABI call on torch's current stream (or `stream`); the queries and nnhipDeviceError take no stream."""
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    if name in NO_STREAM:
        return call_hip_function(name, *args)
    return call_hip_function(name, *args, get_current_stream_ptr() if stream is None else stream)


def forward(d, x, w, b, off=0):
    Ho, Wo = d.out_hw()
    o = FencedAt((d.B, d.Cout, Ho, Wo), off)
    call("nnhipConv2dForward", x, w, b, o.view, cdesc(d))
    return o


def backward(d, x, w, g, want=("dX", "dW", "db"), off=0):
    """nnhipConv2dBackward with the outputs in `want` requested (the others NULL) -> {name: FencedAt}."""
    f = dict(dX=FencedAt((d.B, d.Cin, d.H, d.W), off), dW=FencedAt((d.Cout, d.Cin, d.kh, d.kw), off), db=FencedAt((d.Cout,), off))
    call("nnhipConv2dBackward", x, w, g, *[f[k].view if k in want else None for k in ("dX", "dW", "db")], cdesc(d))
    return {k: f[k] for k in want}, [f[k] for k in f if k not in want]


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()[:24]


def scaled_bound(ref, tol=1e-4):
    """assert_close_scaled's bound (tests/test_hip_parity.py): tol * max(|ref|, rms(ref)) per element."""
    ref = np.asarray(ref, np.float64)
    rms = float(np.sqrt(np.mean(ref ** 2))) if ref.size else 0.0
    return tol * np.maximum(np.abs(ref), rms) + 1e-30


def worst(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    if not np.all(np.isfinite(err)):
        return float("inf")
    return float(np.max(err / bound)) if err.size else 0.0


_refs = {}


def references(case):
    """{tensor: (float64 reference, bound)} of a case, computed once per process."""
    if case.name not in _refs:
        d = case.desc
        X, Wt, b, dO = make_inputs(case.name, d)
        O0 = conv2d_forward64(X, Wt, None, d)
        fsum = forward_abs_sum(X, Wt, d)
        O1 = O0 + b.astype(np.float64)[None, :, None, None]
        dX, dW, db = conv2d_backward64(X, Wt, dO, d)
        _refs[case.name] = dict(O=(O1, dot_rule(O1, fsum)), O_nobias=(O0, dot_rule(O0, fsum)), dX=(dX, dot_rule(dX, dgrad_abs_sum(Wt, dO, d))),
                                dW=(dW, scaled_bound(dW)), db=(db, scaled_bound(db)))
    return _refs[case.name]


def run_case(case, keep=False):
    """-> dict(ratios = {tensor: worst error / bound}, digests = {tensor: sha256}, problems = [text]); keep: also host = {tensor: array}."""
    import torch
    d = case.desc
    X, Wt, b, dO = make_inputs(case.name, d)
    x, w, bd, g = dev(X), dev(Wt), dev(b), dev(dO)
    problems, fences = [], []
    o1, o0 = forward(d, x, w, bd), forward(d, x, w, None)
    joint, _ = backward(d, x, w, g)
    out = dict(O=o1, O_nobias=o0, **joint)
    fences += list(out.values())
    for k in ("dX", "dW", "db"):                                           # each output alone: the same bits, nothing else written
        alone, unasked = backward(d, x, w, g, want=(k,))
        fences.append(alone[k])
        if not torch.equal(alone[k].view, joint[k].view):
            problems.append(f"{k} requested alone differs from the joint call")
        if not all(u.untouched() for u in unasked):
            problems.append(f"{k} requested alone: a buffer that was not passed was written")
    torch.cuda.synchronize()
    call("nnhipDeviceError")
    for f in fences:
        if not f.guards_intact():
            problems.append("a kernel wrote outside an output buffer")
    ref = references(case)
    ratios, digests = {}, {}
    for k in TENSORS:
        got = out[k].host()
        if np.isnan(got).any():
            problems.append(f"NaN left in {k}")
        ratios[k] = worst(got, *ref[k])
        digests[k] = digest(out[k].view)
    res = dict(ratios=ratios, digests=digests, problems=problems)
    if keep:
        res["host"] = {k: v.host() for k, v in out.items()}
    return res


def main():
    import torch
    import neunet_hip
    neunet_hip.load_library()
    done, dX = {}, {}
    dump = sys.argv[1] if len(sys.argv) > 1 else None
    for c in child_cases():
        done[c.name] = run_case(c, keep=dump is not None)
        if dump:
            dX[c.name] = done[c.name].pop("host")["dX"]
        r = done[c.name]["ratios"]
        print(f"[child {c.name}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()), file=sys.stderr)
    torch.cuda.synchronize()
    if dump:
        np.savez(dump, **dX)
    print(json.dumps(dict(env={v: os.environ.get(v, "") for v in ENV.values()}, cases=done)))
    return 0


FUSED_OFF = ("NNHIP_CONV_POOL_FWD", "NNHIP_CONV_POOLED_WGRAD", "NNHIP_CONV_DEFER_REDUCE")


def fused_off_main():
    """python tests/conv_child.py --fused-off, started with the three switches of FUSED_OFF at 0 (they are no part of conv_ref.ENV: route()
    has no entry they move).  Prints ONE JSON object: the switches it saw, what the two ...Ok queries answer for the first fused cases, and
    the digests of nt_c8_o16's dW and db from nnhipConv2dBackward under nnhipWeightGradDefer(1), read after the flush."""
    import torch
    import neunet_hip
    from conv_ref import BY_NAME, POOL_FWD_CASES, POOL_WGRAD_CASES
    from vision_ref import PoolDesc
    neunet_hip.load_library()

    def pool_of(d, kh=2, kw=2):
        return PoolDesc(d.B, d.Cout, *d.out_hw(), kh, kw)
    _, df, _ = POOL_FWD_CASES[0]
    _, dw, win, _ = POOL_WGRAD_CASES[0]
    res = dict(env={v: os.environ.get(v, "") for v in FUSED_OFF},
               pool_fwd_ok=call("nnhipConv2dLeakyMaxPoolForwardOk", cdesc(df), cpool(pool_of(df))),
               pooled_wgrad_ok=call("nnhipConv2dWeightGradPooledOk", cdesc(dw), cpool(pool_of(dw, *win))))
    d = BY_NAME["nt_c8_o16"].desc
    X, Wt, _, dO = make_inputs("nt_c8_o16", d)
    call("nnhipWeightGradDefer", 1)
    try:
        out, _ = backward(d, dev(X), dev(Wt), dev(dO))
        call("nnhipWeightGradFlush")
    finally:
        call("nnhipWeightGradDefer", 0)
    torch.cuda.synchronize()
    res["guards_intact"] = all(f.guards_intact() for f in out.values())
    res["digests"] = {k: digest(out[k].view) for k in ("dW", "db")}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(fused_off_main() if sys.argv[1:] == ["--fused-off"] else main())
