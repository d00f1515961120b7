#!/usr/bin/env python3
"""nn.LSTM timings at the recurrent digits classifier's shape (B 100, T 28, H 128; examples/recurrent_classifier.py) and at H 256 / 512
(two and four hidden tiles per wave: lstm_fwd_kernel<false, 2 / 4>, lstm_bwd_kernel<false, 2 / 4>).

    python tools/lstm_bench.py [--reps 50] [--hidden 128 256 512]

Per --hidden size and layer (in 28 and in H): forward and backward entry points (projection GEMM + recurrence, recurrence + parameter GEMMs) from
HIP events, median of --reps, and the recurrence kernels alone per timestep (torch.profiler device times of lstm_fwd_kernel /
lstm_bwd_kernel).  Then the graph-replayed classifier training step: ms per step, samples/s and kernel launches per step.
Prints one JSON line."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "numpy-nn-model_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def event_median(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def kernel_medians(fn, reps, names):
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for n in names:
        ds = [e.device_time for e in prof.events() if n in e.name and e.device_time > 0]   # us
        out[n] = statistics.median(ds) if ds else None
    return out


def main():
    import argparse

    import numpy as np
    import torch
    import neunet_hip
    from neunet_hip import _lib
    from neunet_hip.nn.experimental.recurrent import _padded, _rec_structs
    import neunet_hip.nn as nn
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 256, 512])
    a = ap.parse_args()
    neunet_hip.load_library()
    B, T = 100, 28
    st = _lib.get_current_stream_ptr
    res = {"B": B, "T": T, "resident": os.environ.get("NNHIP_LSTM_RESIDENT", "1") != "0"}
    np.random.seed(0)
    for H, n_in in ((H, n_in) for H in a.hidden for n_in in (28, H)):
        m = nn.LSTM(n_in, H)
        ps = m.parameters()
        Hp = _padded(H)
        X = torch.rand((B, T, n_in), device="cuda") * 2 - 1
        Y, hp = (torch.empty((B, T, H), device="cuda") for _ in range(2))
        gates = torch.empty((B, T, 4 * Hp), device="cuda")
        cell = torch.empty((B, T + 1, H), device="cuda")
        dY = torch.rand((B, T, H), device="cuda")
        dX = torch.empty_like(X)
        grads = [torch.empty_like(p.data) for p in ps]
        w, g = _rec_structs([m], [grads])

        def fwd():
            _lib.call_hip_function("nnhipLSTMForward", X, w, None, None, Y, gates, cell, hp, None, None, B, T, n_in, H, 0, 1, st())

        def bwd():
            _lib.call_hip_function("nnhipLSTMBackward", X, w, gates, cell, hp, dY, None, dX, g, B, T, n_in, H, 0, 1, st())
        for _ in range(5):
            fwd()
            bwd()
        torch.cuda.synchronize()
        kf = kernel_medians(fwd, a.reps, ["lstm_fwd_kernel"])["lstm_fwd_kernel"]
        kb = kernel_medians(bwd, a.reps, ["lstm_bwd_kernel"])["lstm_bwd_kernel"]
        res[f"h{H}_in{n_in}"] = {"fwd_us": round(event_median(fwd, a.reps), 1), "bwd_us": round(event_median(bwd, a.reps), 1),
                            "fwd_recurrence_us": kf and round(kf, 1), "bwd_recurrence_us": kb and round(kb, 1),
                            "fwd_us_per_step": kf and round(kf / T, 2), "bwd_us_per_step": kb and round(kb / T, 2)}

    # the graph-replayed classifier step
    import recurrent_classifier as rc
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    rng = np.random.default_rng(0)
    model = rc.RecurrentClassifier().to("cuda")
    opt = Adam(model.parameters(), lr=1e-4)
    loss_fn = nn.MSELoss()
    x0, t0, _ = rc.synthetic_batch(rng, B)
    xb = neunet_hip.Tensor(x0, device="cuda", requires_grad=False)
    tb = neunet_hip.Tensor(t0, device="cuda", requires_grad=False)

    def fb():
        loss = loss_fn(model(xb), tb)
        loss.backward()
        return loss
    step = GraphedTrainStep(fb, opt, GradBucket(model.parameters()), warmup=3, count_nodes=True)
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ms = event_median(step, a.steps) / 1e3
    res["graphed_step_ms"] = round(ms, 4)
    res["samples_per_s"] = round(B / ms * 1e3, 1)
    res["launches_per_step"] = step.kernel_nodes
    step.release()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
