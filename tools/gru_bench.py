#!/usr/bin/env python3
"""nn.GRU / nn.RNN / nn.Bidirectional timings (csrc/recurrent_gru.hip), beside tools/lstm_bench.py.

    python tools/gru_bench.py [--reps 50] [--rounds 15]

For GRU and RNN at the LSTM's shape (B 100, T 28, in 128, H 128), at the notebook's (B 1, T 5, in 10, H 50) and at H 256 / 512 (two and
four hidden tiles per wave; the GRU's four-tile instances spill): the forward and backward entries from HIP events (median of
--reps) and the recurrence kernels alone per timestep (torch.profiler device times of rec_fwd_kernel / rec_bwd_kernel).  Then one ndir = 2 entry against two ndir = 1 entries on the same weights, alternating in one
process: --rounds rounds of --reps calls each, median and p10-p90 over the rounds' medians.  Then the sentence classifier
(examples/recurrent_sequences.py): steps/s eager and graph-replayed, kernel launches per step.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "numpy-nn-model_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lstm_bench import event_median, kernel_medians  # noqa: E402


def pctl(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def entry_calls(kind, B, T, n_in, H, ndir):
    """(forward, backward) closures over one set of buffers for an ndir-direction call of `kind`."""
    import torch
    import neunet_hip.nn as nn
    from neunet_hip import _lib
    from neunet_hip.nn.experimental.recurrent import _padded, _rec_structs
    layers = [nn.GRU(n_in, H) if kind == "gru" else nn.RNN(n_in, H) for _ in range(ndir)]
    X = torch.rand((B, T, n_in), device="cuda") * 2 - 1
    Y, hp, dY = (torch.rand((ndir, B, T, H), device="cuda") for _ in range(3))
    gates = torch.empty((ndir, B, T, 3 * _padded(H)), device="cuda")
    dX = torch.empty_like(X)
    outs = [[torch.empty_like(p.data) for p in layer._params()] for layer in layers]
    w, g = _rec_structs(layers, outs)
    st = _lib.get_current_stream_ptr
    keep = (layers, outs)
    if kind == "gru":
        def fwd(_keep=keep):
            _lib.call_hip_function("nnhipGRUForward", X, w, None, Y, gates, hp, None, B, T, n_in, H, 0, 1, ndir, st())

        def bwd():
            _lib.call_hip_function("nnhipGRUBackward", X, w, gates, hp, dY, None, dX, g, B, T, n_in, H, 0, 1, ndir, st())
    else:
        def fwd(_keep=keep):
            _lib.call_hip_function("nnhipRNNForward", X, w, None, Y, hp, None, B, T, n_in, H, 0, ndir, st())

        def bwd():
            _lib.call_hip_function("nnhipRNNBackward", X, w, Y, hp, dY, None, dX, g, B, T, n_in, H, 0, ndir, st())
    return fwd, bwd


def main():
    import argparse

    import numpy as np
    import torch
    import neunet_hip
    import neunet_hip.nn as nn
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    neunet_hip.load_library()
    np.random.seed(0)
    res = {}
    # h256 / h512: the widest instance without scratch (two tiles per wave) against the four-tiles-per-wave one, whose GRU variants spill
    shapes = {"lstm_shape": (100, 28, 128, 128), "notebook_shape": (1, 5, 10, 50), "h256": (100, 28, 128, 256), "h512": (100, 28, 128, 512)}
    for tag, (B, T, n_in, H) in shapes.items():
        for kind in ("gru", "rnn"):
            fwd, bwd = entry_calls(kind, B, T, n_in, H, 1)
            for _ in range(5):
                fwd()
                bwd()
            torch.cuda.synchronize()
            kf = kernel_medians(fwd, a.reps, ["rec_fwd_kernel"])["rec_fwd_kernel"]
            kb = kernel_medians(bwd, a.reps, ["rec_bwd_kernel"])["rec_bwd_kernel"]
            res[f"{kind}_{tag}"] = {"B": B, "T": T, "in": n_in, "H": H, "fwd_us": round(event_median(fwd, a.reps), 1),
                                    "bwd_us": round(event_median(bwd, a.reps), 1), "fwd_us_per_step": kf and round(kf / T, 2),
                                    "bwd_us_per_step": kb and round(kb / T, 2)}
            # one two-direction call against two one-direction calls, alternating
            f2, b2 = entry_calls(kind, B, T, n_in, H, 2)
            f1a, b1a = entry_calls(kind, B, T, n_in, H, 1)

            def two_fwd():
                fwd()
                f1a()

            def two_bwd():
                bwd()
                b1a()
            for fn in (f2, b2, two_fwd, two_bwd):
                fn()
            torch.cuda.synchronize()
            rounds = {"ndir2_fwd": [], "two_calls_fwd": [], "ndir2_bwd": [], "two_calls_bwd": []}
            for _ in range(a.rounds):
                for name, fn in (("ndir2_fwd", f2), ("two_calls_fwd", two_fwd), ("ndir2_bwd", b2), ("two_calls_bwd", two_bwd)):
                    rounds[name].append(event_median(fn, a.reps))
            res[f"{kind}_{tag}"]["directions_us"] = {k: {"median": round(statistics.median(v), 1), "p10": round(pctl(v, 0.1), 1),
                                                         "p90": round(pctl(v, 0.9), 1)} for k, v in rounds.items()}

    # the sentence classifier: eager and graph-replayed steps
    import recurrent_sequences as rs
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    np.random.seed(0)
    docs, _ = rs.encode_document()
    model = rs.SequenceClassifier().to("cuda")
    opt = Adam(model.parameters(), lr=1e-3)
    loss_fn = nn.MSELoss()
    tok = neunet_hip.Tensor(docs[0], dtype=np.int32, device="cuda", requires_grad=False)
    lab = neunet_hip.Tensor(np.ones((1, 1, 1), np.float32), device="cuda", requires_grad=False)

    def fb():
        loss = loss_fn(model(tok), lab)
        loss.backward()
        return loss

    def eager():
        opt.zero_grad()
        fb()
        opt.step()
    for _ in range(10):
        eager()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        eager()
    torch.cuda.synchronize()
    res["classifier_eager_steps_per_s"] = round(a.steps / (time.perf_counter() - t0), 1)
    step = GraphedTrainStep(fb, opt, GradBucket(model.parameters()), warmup=3, count_nodes=True)
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    res["classifier_graphed_steps_per_s"] = round(a.steps / (time.perf_counter() - t0), 1)
    res["classifier_graphed_step_us"] = round(event_median(step, a.reps), 1)
    res["classifier_launches_per_step"] = step.kernel_nodes
    step.release()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
