#!/usr/bin/env python3
"""Achieved HBM bytes/s of the multi-tensor optimizer step, every rule of csrc/optim_rules.hip beside AdamW (csrc/optim.hip) in one
process.

    python tools/optim_bench.py [--log2-elements 26] [--tensors 16] [--reps 20] [--rounds 9]

One parameter set of 2^26 elements (in --tensors equal tensors: the 16384-element chunk plan) and one gradient set, shared by the
optimizers; each keeps its own states.  A round times --reps consecutive step() calls of each optimizer in turn with HIP events
(the host builds its tables in a fraction of a kernel's time, so the events span back-to-back kernels); the optimizers alternate
within a round, --rounds rounds.  Bytes per element are what the rule has to move: p and g read, p written (12) plus 8 per state
stream -- SGD 12; Momentum, RMSprop, Adagrad 20; Adadelta, Adamax, NAdam and AdamW 28.

The yardstick is AdamW in the same run: a rule meets the bar when its median bytes/s is no lower than AdamW's median less the
min-to-max spread of AdamW's own rounds.  Prints one line per optimizer and one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "numpy-nn-model_amd"))

BYTES_PER_ELEMENT = {"AdamW": 28, "SGD": 12, "Momentum": 20, "RMSprop": 20, "Adagrad": 20, "Adadelta": 28, "Adamax": 28, "NAdam": 28}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elements", type=int, default=26)
    ap.add_argument("--tensors", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    import torch
    import neunet_hip
    from neunet_hip import optim
    from neunet_hip.nn import Parameter
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py needs a HIP device: there is nothing to measure without one")
    total = 1 << a.log2_elements
    per = total // a.tensors
    total = per * a.tensors
    gen = torch.Generator(device="cuda").manual_seed(7)
    params = []
    for _ in range(a.tensors):
        p = Parameter(neunet_hip.Tensor(torch.randn(per, device="cuda", generator=gen), device="cuda"))
        p.grad = torch.randn(per, device="cuda", generator=gen)
        params.append(p)
    opts = {name: getattr(optim, name)(params, lr=1e-4) for name in BYTES_PER_ELEMENT}
    times = {name: [] for name in opts}                       # seconds per step, one entry per round
    for opt in opts.values():                                 # plan upload, code objects
        opt.step()
        opt.step()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, opt in opts.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                opt.step()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e-3 / a.reps)
    assert all(bool(torch.isfinite(p.data).all()) for p in params)

    def rates(name):
        return [BYTES_PER_ELEMENT[name] * total / t for t in times[name]]

    base = rates("AdamW")
    base_med, spread = statistics.median(base), max(base) - min(base)
    bar = base_med - spread
    out = {"elements": total, "tensors": a.tensors, "reps": a.reps, "rounds": a.rounds, "bar_TBps": bar / 1e12,
           "adamw_spread_TBps": spread / 1e12, "rules": {}}
    for name in opts:
        r = rates(name)
        med = statistics.median(r)
        out["rules"][name] = {"bytes_per_element": BYTES_PER_ELEMENT[name], "us_per_step": statistics.median(times[name]) * 1e6,
                              "TBps_median": med / 1e12, "TBps_min": min(r) / 1e12, "TBps_max": max(r) / 1e12,
                              "meets_bar": bool(med >= bar)}
        print(f"{name:9s} {BYTES_PER_ELEMENT[name]:2d} B/elem  {statistics.median(times[name]) * 1e6:8.1f} us/step  "
              f"{med / 1e12:6.3f} TB/s (min {min(r) / 1e12:6.3f}, max {max(r) / 1e12:6.3f})  {'meets' if med >= bar else 'BELOW'} the bar "
              f"{bar / 1e12:6.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
