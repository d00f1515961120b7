#!/usr/bin/env python3
"""Seq2seq Transformer timings at the notebook's configuration (examples/seq2seq.ipynb cell 13: d_model 256, 8 heads of 32,
d_ff 512, 3 + 3 layers, vocab 15000; random weights).

    python tools/seq2seq_bench.py [--reps 200] [--runs 5] [--only kernel|translate|train] > bench.json

  kernel      nnhipAttentionDecodeCross (without and with the attention map) beside the only thing the library had for the same maths
              before -- nnhipAttentionForward with Tq = 1 on token-major keys / values -- and beside a read-only stream of the same
              bytes (torch.sum), at (B, H, S, dh) = (1, 8, 32, 32), (32, 8, 32, 32), (64, 8, 1024, 64).  The contenders ALTERNATE call by
              call in one process, device events around each call, warm-up first; every contender cycles through one memory per
              decoder layer, as a decode step does.  Median and the 10 % / 90 % quantiles of the repeats.
  translate   tokens/s of the three modes of examples/seq2seq.py translate(): source length 16 and 32, max_length 50, batch 1 and 32,
              end to end (encoder, memory fill and, in graph mode, warm-up + capture included) and over the token loop alone, with
              the kernel nodes of the captured step.  EOS is disabled (eos_idx = -1) so that every run decodes max_length - 1 tokens
              whatever the random weights choose.  Median and range over --runs runs, after one warm-up run per mode and shape.
  train       the eager training step (forward, cross entropy, backward, Adam) at batch 32 on the reverse task, dropout 0.1: a host
              clock around steps that end in a device synchronise.
Prints one JSON line.  Nothing is measured without the HIP device."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "numpy-nn-model_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

KERNEL_SHAPES = ((1, 8, 32, 32), (32, 8, 32, 32), (64, 8, 1024, 64))
LAYERS = 3


def spread(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]  # noqa: E731
    return {"median": round(statistics.median(ts), 2), "p10": round(q(0.1), 2), "p90": round(q(0.9), 2)}


def bench_kernel(reps):
    import torch
    from neunet_hip import _lib
    call, st = _lib.call_hip_function, _lib.get_current_stream_ptr
    out = []
    for B, H, S, dh in KERNEL_SHAPES:
        D = H * dh
        scale = 1.0 / (D ** 0.5)
        q = torch.randn((B, D), device="cuda")
        km = [torch.randn((B, H, S, dh), device="cuda") for _ in range(LAYERS)]
        vm = [torch.randn((B, H, S, dh), device="cuda") for _ in range(LAYERS)]
        kt = [k.permute(0, 2, 1, 3).reshape(B, S, D).contiguous() for k in km]       # the same numbers, token-major
        vt = [v.permute(0, 2, 1, 3).reshape(B, S, D).contiguous() for v in vm]
        valid = torch.ones((B, S), dtype=torch.int32, device="cuda")
        valid[:, S - S // 4:] = 0                                                 # a quarter of the source is padding
        o, p = torch.empty((B, D), device="cuda"), torch.empty((B, H, S), device="cuda")
        ctx, lse = torch.empty((B, 1, D), device="cuda"), torch.empty((B, H, 1, 2), device="cuda")
        nbytes = 2 * B * H * S * dh * 4
        xs = [torch.randn(max(nbytes // 4, 1024), device="cuda") for _ in range(LAYERS)]
        it = {"i": 0}
        fns = {
            "cross_decode": lambda i: call("nnhipAttentionDecodeCross", q, km[i], vm[i], valid, o, None, B, H, S, dh, D, scale, st()),
            "cross_decode_with_map": lambda i: call("nnhipAttentionDecodeCross", q, km[i], vm[i], valid, o, p, B, H, S, dh, D, scale, st()),
            "attention_forward_tq1": lambda i: call("nnhipAttentionForward", q, kt[i], vt[i], valid, ctx, lse, B, H, 1, S, dh, D, scale,
                                                    0, st()),
            "read_stream": lambda i: torch.sum(xs[i]),
        }
        names = list(fns)
        ts = {n: [] for n in names}
        warm = 8 * len(names)
        for k in range(warm + reps * len(names)):                                 # alternate call by call
            n = names[k % len(names)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[n](it["i"] % LAYERS)
            e1.record()
            e1.synchronize()
            if k % len(names) == len(names) - 1:
                it["i"] += 1
            if k >= warm:
                ts[n].append(e0.elapsed_time(e1) * 1e3)
        # the two attention paths compute the same thing
        call("nnhipAttentionDecodeCross", q, km[0], vm[0], valid, o, None, B, H, S, dh, D, scale, st())
        call("nnhipAttentionForward", q, kt[0], vt[0], valid, ctx, lse, B, H, 1, S, dh, D, scale, 0, st())
        err = float((o - ctx.reshape(B, D)).abs().max())
        row = {"B": B, "H": H, "S": S, "dh": dh, "bytes": nbytes, "blocks": B * H, "max_abs_diff_vs_forward": err}
        for n in names:
            row[n + "_us"] = spread(ts[n])
        row["cross_decode_GBps"] = round(nbytes / row["cross_decode_us"]["median"] / 1e3, 1)
        row["forward_tq1_over_cross_decode"] = round(row["attention_forward_tq1_us"]["median"] / row["cross_decode_us"]["median"], 2)
        row["cross_decode_over_read_stream"] = round(row["cross_decode_us"]["median"] / row["read_stream_us"]["median"], 2)
        out.append(row)
    return out


def notebook_model(seed=0, dropout=0.0, max_len=64):
    import numpy as np
    import seq2seq as S
    np.random.seed(seed)
    return S, S.build_seq2seq(dropout=dropout, max_len=max_len, **S.CONFIGS["notebook"])


def bench_translate(runs, max_length=50):
    import numpy as np
    S, model = notebook_model()
    rng = np.random.default_rng(1)
    res = []
    for src_len in (16, 32):
        for B in (1, 32):
            src = [[S.SOS] + rng.integers(3, 15000, src_len - 2).tolist() + [S.EOS] for _ in range(B)]
            toks = {}
            for mode in ("recompute", "cached", "graph"):
                S.translate(model, src, max_length=max_length, mode=mode, eos_idx=-1)              # warm every shape once
                wall, loop, stats = [], [], {}
                for _ in range(runs):
                    stats = {}
                    t0 = time.perf_counter()
                    toks[mode] = S.translate(model, src, max_length=max_length, mode=mode, eos_idx=-1, stats=stats)
                    wall.append(time.perf_counter() - t0)                          # (translate ends in a device-to-host copy)
                    loop.append(stats["decode_s"])
                n = B * (max_length - 1)
                assert all(len(r) == max_length for r in toks[mode])
                res.append({"src_len": src_len, "B": B, "mode": mode, "new_tokens": n,
                            "tokens_per_s_end_to_end": {"median": round(n / statistics.median(wall), 1), "min": round(n / max(wall), 1),
                                                        "max": round(n / min(wall), 1)},
                            "tokens_per_s_token_loop": {"median": round(n / statistics.median(loop), 1), "min": round(n / max(loop), 1),
                                                        "max": round(n / min(loop), 1)},
                            "ms_per_step": round(statistics.median(loop) / (max_length - 1) * 1e3, 4),
                            "host_syncs_between_tokens": stats["host_syncs_between_tokens"], "kernel_nodes": stats.get("kernel_nodes"),
                            "graph_nodes": stats.get("graph_nodes"), "capture_s": round(stats.get("capture_s", 0.0), 4)})
            res.append({"src_len": src_len, "B": B, "cached_equals_graph": toks["cached"] == toks["graph"],
                        "recompute_matches_cached": float(np.mean(np.asarray(toks["cached"]) == np.asarray(toks["recompute"])))})
    return res


def bench_train(steps=30, warm=5, batch=32):
    import torch
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    S, model = notebook_model(dropout=0.1)
    opt = Adam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9)
    loss_fn = nn.CrossEntropyLoss(ignore_index=S.PAD)
    ts, losses = [], []
    for i, (src, tgt) in enumerate(S.reverse_batches(15000, batch, warm + steps, seed=0, min_len=14, max_len=30)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = S.train_step(model, opt, loss_fn, src, tgt)
        torch.cuda.synchronize()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
        losses.append(round(loss.item(), 4))
    return {"batch": batch, "steps": steps, "src_tokens_up_to": 32, "ms_per_step": spread(ts), "first_loss": losses[0], "last_loss": losses[-1]}


def main():
    import argparse

    import torch
    import neunet_hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["kernel", "translate", "train"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seq2seq_bench needs the HIP device: nothing is measured without it")
    neunet_hip.load_library()
    res = {}
    if a.only in (None, "kernel"):
        res["kernel"] = bench_kernel(a.reps)
    if a.only in (None, "translate"):
        res["translate"] = bench_translate(a.runs)
    if a.only in (None, "train"):
        res["train"] = bench_train()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
