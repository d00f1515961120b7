#!/usr/bin/env python3
"""GPT-2 inference timings (the shapes of GPT-2 small: 12 layers, 12 heads of 64, d 768, vocab 50257).

    python tools/decode_bench.py [--reps 50] [--skip-generate] > bench.json
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o decode -- python tools/decode_bench.py --families-run 512
    python tools/decode_bench.py --families-summary DIR/.../decode_kernel_stats.csv bench.json 512

  attention   the KV-cached decode kernel (nnhipAttentionDecode) over B in {1, 8, 64} x t in {128, 512, 1024} attended keys, Tmax 1024:
              HIP-event medians per call, cycling through the 12 layers' caches as a decode step does (so a cache that fits the
              256 MiB Infinity Cache is re-read after eleven others, not back to back), with the bytes the call must read
              (2 B H t dh 4) over that time; next to it the only thing the library had for the same maths before:
              nnhipAttentionForward with Tq = 1, Tk = t on dense [B, t, D] keys / values, and two plain streams of the SAME
              number of bytes: read-only (torch.sum) and 1 read + 1 write (nnhipReLUForward).
  rows        nn.LayerNorm and nn.GELU kernels at [16384, 768] and [16384, 3072], forward and backward.
  generate    tokens/s of the three modes of examples/gpt2_infer.py (prompt 128, 128 new tokens, B 1 and 32, random weights), beside
              the floor of streaming every parameter once per step at the measured stream rate; then top_k 40 in graph mode with
              the host sampler (a synchronisation and a [B, vocab] transfer per token) and the device sampler (nnhipSampleTopK
              inside the captured step).
  sampler     one nnhipSampleTopK call (top_k 40) beside one nnhipArgmaxF32 call on the same [B, 50257] logits, B 1 and 32: both
              read every logit once.
  linear      the five Linear shapes of GPT-2 small (768 -> 2304, 768 -> 768, 768 -> 3072, 3072 -> 768, 768 -> 50257) at 1, 2, 4 and 8
              rows: nnhipLinearModuleForwardEx with the GEMV switch off (the tiled GEMM, its split-K reduce included) and
              nnhipLinearGemvForward, alternating in one process over a ring of weight copies larger than the Infinity Cache, as a
              decode step meets its weights; the algorithmic bytes 4 (in out + rows (in + out)) over each time, and the read-only
              stream at the same footprint.  The generate section then runs graph mode at B 1 and 8 with --linear gemm and gemv.
  families    (a rocprofv3 run of its own, then a summary) device time per kernel family of B = 1 graph-replayed decode steps:
              Linear, attention, norms / activations / embedding, the gaps between kernels, and Linear's distance from streaming
              every weight once.
Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "numpy-nn-model_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

H, DH, TMAX, LAYERS = 12, 64, 1024, 12


def event_median(fn, reps, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)          # us


def bench_attention(reps):
    import torch
    from neunet_hip import _lib
    from neunet_hip.nn.experimental.causal_attention import KVCache, attention_decode
    st = _lib.get_current_stream_ptr
    D = H * DH
    out = []
    for B in (1, 8, 64):
        cache = KVCache(B, TMAX, LAYERS, H, DH)
        cache.k.normal_()
        cache.v.normal_()
        qkv = torch.randn((B, 3 * D), device="cuda")
        o = torch.empty((B, D), device="cuda")
        for t in (128, 512, 1024):
            cache.set_lengths([t - 1] * B)
            it = {"i": 0}

            def dec():
                attention_decode(qkv, cache.layer(it["i"] % LAYERS), o, 0.125)
                it["i"] += 1
            us = event_median(dec, reps, warm=LAYERS)
            nbytes = 2 * B * H * t * DH * 4
            # the parent's way: the flash-style forward with one query row, dense [B, t, D] keys / values (one set per layer)
            q = torch.randn((B, 1, D), device="cuda")
            ks = [torch.randn((B, t, D), device="cuda") for _ in range(LAYERS)]
            vs = [torch.randn((B, t, D), device="cuda") for _ in range(LAYERS)]
            ctx = torch.empty((B, 1, D), device="cuda")
            lse = torch.empty((B, H, 1, 2), device="cuda")

            def fwd():
                i = it["i"] % LAYERS
                _lib.call_hip_function("nnhipAttentionForward", q, ks[i], vs[i], None, ctx, lse, B, H, 1, t, DH, D, 0.125, 0, st())
                it["i"] += 1
            try:
                us_fwd = round(event_median(fwd, reps, warm=LAYERS), 2)
            except _lib.NeunetHipError as exc:                          # the entry refuses the shape: say so instead of a time
                us_fwd = f"refused: {exc}"[:160]
            del ks, vs
            # plain streams of the same bytes, over 12 buffers in turn: a READ-ONLY one (torch.sum: the decode kernel reads and writes
            # next to nothing) and the library's 1R1W elementwise stream (nnhipReLUForward, half read, half written)
            n = max(nbytes // 4, 1024)
            xs = [torch.randn(n, device="cuda") for _ in range(LAYERS)]

            def rsum():
                torch.sum(xs[it["i"] % LAYERS])
                it["i"] += 1
            us_read = event_median(rsum, reps, warm=LAYERS)
            y = torch.empty(n // 2, device="cuda")

            def relu():
                _lib.call_hip_function("nnhipReLUForward", y, xs[it["i"] % LAYERS], n // 2, st())
                it["i"] += 1
            us_stream = event_median(relu, reps, warm=LAYERS)
            del xs, y
            out.append({"B": B, "t": t, "bytes": nbytes, "decode_us": round(us, 2), "decode_GBps": round(nbytes / us / 1e3, 1),
                        "attention_forward_tq1_us": us_fwd, "read_stream_us": round(us_read, 2),
                        "read_stream_GBps": round(4 * n / us_read / 1e3, 1), "relu_1r1w_stream_us": round(us_stream, 2),
                        "relu_1r1w_GBps": round(8 * (n // 2) / us_stream / 1e3, 1)})
        del cache
    return out


def bench_rows(reps):
    import torch
    from neunet_hip import _lib
    st = _lib.get_current_stream_ptr
    call = _lib.call_hip_function
    res = []
    rows = 16384
    for cols in (768, 3072):
        X, dY = torch.randn((rows, cols), device="cuda"), torch.randn((rows, cols), device="cuda")
        Y, dX = torch.empty_like(X), torch.empty_like(X)
        w, b = torch.rand(cols, device="cuda") + 0.5, torch.rand(cols, device="cuda")
        dw, db = torch.empty_like(w), torch.empty_like(b)
        mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
        n = rows * cols
        t = {"ln_fwd": event_median(lambda: call("nnhipLayerNormForward", X, w, b, Y, mean, rstd, rows, cols, 1e-5, st()), reps),
             "ln_bwd": event_median(lambda: call("nnhipLayerNormBackward", dY, X, w, mean, rstd, dX, dw, db, rows, cols, st()), reps),
             "gelu_fwd": event_median(lambda: call("nnhipGELUForward", Y, X, n, st()), reps),
             "gelu_bwd": event_median(lambda: call("nnhipGELUBackward", dX, dY, X, n, st()), reps)}
        per = {"ln_fwd": 8, "ln_bwd": 12, "gelu_fwd": 8, "gelu_bwd": 12}        # algorithmic bytes per element
        res.append({"rows": rows, "cols": cols, **{k + "_us": round(v, 2) for k, v in t.items()},
                    **{k + "_GBps": round(per[k] * n / v / 1e3, 1) for k, v in t.items()}})
    return res


LINEAR_SHAPES = ((768, 2304), (768, 768), (768, 3072), (3072, 768), (768, 50257))       # (in, out): c_attn, attn c_proj, c_fc, mlp c_proj, lm_head
LINEAR_ROWS = (1, 2, 4, 8)
RING_BYTES = 600 << 20               # weight copies cycled per shape: more than the 256 MiB Infinity Cache, so every call reads HBM


def bench_linear(reps):
    """Per (shape, rows): median device time of the tiled-GEMM path (switch off) and of the GEMV kernel, alternating call by call."""
    import torch
    import neunet_hip
    from neunet_hip import _lib
    st = _lib.get_current_stream_ptr
    call = _lib.call_hip_function
    res = []
    neunet_hip.set_linear_gemv(False)
    for n_in, n_out in LINEAR_SHAPES:
        copies = max(2, min(256, -(-RING_BYTES // (4 * n_in * n_out))))
        Ws = [torch.randn((n_out, n_in), device="cuda") * 0.02 for _ in range(copies)]
        b = torch.randn((n_out,), device="cuda")
        n = n_in * n_out
        it = {"i": 0}

        def rsum():
            torch.sum(Ws[it["i"] % copies])
            it["i"] += 1
        us_read = event_median(rsum, reps, warm=min(copies, 12))
        for rows in LINEAR_ROWS:
            X = torch.randn((rows, n_in), device="cuda")
            add = torch.randn((rows, n_out), device="cuda")
            O = torch.empty((rows, n_out), device="cuda")
            fns = {"gemm": lambda: call("nnhipLinearModuleForwardEx", X, Ws[it["i"] % copies], b, add, O, rows, n_in, n_out, st()),
                   "gemv": lambda: call("nnhipLinearGemvForward", X, Ws[it["i"] % copies], b, add, O, rows, n_in, n_out, st())}
            ts = {"gemm": [], "gemv": []}
            for k in range(2 * (reps + 6)):                                 # alternate: gemm, gemv, gemm, ... (the first 6 of each: warm-up)
                name = ("gemm", "gemv")[k & 1]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[name]()
                e1.record()
                e1.synchronize()
                it["i"] += 1
                if k >= 12:
                    ts[name].append(e0.elapsed_time(e1) * 1e3)
            us = {k: statistics.median(v) for k, v in ts.items()}
            nbytes = 4 * (n + rows * (n_in + n_out))
            res.append({"in": n_in, "out": n_out, "rows": rows, "bytes": nbytes, "weight_copies_cycled": copies,
                        "gemm_us": round(us["gemm"], 2), "gemv_us": round(us["gemv"], 2),
                        "gemm_GBps": round(nbytes / us["gemm"] / 1e3, 1), "gemv_GBps": round(nbytes / us["gemv"] / 1e3, 1),
                        "gemv_over_gemm": round(us["gemv"] / us["gemm"], 3),
                        "read_stream_us": round(us_read, 2), "read_stream_GBps": round(4 * n / us_read / 1e3, 1),
                        "gemv_over_read_stream": round(us["gemv"] / (us_read * nbytes / (4 * n)), 3)})
        del Ws
    return res


def build_model(seed=0):
    import numpy as np
    import gpt2_infer as G
    np.random.seed(seed)
    model = G.GPT2(dict(G.GPT2_SMALL))
    G.load_gpt2_weights(model, G.random_gpt2_state(G.GPT2_SMALL, seed))
    return G, model


def param_bytes(model):
    seen, n = set(), 0
    for p in model.parameters():
        if id(p) not in seen:
            seen.add(id(p))
            n += p.data.numel() * 4
    return n


def bench_generate(stream_GBps):
    import numpy as np
    G, model = build_model()
    pb = param_bytes(model)
    res = {"param_bytes": pb, "stream_GBps": stream_GBps, "floor_ms_per_step": round(pb / stream_GBps / 1e6, 4), "runs": [],
           "sampled_runs": []}
    rng = np.random.default_rng(1)
    for B in (1, 32):
        ids = rng.integers(0, G.GPT2_SMALL["vocab_size"], (B, 128)).astype(np.int32)
        toks = {}
        for mode in ("recompute", "cached", "graph"):
            G.generate(model, ids, 4, mode=mode)                      # warm every shape family once
            stats = {}
            t0 = time.perf_counter()
            out = G.generate(model, ids, 128, mode=mode, stats=stats)
            wall = time.perf_counter() - t0                           # (generate ends in a device-to-host copy)
            toks[mode] = out
            steps = 128 if mode == "recompute" else 127               # cached / graph: the first new token comes from the prefill
            res["runs"].append({"B": B, "mode": mode, "wall_s": round(wall, 4), "tokens_per_s_end_to_end": round(B * 128 / wall, 1),
                                "decode_s": round(stats["decode_s"], 4), "ms_per_step": round(stats["decode_s"] / steps * 1e3, 4),
                                "tokens_per_s_token_loop": round(B * steps / stats["decode_s"], 1),
                                "prefill_s": round(stats.get("prefill_s", 0.0), 4), "capture_s": round(stats.get("capture_s", 0.0), 4),
                                "kernel_nodes": stats.get("kernel_nodes")})
        res[f"same_tokens_B{B}"] = bool(np.array_equal(toks["cached"], toks["graph"]))
        res[f"recompute_matches_cached_B{B}"] = float(np.mean(toks["cached"] == toks["recompute"]))
        for sampler in ("host", "device"):                            # the reference script's default: top_k 40
            G.generate(model, ids, 4, top_k=40, mode="graph", seed=0, sampler=sampler)
            stats = {}
            t0 = time.perf_counter()
            G.generate(model, ids, 128, top_k=40, mode="graph", seed=0, stats=stats, sampler=sampler)
            wall = time.perf_counter() - t0
            res["sampled_runs"].append({"B": B, "mode": "graph", "top_k": 40, "sampler": sampler, "wall_s": round(wall, 4),
                                        "tokens_per_s_end_to_end": round(B * 128 / wall, 1), "decode_s": round(stats["decode_s"], 4),
                                        "ms_per_step": round(stats["decode_s"] / 127 * 1e3, 4),
                                        "tokens_per_s_token_loop": round(B * 127 / stats["decode_s"], 1),
                                        "host_syncs_between_tokens": stats["host_syncs_between_tokens"],
                                        "kernel_nodes": stats.get("kernel_nodes"), "graph_nodes": stats.get("graph_nodes")})
    # graph mode, greedy, at the batch sizes the GEMV kernel takes (1..8 rows per step): the tiled GEMM beside --linear gemv
    res["linear_runs"] = []
    for B in (1, 8):
        ids = rng.integers(0, G.GPT2_SMALL["vocab_size"], (B, 128)).astype(np.int32)
        toks = {}
        for linear in ("gemm", "gemv"):
            G.generate(model, ids, 4, mode="graph", linear=linear)
            stats = {}
            t0 = time.perf_counter()
            toks[linear] = G.generate(model, ids, 128, mode="graph", stats=stats, linear=linear)
            wall = time.perf_counter() - t0
            res["linear_runs"].append({"B": B, "mode": "graph", "linear": linear, "wall_s": round(wall, 4),
                                       "decode_s": round(stats["decode_s"], 4), "ms_per_step": round(stats["decode_s"] / 127 * 1e3, 4),
                                       "tokens_per_s_token_loop": round(B * 127 / stats["decode_s"], 1),
                                       "kernel_nodes": stats.get("kernel_nodes"), "graph_nodes": stats.get("graph_nodes")})
        res[f"gemv_same_tokens_as_gemm_B{B}"] = bool(np.array_equal(toks["gemm"], toks["gemv"]))      # reported, not required
    return res


def bench_sampler(reps):
    import torch
    import neunet_hip
    from neunet_hip import _lib
    st = _lib.get_current_stream_ptr
    res = []
    for B in (1, 32):
        x = torch.randn((B, 50257), device="cuda") * 3
        out = torch.empty((B,), dtype=torch.int32, device="cuda")
        us_arg = event_median(lambda: _lib.call_hip_function("nnhipArgmaxF32", out, x, B, 50257, 1, st()), reps)
        us_smp = event_median(lambda: neunet_hip.sample_top_k(x, 40, 0.9, seed=1, out=out), reps)
        res.append({"B": B, "n": 50257, "top_k": 40, "argmax_us": round(us_arg, 2), "sample_top_k_us": round(us_smp, 2)})
    return res


def family_of(name):
    """Kernel family of a demangled kernel name, matched on the START of the library's own kernel names."""
    n = name.replace("void ", "").replace("nnhip::", "")
    if n.startswith("attn_decode"):
        return "attention"
    if n.startswith(("gemm_", "sg_", "splitk_", "colsum_", "linear_gemv_")):   # every Linear: the GEMM kernels, their reduces / bias sums, the GEMV
        return "linear"
    if n.startswith(("layernorm_", "map1_kernel", "map2_kernel", "embedding_", "argmax_", "sample_", "at::native")):
        return "norm_act_embed"                                        # (at::native: torch's cache_len += 1)
    return "other"


def families_run(steps):
    """The workload of the per-family profile: B = 1, prompt 128, then `steps` graph-replayed decode steps.  Run it under
    `rocprofv3 --kernel-trace --stats`; the prefill and the one eager warm-up step are in the trace too (about two steps' worth
    of `steps + 1`)."""
    import numpy as np
    import torch
    G, model = build_model()
    model.eval()
    ids = np.random.default_rng(1).integers(0, G.GPT2_SMALL["vocab_size"], (1, 128)).astype(np.int32)
    cache = model.new_cache(1, 128 + steps + 8)
    model(ids, cache=cache, last_only=True)
    step = G.GraphedDecodeStep(model, cache, greedy=True)
    for _ in range(steps):
        step.replay()
    torch.cuda.synchronize()
    step.release()
    print(json.dumps({"families_run_steps": steps, "kernel_nodes": step.kernel_nodes}))


def families_summary(stats_csv, bench_json, steps):
    """rocprofv3's kernel_stats.csv of families_run + the main run's JSON (B = 1 graph ms per step, read-stream rate) ->
    per-family device time per step, its share of the step, the gaps, and how far Linear is from streaming every weight once."""
    import csv
    bench = json.loads(open(bench_json).read().strip().splitlines()[-1])
    gen = bench["generate"]
    ms_step = next(r["ms_per_step"] for r in gen["runs"] if r["B"] == 1 and r["mode"] == "graph")
    fam, names = {"attention": 0.0, "linear": 0.0, "norm_act_embed": 0.0, "other": 0.0}, {}
    for r in csv.DictReader(open(stats_csv)):
        us = float(r["TotalDurationNs"]) / 1e3 / (steps + 1)
        fam[family_of(r["Name"])] += us
        names[r["Name"][:70]] = round(us, 2)
    kernel_ms = sum(fam.values()) / 1e3
    floor_ms = gen["floor_ms_per_step"]
    top = dict(sorted(names.items(), key=lambda kv: -kv[1])[:12])
    print(json.dumps({"families_B1": {
        "source": "rocprofv3 --kernel-trace --stats", "steps": steps, "ms_per_step_unprofiled": ms_step,
        # kernels run longer under the tracer than in the untraced step (a few us each, and a step is ~150 short kernels), so their
        # sum can exceed the untraced step time: the shares are of the traced kernel time, and the gap is only reported when positive
        "kernel_ms_per_step_traced": round(kernel_ms, 4),
        "gaps_ms_per_step": round(ms_step - kernel_ms, 4) if ms_step > kernel_ms else None,
        "family_us_per_step": {k: round(v, 2) for k, v in fam.items()},
        "family_share_of_kernel_time": {k: round(v / 1e3 / kernel_ms, 4) for k, v in fam.items()},
        "param_bytes": gen["param_bytes"], "read_stream_GBps": gen["stream_GBps"], "weight_stream_floor_ms": floor_ms,
        "linear_ms_over_weight_stream_floor": round(fam["linear"] / 1e3 / floor_ms, 2), "top_kernels_us_per_step": top}}))


def main():
    import argparse

    import torch
    import neunet_hip
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--only", default=None, choices=["sampler", "generate", "linear"], help="only this section (generate: with the read-stream "
                    "rate given by --stream-GBps instead of the attention section's measurement)")
    ap.add_argument("--stream-GBps", type=float, default=0.0)
    ap.add_argument("--families-run", type=int, default=0, metavar="STEPS", help="only the workload of the per-family profile")
    ap.add_argument("--families-summary", nargs=3, metavar=("KERNEL_STATS_CSV", "BENCH_JSON", "STEPS"),
                    help="summarise rocprofv3's kernel stats of a --families-run (no device needed)")
    a = ap.parse_args()
    if a.families_summary:
        families_summary(a.families_summary[0], a.families_summary[1], int(a.families_summary[2]))
        return
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs the HIP device: nothing is measured without it")
    neunet_hip.load_library()
    if a.families_run:
        families_run(a.families_run)
        return
    if a.only == "linear":
        print(json.dumps({"linear": bench_linear(a.reps)}))
        return
    if a.only:
        res = {"sampler": bench_sampler(a.reps)}
        if a.only == "generate":
            if a.stream_GBps <= 0:
                raise SystemExit("--only generate needs --stream-GBps (the read-only stream rate the weight-stream floor is computed from)")
            res["generate"] = bench_generate(a.stream_GBps)
        print(json.dumps(res))
        return
    res = {"H": H, "dh": DH, "Tmax": TMAX, "layers_cycled": LAYERS, "attention": bench_attention(a.reps), "rows": bench_rows(a.reps),
           "sampler": bench_sampler(a.reps), "linear": bench_linear(a.reps)}
    if not a.skip_generate:
        big = max(r["read_stream_GBps"] for r in res["attention"])      # the read-only stream at the largest footprint
        res["generate"] = bench_generate(big)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
