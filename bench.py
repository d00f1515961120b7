#!/usr/bin/env python3
"""bench.py -- training-step throughput of the neunet dense hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload headline|c1|c2|c3|c4|c5] [--full] [--dump-outputs DIR]

BASELINE.json's metric: "samples/sec training step (MNIST-MLP & GPT-tiny) at 1/2/4/8 GPUs; Linear fwd GFLOP/s vs
MFMA peak".  A plain run of the default workload ("headline") sets up, warms up, times the steps and prints ONE JSON line:
  * value / ms_per_step : the C4 GPT-tiny training step (d512 L6 H8 d_ff2048 vocab15000, batch 64 x seq 256 per GPU,
                          weak scaling): the W warm-up + exactly K timed steps of the contract;
  * roofline            : the GEMM-equivalent TFLOP/s of those timed steps (their HIP-event device time) vs the fp32 MFMA peak;
  * gemm_mode           : 0 (exact fp32 MFMA) -- the run exits 4 otherwise: `dtype: f32` and `value` are defined for that mode only.
`--dump-outputs DIR` (headline / c4) then writes what the last timed step computed: loss.npy, param.<key>.npy and grad.<key>.npy
for every trained parameter (keys of Module.state_dict(); tensors above 32768 elements as a fixed, seeded sample of their flat
indices), float32, under 64 MB; the inputs and the initial weights are seeded, so two builds can be compared output for output.

`--full` adds everything else it measures, each in runs of its own after the timed steps:
  * roofline            : the C2 Linear(4096->4096) forward GEMM, batch 4096 -- the metric's "Linear fwd vs MFMA peak"
                          half: HIP-event timed launches of the same gemm_f32_kernel that does 86 % of the C4 step;
  * also.c1             : MNIST-MLP (784->128->10, batch 32 per GPU) training-step samples/s, sustained over 512 steps (16 per captured graph), also with the per-replay input copy and with the separate optimizer launch;
  * also.c2             : the whole C2 training step (fwd + bwd + AdamW) and a sustained (>= 2 s) forward figure;
  * also.c4_gemm        : GEMM-equivalent TFLOP/s of the whole C4 step;
  * also.c3 / also.c5   : every op of the fused micro-bench (rows 8192 x d 4096) with its HBM / MFMA fraction; the conv classifier step;
  * also.c4_strong      : (N > 1) the strong-scaling step next to the weak-scaling `value`;
  * cpu_baseline        : the NumPy oracle's FULL GPT-tiny step (forward, backward, Adam): live n = 1 on the whole per-GPU batch + the
                          committed n = 3 collection of the same step (profiles/cpu_c4_full_batch.json); --workload cN: that config's;
  * also.c4_families    : every GEMM / attention launch of the step at its own shape, isolated (HIP events) and INSIDE the replayed step
                          (`instep_ms`, from the committed rocprofv3 trace, profiles/c4_instep_families.json); roofline.instep likewise;
  * allreduce_ms        : (N > 1 or --force-dp, headline / c4) the gradient exchange alone (`total`) and what it adds to the step
                          (`exposed`); RCCL's own algorithm / protocol lines (`rccl`) are in every N > 1 line;
  * also.linear_swish_sweep : the reference's Linear->Swish bench sweep (scripts/benchmark_linear_swish_cuda.py:127-138), its methodology.
`--workload c1..c5` runs one BASELINE config on its own with the per-config detail (C3: per-op HBM fractions).

`--gpus N` with no torchrun environment re-executes itself under torch.distributed.run with N ranks (one per GPU,
backend nccl = RCCL); under torchrun (the driver's launch) it reads RANK / LOCAL_RANK / WORLD_SIZE.  `rccl_ranks` in
the JSON is dist.get_world_size() after a real all-reduce.
Inputs and weights are resident in HBM before any timed region.  One JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "numpy-nn-model_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md "Peak FP32 (matrix)"
PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md "HBM3E peak BW" (spec; ~6.3 TB/s achievable)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="headline", choices=["headline", "c1", "c2", "c3", "c4", "c5", "nb"])
    ap.add_argument("--c1-steps", type=int, default=512, help="headline: sustained MNIST-MLP steps (a multiple of 16: 16 steps per captured graph)")
    ap.add_argument("--overlap", type=int, default=1, help="N>1: overlap the gradient exchange with the backward pass")
    ap.add_argument("--c4-batch", type=int, default=64, help="sequences per GPU for the GPT-tiny workload")
    ap.add_argument("--graph", type=int, default=1, help="c1/c4: replay the step as a captured hipGraph (1) or launch eagerly (0)")
    ap.add_argument("--unroll", type=int, default=16, help="c1/c5, one process: at most this many training steps captured per hipGraph "
                                                          "(the largest divisor of --steps not above it is used; 1 = one step per replay)")
    ap.add_argument("--force-dp", action="store_true",
                    help="one rank: run the data-parallel machinery anyway (1-rank nccl = RCCL process group, bucket segments, "
                         "graph cuts, async all-reduce, 'sum' loss + device-side divisor)")
    ap.add_argument("--dp-ingraph", type=int, default=int(os.environ.get("NNHIP_DP_INGRAPH", "0")),
                    help="DP + hipGraph: capture the all-reduces INTO the step graph (falls back to graph pieces if refused)")
    ap.add_argument("--dp-op", default="sum", choices=["sum", "avg"],
                    help="reduction of the gradient all-reduce (avg: RCCL pre-scales by 1/world; on a forced 1-rank group it is "
                         "what makes RCCL launch a device kernel -- a 1-rank in-place SUM is elided by the library)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: 64 sequences (C4) per GPU; strong: the global batch of 64 sequences divided over the ranks "
                         "(SURVEY 8e asks for both curves; an N > 1 headline run reports the other one under also.c4_strong)")
    ap.add_argument("--comm", default=os.environ.get("NNHIP_COMM", "torch"), choices=["torch", "native"],
                    help="gradient exchange backend of the C4 step: torch.distributed (nccl = RCCL) or the library's own RCCL "
                         "entry points (nnhipCommInitRank / nnhipAllReduceSumF32 behind neunet_hip.distributed.NativeComm)")
    ap.add_argument("--c1-input-copy", type=int, default=0,
                    help="c1: 1 = every step first copies its batch (100 KB pinned host -> the static device slot), as the "
                         "reference's benches do (benchmark_linear_swish_cuda.py:31)")
    ap.add_argument("--c1-fuse-opt", type=int, default=int(os.environ.get("NNHIP_C1_FUSE_OPT", "2")),
                    help="c1: 2 = the default a README user gets (no opt-in: the backward launch waits for optimizer.step() and "
                         "takes Adam with it); 1 = optimizer.fuse_backward(True) (Adam inside the launch issued by backward()); "
                         "0 = backward and Adam as two launches (NNHIP_AUTO_FUSE_STEP=0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--cpu-full-batch", action="store_true",
                    help="time --cpu-full-steps full-batch (64 x 256) NumPy-oracle GPT-tiny steps, print them as JSON and exit (no GPU work): "
                         "the n >= 3 collection committed as profiles/cpu_c4_full_batch.json, which the live n = 1 sample of every line cites")
    ap.add_argument("--cpu-full-steps", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides the timed steps of the chosen workload: the headline's roofline and `also` "
                         "legs (other configs, kernel families, the opt-in bf16x3 mode, the Linear->Swish sweep), the gradient "
                         "exchange on its own (allreduce_ms) and the CPU baseline.  Off: setup, warm-up, the timed steps, the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (loss, updated parameters, gradients; "
                         "a fixed sample of the larger tensors) as DIR/<name>.npy, float32, at most 64 MB in all")
    return ap.parse_args()


def timed_region(step_fn, steps, warmup, world, min_warm_s=0.0):
    """W untimed steps, then EXACTLY K steps bracketed by barrier + synchronize; max over ranks.
    min_warm_s: sub-millisecond steps (C1, C5) keep stepping untimed until that much wall time has passed -- a GPU that
    has idled sits in a low power state and replays the same graph ~2x slower for the first few hundred ms."""
    import torch
    import torch.distributed as dist
    # The timed steps record one HIP-event pair each (device time per step).  The first few hundred timing events of a
    # process are slow to create (the runtime grows its signal pool in chunks: ~35 ms in total, measured) -- a fixed cost
    # that would double the reported time of a workload whose whole timed region is 30 ms (C1).  Warm the pool here.
    pool = [torch.cuda.Event(enable_timing=True) for _ in range(2 * min(steps, 4096) + 2)]
    for e in pool:
        e.record()
    torch.cuda.synchronize()
    pool[0].elapsed_time(pool[-1])
    del pool
    tw = time.perf_counter()
    for _ in range(warmup):
        step_fn(False)
    if min_warm_s > 0.0 and warmup > 0:
        torch.cuda.synchronize()
        el = time.perf_counter() - tw
        extra = max(0, min(20000, int((min_warm_s - el) / max(el / warmup, 1e-6))))
        if world > 1:                                   # every rank must replay the same number of (collective) steps
            n = torch.tensor([extra], dtype=torch.int64, device="cuda")
            dist.all_reduce(n, op=dist.ReduceOp.MAX)
            extra = int(n.item())
        for _ in range(extra):
            step_fn(False)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step_fn(True)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


def graph_unroll(args, world):
    """Steps captured per hipGraph for the sub-0.1 ms workloads (C1, C5): U > 1 only for one process replaying graphs, and only
    when the requested step counts are whole numbers of replays (EXACTLY --steps steps are timed either way)."""
    from neunet_hip.distributed import collectives_live
    U = max(1, int(args.unroll))
    if world != 1 or collectives_live() or not args.graph:
        return 1
    # the largest divisor of --steps that is <= --unroll: 500 steps -> 10 per graph, 8000 -> 16, 20 -> 10
    return max(d for d in range(1, min(U, args.steps) + 1) if args.steps % d == 0)


class EventTimer:
    """HIP-event pairs on the launch stream (torch's current stream == the stream handed to the C ABI)."""

    def __init__(self):
        self.pairs = []

    def span(self):
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pairs.append((a, b))
        return a, b

    def mean_ms(self):
        return float(np.mean([a.elapsed_time(b) for a, b in self.pairs])) if self.pairs else float("nan")

    def median_ms(self):
        """Median of the spans: one sample that caught a host stall between its two records (the device idle, waiting for the
        next launch) no longer decides the figure (round-5 review: C1's mean device time came out ABOVE its wall time)."""
        return float(np.median([a.elapsed_time(b) for a, b in self.pairs])) if self.pairs else float("nan")


def device_step_ms(ev, per_call, wall_ms_per_step):
    """Device time of one step from the sampled event spans (median), or None when it cannot be trusted: an event pair also spans
    whatever the host did between its two records, so a figure more than 5 % ABOVE the wall-clock time per step of the same timed
    region measured host stalls, not the device -- dropped rather than reported."""
    if not ev.pairs:
        return None
    ms = ev.median_ms() / per_call
    return ms if ms <= 1.05 * wall_ms_per_step else None


def read_traffic(tag):
    """HBM bytes per launch from the committed PMC pass (profiles/pmc_traffic.json: separate rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE passes over this same bench.py, tools/collect_profiles.sh + tools/make_profiles.sh), or None.  A static
    number the current run did not measure: traffic_source() says which collection it is from."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(path):
        try:
            return json.load(open(path)).get(tag)
        except Exception:
            return None
    return None


def read_instep():
    """Per-family kernel durations INSIDE the replayed C4 step (profiles/c4_instep_families.json: rocprofv3 --kernel-trace of
    `bench.py --workload c4`, tools/c4_instep.py), or {}.  Static: collected once per round, not by this run."""
    path = os.path.join(ROOT, "profiles", "c4_instep_families.json")
    try:
        return json.load(open(path))
    except Exception:
        return {}


def traffic_source():
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        d = json.load(open(path))
        tag = d.get("_collected") or (d.get("_note", "").rsplit("round ", 1)[-1].rstrip(". ") or "?")
        return f"profiles/pmc_traffic.json (rocprofv3 --pmc passes, collection {tag}; not measured by this run)"
    except Exception:
        return None


DUMP_LIMIT_BYTES = 64 << 20     # --dump-outputs: at most this much in all
DUMP_SAMPLE = 32768             # elements kept of a larger tensor: a fixed, seeded choice of flat indices


def named_parameters(module, prefix=""):
    """(key, Parameter) pairs of a module tree under the keys Module.state_dict() gives them (nn/modules.py), in that order."""
    children = getattr(module, "modules", None)
    if isinstance(children, list):                  # Sequential / ModuleList: children keyed by their index
        for i, m in enumerate(children):
            if hasattr(m, "state_dict"):
                yield from named_parameters(m, f"{prefix}{i}.")
        return
    for name, item in module.__dict__.items():
        if item.__class__.__name__ == "Parameter":
            yield prefix + name, item
        elif hasattr(item, "state_dict"):
            yield from named_parameters(item, prefix + name + ".")


def dump_sample(name, a):
    """The whole tensor (flattened) up to DUMP_SAMPLE elements, else the same DUMP_SAMPLE flat indices in every run (seeded by name)."""
    import zlib
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if a.size <= DUMP_SAMPLE:
        return a
    idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, DUMP_SAMPLE, replace=False))
    return a[idx]


def dump_outputs(out_dir, arrays):
    """--dump-outputs: write [(name, array)] as out_dir/<name>.npy (float32), refusing to go past DUMP_LIMIT_BYTES."""
    total = sum(a.nbytes for _, a in arrays)
    if total > DUMP_LIMIT_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes of outputs, more than the {DUMP_LIMIT_BYTES} allowed")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays:
        np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"[bench] wrote {len(arrays)} arrays ({total / 2**20:.1f} MB) to {out_dir}", file=sys.stderr)


def c4_step_outputs(model, loss, active):
    """What a caller of the C4 training step holds after it: the loss, and every trained parameter with its gradient
    (p.grad is the gradient bucket's view of the last step), each sampled by dump_sample."""
    import torch
    arrays = [("loss", np.asarray(loss.numpy(), dtype=np.float32).reshape(-1))]
    seen, trained = set(), {id(p) for p in active}
    for key, p in named_parameters(model):
        if id(p) in seen or id(p) not in trained:
            continue
        seen.add(id(p))
        arrays.append(("param." + key, dump_sample("param." + key, p.numpy())))
        g = p.grad.detach().cpu().numpy() if isinstance(p.grad, torch.Tensor) else p.grad.numpy()
        arrays.append(("grad." + key, dump_sample("grad." + key, g)))
    if len(seen) != len(trained):
        raise RuntimeError(f"--dump-outputs: {len(trained) - len(seen)} trained parameter(s) have no state_dict key")
    return arrays


# ------------------------------------------------------------------------------------------------ C2
def workload_c2(args, rank, world):
    import torch
    import neunet_hip
    from neunet_hip.distributed import GradBucket
    from neunet_hip.nn.experimental import HIPLinear
    from neunet_hip.optim import HIPFusedMultiTensorAdamW
    Bsz, D = 4096, 4096
    rng = np.random.default_rng(1002)                     # same weights on every rank
    layer = HIPLinear(D, D)
    layer.weight.data.copy_(torch.from_numpy(rng.uniform(-1 / 64, 1 / 64, (D, D)).astype(np.float32)))
    layer.bias.data.copy_(torch.from_numpy(rng.uniform(-1 / 64, 1 / 64, (1, D)).astype(np.float32)))
    drng = np.random.default_rng(2000 + rank)             # a different shard per rank
    X = neunet_hip.Tensor(drng.uniform(-1, 1, (Bsz, D)).astype(np.float32), device="cuda", requires_grad=True)
    dO = torch.from_numpy(drng.uniform(-1, 1, (Bsz, D)).astype(np.float32)).cuda()
    params = layer.parameters()
    # N > 1: dW/db are computed first and their all-reduce is launched asynchronously, under the dX GEMM
    # (NNHIP_DP_OVERLAP=0 -> one blocking all-reduce after backward)
    overlap = world > 1 and os.environ.get("NNHIP_DP_OVERLAP", "1") != "0"
    bucket = GradBucket(params, overlap=overlap)
    opt = HIPFusedMultiTensorAdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    opt.grad_scale = 1.0 / world
    fwd_t, bwd_t = EventTimer(), EventTimer()

    def step(timed):
        opt.zero_grad()
        X.grad = None
        if timed:
            a, b = fwd_t.span()
            a.record()
        out = layer(X)
        out.data                  # HIPLinear defers its GEMM until the output is read (a loss would): launch it here
        if timed:
            b.record()
            c, d = bwd_t.span()
            c.record()
        out.backward(dO)
        if timed:
            d.record()
        bucket.all_reduce()
        opt.step()

    if overlap:
        # one probing step outside the timed region: if the asynchronous exchange cannot run on this stack, fall back to
        # the plain bucket (identical results, the exchange just is not hidden) instead of losing the measurement
        try:
            step(False)
            torch.cuda.synchronize()
        except Exception as exc:  # noqa: BLE001
            print(f"[bench] overlapped all-reduce unavailable ({exc!r}); using the blocking exchange", file=sys.stderr)
            bucket.detach()
            bucket = GradBucket(params)
    dt = timed_region(step, args.steps, args.warmup, world)
    flops = 2.0 * Bsz * D * D
    fwd_ms, bwd_ms = fwd_t.mean_ms(), bwd_t.mean_ms()
    ach = flops / (fwd_ms * 1e-3) / 1e12
    res = {
        "samples_per_step": Bsz * world,
        "dt": dt,
        "config": {"workload": "C2: Linear(4096->4096) training step (fwd + bwd + grad all-reduce + fused AdamW), "
                               "batch 4096 per GPU, fp32 MFMA", "global_batch": Bsz * world,
                   "parallelism": f"dp{world}"},
        "roofline": {"kernel": "gemm_f32_kernel<32,k-major,k-major> (Linear forward, 1 launch/step)",
                     "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4), "traffic": read_traffic("gemm_fwd_c2"),
                     "flops_per_launch": flops, "avg_launch_ms": round(fwd_ms, 4)},
        "extra": {"linear_fwd_tflops": round(ach, 2),
                  "linear_bwd_tflops": round(2 * flops / (bwd_ms * 1e-3) / 1e12, 2),
                  "linear_bwd_ms": round(bwd_ms, 4),
                  "note": "bwd = dX GEMM + dW GEMM + db column-sum (2 small kernels)",
                  "dp_exchange": ("overlapped per-segment all-reduce" if bucket.overlap else "one blocking all-reduce") if world > 1 else "none"},
    }
    return res


def cpu_c2(seconds):
    """The same step through the NumPy oracle (= the reference's CPU algorithm) on the host cores."""
    from oracle import neunet_oracle as O
    Bsz, D = 4096, 4096
    rng = np.random.default_rng(1002)
    W = rng.uniform(-1 / 64, 1 / 64, (D, D)).astype(np.float32)
    b = rng.uniform(-1 / 64, 1 / 64, (1, D)).astype(np.float32)
    X = rng.uniform(-1, 1, (Bsz, D)).astype(np.float32)
    dO = rng.uniform(-1, 1, (Bsz, D)).astype(np.float32)
    mW, vW, mb, vb = np.zeros_like(W), np.zeros_like(W), np.zeros_like(b), np.zeros_like(b)

    def step(t):
        nonlocal mW, vW, mb, vb
        O.linear_forward(X, W, b)
        _, dW, db = O.linear_backward(X, W, b, dO)
        mW, vW = O.adamw_step(W, dW, mW, vW, t, 1e-3, (0.9, 0.999), 1e-8, 1e-2)
        mb, vb = O.adamw_step(b, db, mb, vb, t, 1e-3, (0.9, 0.999), 1e-8, 1e-2)

    step(1)
    times, t, t_start = [], 2, time.perf_counter()
    while time.perf_counter() - t_start < seconds and len(times) < 50:
        t0 = time.perf_counter()
        step(t)
        times.append(time.perf_counter() - t0)
        t += 1
    best = min(times)
    return {"value": round(Bsz / best, 2), "unit": "samples/s", "cores": blas_threads(), "kind": "port",
            "sample": f"{len(times)} full C2 steps (Linear 4096x4096x4096 fwd+bwd+AdamW) via the NumPy oracle, "
                      f"min step {best * 1e3:.1f} ms, OpenBLAS threads={blas_threads()}, host cpus={os.cpu_count()}"}


# ------------------------------------------------------------------------------------------------ C1
def workload_c1(args, rank, world):
    """README quick-start MLP 784->128->10, batch 32 per GPU, CE(mean) + Adam(1e-3): launch-latency bound."""
    import torch
    import neunet_hip
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.optim import Adam
    Bsz = 32
    np.random.seed(1001)

    class MLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.l1 = nn.Linear(784, 128)
            self.relu = nn.ReLU()
            self.l2 = nn.Linear(128, 10)

        def forward(self, x):
            return self.l2(self.relu(self.l1(x)))

    model = MLP()
    params = model.parameters()
    bucket = GradBucket(params)
    opt = Adam(params, lr=1e-3)
    opt.grad_scale = 1.0 / world
    opt_mode = int(getattr(args, "c1_fuse_opt", 2)) if world == 1 else 0
    import neunet_hip.nn.experimental.linear as _lin
    auto_was = _lin._AUTO_FUSE_STEP
    _lin._AUTO_FUSE_STEP = auto_was and opt_mode != 0      # 0: the two-launch comparison line
    if opt_mode == 1:
        opt.fuse_backward(True)     # opt-in: the launch issued by backward() applies Adam itself (bit-identical to the separate launch)
    fused_opt = opt_mode != 0 and (opt_mode == 1 or _lin._AUTO_FUSE_STEP)
    loss_fn = nn.CrossEntropyLoss()
    drng = np.random.default_rng(3000 + rank)
    U = graph_unroll(args, world)                        # steps per captured graph, each reading its own static batch slot
    Xs = [neunet_hip.Tensor(drng.uniform(-1, 1, (Bsz, 784)).astype(np.float32), device="cuda", requires_grad=False) for _ in range(U)]
    Ys = [neunet_hip.Tensor(drng.integers(0, 10, Bsz).astype(np.int32), dtype=np.int32, requires_grad=False, device="cuda")
          for _ in range(U)]
    ev = EventTimer()
    from neunet_hip.graph import GraphedTrainStep
    # --c1-input-copy 1: the batch of every step crosses PCIe inside the timed region (pinned host -> static device slot,
    # asynchronous on the launch stream), as in the reference's benches (scripts/benchmark_linear_swish_cuda.py:31 copies its
    # input every iteration); 0: the batches are resident (the bench contract's "inputs already in HBM")
    feed = bool(getattr(args, "c1_input_copy", 0))
    launches = None
    if feed:
        # The U static batch slots of a captured graph (inputs and labels) are views into ONE device buffer, filled from ONE pinned
        # host buffer with ONE asynchronous copy per replay: a graph of U steps needs its U batches up front anyway, and 2 U small
        # copies cost the host ~2.4 us each (round 4, first version: 0.0466 ms per step against 0.0232 with resident batches).
        xb, yb = Bsz * 784 * 4, Bsz * 4
        slot = (xb + yb + 255) // 256 * 256
        dbuf = torch.empty(U * slot, dtype=torch.uint8, device="cuda")
        hbuf = torch.empty(U * slot, dtype=torch.uint8).pin_memory()
        for k in range(U):
            hbuf[k * slot: k * slot + xb].view(torch.float32).copy_(torch.from_numpy(drng.uniform(-1, 1, Bsz * 784).astype(np.float32)))
            hbuf[k * slot + xb: k * slot + xb + yb].view(torch.int32).copy_(torch.from_numpy(drng.integers(0, 10, Bsz).astype(np.int32)))
            Xs[k].data = dbuf[k * slot: k * slot + xb].view(torch.float32).view(Bsz, 784)
            Ys[k].data = dbuf[k * slot + xb: k * slot + xb + yb].view(torch.int32)
        dbuf.copy_(hbuf)

        def copy_in():
            dbuf.copy_(hbuf, non_blocking=True)
    else:
        def copy_in():
            pass

    def fwd_bwd(k=0):
        loss = loss_fn(model(Xs[k]), Ys[k])
        loss.backward()
        return loss

    if args.graph:
        gstep = GraphedTrainStep(fwd_bwd, opt, bucket, warmup=3, world=world, unroll=U, count_nodes=True)
        if gstep.kernel_nodes:
            launches = round(gstep.kernel_nodes / U, 2)
        tick = [0]
        n_calls = max(1, args.steps // U)
        every = 16 if n_calls >= 64 else max(1, n_calls // 4)      # short runs: still a few device-time samples

        def step(timed):
            # the device-time events go around every 16th step only: at ~0.06 ms per step two event records per step are a
            # measurable part of what they measure (host time and two more device-side nodes between the graph launches)
            tick[0] += 1
            sample = timed and tick[0] % every == 0
            if sample:
                a, b = ev.span()
                a.record()
            copy_in()
            gstep()
            if sample:
                b.record()
    else:
        def step(timed):
            if timed:
                a, b = ev.span()
                a.record()
            copy_in()
            opt.zero_grad()
            fwd_bwd()
            if world > 1:
                bucket.all_reduce()
            opt.step()
            if timed:
                b.record()

    dt = timed_region(step, args.steps // U, max(1, args.warmup // U), world, min_warm_s=0.5)      # one call = U steps
    if args.graph:
        gstep.release()
    _lin._AUTO_FUSE_STEP = auto_was
    wall_ms = dt / max(1, (args.steps // U) * U) * 1e3
    dev_ms_checked = device_step_ms(ev, U, wall_ms)
    dev_ms = dev_ms_checked if dev_ms_checked is not None else wall_ms     # (the roofline entry below falls back to the wall time)
    flops = 2.0 * 3 * Bsz * (784 * 128 + 128 * 10)
    return {
        "samples_per_step": Bsz * world, "dt": dt,
        "config": {"workload": "C1: MNIST-MLP 784->128->10 training step (Linear+ReLU+CrossEntropy+Adam), batch 32 per GPU",
                   "global_batch": Bsz * world, "parallelism": f"dp{world}",
                   "optimizer_launch": ("inside the backward launch, no opt-in (the launch waits for optimizer.step(): the default a README user gets)"
                                        if opt_mode == 2 and fused_opt else
                                        "inside the backward launch (optimizer.fuse_backward(True), opt-in)" if fused_opt
                                        else "separate fused-Adam launch (NNHIP_AUTO_FUSE_STEP=0)"),
                   "input": (f"pinned host batches copied into the device slots inside the timed region (one {U * 100.5:.0f} KB H2D copy per "
                             f"replay of {U} steps)") if feed
                            else "batches resident in HBM",
                   "launch": (f"hipGraph replay, {U} steps per graph" if U > 1 else "hipGraph replay") if args.graph else "eager"},
        "roofline": {"kernel": "whole step (3 launches: Linear+ReLU, Linear+CrossEntropy, backward+Adam; dependent-latency bound)", "bound": "mfma",
                     "achieved": round(flops / (dev_ms * 1e-3) / 1e12, 5), "peak": PEAK_F32_MFMA_TFLOPS,
                     "unit": "TFLOP/s", "frac": round(flops / (dev_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 6),
                     "traffic": None, "avg_step_device_ms": round(dev_ms_checked, 4) if dev_ms_checked is not None else None,
                     "device_ms_how": "median of HIP-event spans around sampled graph replays / steps per replay; None = the spans exceeded the wall time per step by > 5 % (host stalls inside the pairs) and were dropped"},
        "extra": {"launches_per_step": launches},
    }


def cpu_c1(seconds):
    from oracle import neunet_oracle as O
    rng = np.random.default_rng(1001)
    W1 = rng.uniform(-1 / 28, 1 / 28, (128, 784)).astype(np.float32)
    b1 = rng.uniform(-1 / 28, 1 / 28, (1, 128)).astype(np.float32)
    s2 = 1 / np.sqrt(128)
    W2 = rng.uniform(-s2, s2, (10, 128)).astype(np.float32)
    b2 = rng.uniform(-s2, s2, (1, 10)).astype(np.float32)
    st = O.MLPState(W1, b1, W2, b2, lr=1e-3)
    X = rng.uniform(-1, 1, (32, 784)).astype(np.float32)
    Y = rng.integers(0, 10, 32).astype(np.int32)
    for _ in range(3):
        st.step(X, Y)
    times, t_start = [], time.perf_counter()
    while time.perf_counter() - t_start < min(seconds, 5.0):
        t0 = time.perf_counter()
        st.step(X, Y)
        times.append(time.perf_counter() - t0)
    best = min(times)
    return {"value": round(32 / best, 1), "unit": "samples/s", "cores": blas_threads(), "kind": "port", "samples": len(times),
            "sample": f"{len(times)} C1 MLP steps via the NumPy oracle, min step {best * 1e3:.3f} ms (median {np.median(times) * 1e3:.3f} ms)"}


# ------------------------------------------------------------------------------------------------ C3
def workload_c3(args, rank, world):
    """Fused micro-bench, rows 8192 x d 4096 per GPU (BASELINE config 3: "Fused Linear-Swish + RMSNorm + Softmax +
    MultiTensorAdamW"): the fused Linear(4096->4096)->Swish forward and backward (MFMA bound), Swish, RMSNorm, Softmax
    fwd+bwd, fused CE fwd+bwd, multi-tensor AdamW on one 8192x4096 tensor -- each called through the functional C-ABI
    wrappers on pre-allocated buffers (the shape of the reference's scripts/benchmark_swish_cuda.py).  A 'step' is one
    pass over all of them; the roofline entry is the Swish forward kernel (HBM bound), per-op GB/s (TFLOP/s for the
    two GEMM ops) in `ops`."""
    import torch
    import neunet_hip
    from neunet_hip.nn import Parameter
    from neunet_hip.nn.experimental.activations import (hip_softmax_backward, hip_softmax_forward,
                                                        hip_swish_backward, hip_swish_forward)
    from neunet_hip.nn.experimental.linear_swish import hip_linear_swish_backward, hip_linear_swish_forward
    from neunet_hip.nn.experimental.losses import cross_entropy_forward_backward
    from neunet_hip.nn.experimental.rmsnorm import rmsnorm_backward, rmsnorm_forward
    from neunet_hip.optim import HIPFusedMultiTensorAdamW
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    R, D = 8192, 4096
    rng = np.random.default_rng(1003 + rank)
    Xn = rng.standard_normal((R, D)).astype(np.float32)
    x = torch.from_numpy(Xn).cuda()
    dY = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).cuda()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    logits = x.clone()
    labels = torch.from_numpy(rng.integers(0, D, R).astype(np.int32)).cuda()
    w, std, dw = torch.ones(D, device="cuda"), torch.empty(R, device="cuda"), torch.empty(D, device="cuda")
    p = Parameter(neunet_hip.Tensor(Xn, device="cuda"))
    p.grad = dY
    opt = HIPFusedMultiTensorAdamW([p], lr=1e-3, weight_decay=1e-2)
    Wl = torch.from_numpy((rng.uniform(-1, 1, (D, D)) / 64).astype(np.float32)).cuda()
    bl = torch.from_numpy((rng.uniform(-1, 1, (1, D)) / 64).astype(np.float32)).cuda()
    z, ls_out, dXl, dWl, dbl = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x), torch.empty_like(Wl), torch.empty_like(bl)
    # the many-tensor optimizer case of scripts/profile_adam.py:11-14: 200 parameters of (512, 1024), one launch
    NT, TS = 200, (512, 1024)
    g_many = torch.Generator(device="cuda").manual_seed(1003 + rank)
    many = []
    for _ in range(NT):
        q = Parameter(neunet_hip.Tensor(np.zeros(TS, np.float32), device="cuda"))
        q.data.normal_(generator=g_many)
        q.grad = torch.randn(TS, device="cuda", generator=g_many)
        many.append(q)
    opt_many = HIPFusedMultiTensorAdamW(many, lr=1e-3, weight_decay=1e-2)
    # Order matters for cold-cache timing: a kernel that follows AdamW also pays for the write-back of AdamW's
    # 402 MB of dirty lines (+12 us measured on ANY streaming kernel placed there, tools/order_check.py), so
    # AdamW goes last, the two MFMA-bound Linear->Swish ops first, and the fused CE follows a GEMM -- as it does in a
    # real step, where its predecessor is the vocabulary projection.
    ops = [
        ("linear_swish_fwd", lambda: hip_linear_swish_forward(x, Wl, bl, ls_out, z, R, D, D, 1.0, True)),
        ("linear_swish_bwd", lambda: hip_linear_swish_backward(x, Wl, bl, dY, z, dXl, dWl, dbl, R, D, D, 1.0, False)),
        ("ce_fwd_bwd", lambda: cross_entropy_forward_backward(logits, labels, "mean", -100, inplace=False)),
        ("swish_fwd", lambda: hip_swish_forward(x, y, 1.0)),
        ("swish_bwd", lambda: hip_swish_backward(dx, dY, x, 1.0)),
        ("rmsnorm_fwd", lambda: rmsnorm_forward(x, w, None, None, std, y, 1e-6)),
        ("rmsnorm_bwd", lambda: rmsnorm_backward(x, w, None, dY, dx, dw, None, None, std)),
        ("softmax_fwd", lambda: hip_softmax_forward(x, y, -1)),
        ("softmax_bwd", lambda: hip_softmax_backward(dx, dY, y, -1)),
        ("adamw_200x512x1024", lambda: opt_many.step()),
        ("adamw", lambda: opt.step()),
    ]
    timers = {k: EventTimer() for k, _ in ops}
    n = R * D
    bytes_per = {"swish_fwd": 8 * n, "swish_bwd": 12 * n, "rmsnorm_fwd": 8 * n + 4 * R + 4 * D,
                 "rmsnorm_bwd": 12 * n + 4 * R + 8 * D, "softmax_fwd": 8 * n, "softmax_bwd": 12 * n,
                 "ce_fwd_bwd": 8 * n + 12 * R, "adamw": 28 * n, "adamw_200x512x1024": 28 * NT * TS[0] * TS[1]}
    flops_per = {"linear_swish_fwd": 2.0 * R * D * D, "linear_swish_bwd": 4.0 * R * D * D}

    def step(timed):
        for k, fn in ops:
            if timed:
                a, b = timers[k].span()
                a.record()
                fn()
                b.record()
            else:
                fn()

    dt = timed_region(step, args.steps, args.warmup, world)
    # An event pair around ONE launch also spans the command processor's handling of the two event packets and the dispatch of
    # the kernel (~2-3 us): measured here as the span of a pair around a one-element kernel and subtracted, so that `ms` is the
    # kernel's duration -- the number rocprofv3 --kernel-trace reports (profiles/*_c3_kernel_stats.md); `span_ms` is the raw pair.
    # (each sample is queued behind a ~60 us kernel so that the host is ahead of the device, as it is for the timed ops: with an
    #  idle queue the span of a tiny kernel is the HOST's enqueue time -- 14 us through ctypes -- not the device's overhead)
    #  A pair around ONE tiny kernel spans overhead + that kernel (d); around TWO it spans overhead + 2 d: overhead = 2 s1 - s2.
    one = torch.zeros(4, device="cuda")
    cal1, cal2 = EventTimer(), EventTimer()
    for i in range(80):
        hip_swish_backward(dx, dY, x, 1.0)
        a, b = (cal1 if i % 2 == 0 else cal2).span()
        a.record()
        call_hip_function("nnhipScale", one, 1.0, 1, get_current_stream_ptr())
        if i % 2:
            call_hip_function("nnhipScale", one, 1.0, 1, get_current_stream_ptr())
        b.record()
    torch.cuda.synchronize()
    s1 = float(np.median([a.elapsed_time(b) for a, b in cal1.pairs[4:]]))
    s2 = float(np.median([a.elapsed_time(b) for a, b in cal2.pairs[4:]]))
    # Checked against rocprofv3's kernel durations of the same pass (profiles/r04*_c3_kernel_stats.md): the two-point estimate is ~25 %
    # high (the second tiny kernel's dispatch partly hides behind the first), so 0.75 of it is subtracted -- the conservative side.
    overhead = 0.75 * min(max(2.0 * s1 - s2, 0.0), s1)
    # PRIMARY numbers = the raw event spans (round-4 review: the subtraction was in the builder's favour every time); the span minus the
    # calibrated event overhead -- what rocprofv3 --kernel-trace reports as the kernel's duration, to ~2 % -- rides along, labelled
    kms = {k: t.mean_ms() for k, t in timers.items()}
    kcorr = {k: max(t.mean_ms() - overhead, 1e-6) for k, t in timers.items()}
    res_ops = {k: {"ms": round(kms[k], 4), "GBps": round(bytes_per[k] / (kms[k] * 1e-3) / 1e9, 1),
                   "frac_of_8TBps": round(bytes_per[k] / (kms[k] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                   "ms_minus_event_overhead": round(kcorr[k], 4),
                   "frac_of_8TBps_minus_event_overhead": round(bytes_per[k] / (kcorr[k] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                   "hbm_traffic_pmc": read_traffic(k.replace("_fwd_bwd", "") + "_c3")}
               for k, t in timers.items() if k in bytes_per}
    for k, fl in flops_per.items():
        ms = kms[k]
        res_ops[k] = {"ms": round(ms, 4), "ms_minus_event_overhead": round(kcorr[k], 4), "TFLOPs": round(fl / (ms * 1e-3) / 1e12, 2),
                      "frac_of_mfma_peak": round(fl / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                      "launches": 1 if k.endswith("fwd") else 3}
    res_ops["_event_pair_overhead_ms"] = round(overhead, 4)
    res_ops["_timing"] = "ms = mean HIP-event span around ONE launch on the launch stream (includes ~3 us of event handling); *_minus_event_overhead = the same minus a calibrated overhead"
    # The BASELINE-size buffers (128 MiB each) partly live in the 256 MiB Infinity Cache between launches: the same kernels on 512 MiB
    # buffers (rows 32768 x d 4096) are the DRAM-resident figure (round-4 review, item 5)
    try:
        Rb = 4 * R
        xb = torch.randn(Rb, D, device="cuda")
        yb, gb = torch.empty_like(xb), torch.randn(Rb, D, device="cuda")
        dxb, stdb, dwb = torch.empty_like(xb), torch.empty(Rb, device="cuda"), torch.empty(D, device="cuda")
        big_ops = [("swish_fwd", lambda: hip_swish_forward(xb, yb, 1.0), 8 * Rb * D),
                   ("swish_bwd", lambda: hip_swish_backward(dxb, gb, xb, 1.0), 12 * Rb * D),
                   ("rmsnorm_fwd", lambda: rmsnorm_forward(xb, w, None, None, stdb, yb, 1e-6), 8 * Rb * D),
                   ("rmsnorm_bwd", lambda: rmsnorm_backward(xb, w, None, gb, dxb, dwb, None, None, stdb), 12 * Rb * D)]
        bt = {k: EventTimer() for k, _, _ in big_ops}
        for it in range(8):
            for k, fn, _ in big_ops:
                if it >= 2:
                    a, b = bt[k].span()
                    a.record()
                    fn()
                    b.record()
                else:
                    fn()
        torch.cuda.synchronize()
        res_ops["dram_resident"] = {"what": f"the same kernels on rows {Rb} x d {D}: 512 MiB per buffer, nothing survives in the 256 MiB Infinity Cache",
                                    **{k: {"ms": round(bt[k].mean_ms(), 4), "GBps": round(nb / (bt[k].mean_ms() * 1e-3) / 1e9, 1),
                                           "frac_of_8TBps": round(nb / (bt[k].mean_ms() * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)} for k, _, nb in big_ops}}
        del xb, yb, gb, dxb
    except Exception as exc:  # noqa: BLE001
        res_ops["dram_resident"] = {"error": repr(exc)[:200]}
    sw = res_ops["swish_fwd"]
    return {
        "samples_per_step": R * world, "dt": dt,
        "config": {"workload": "C3: fused micro-bench rows 8192 x d 4096 per GPU (fused Linear(4096->4096)->Swish fwd+bwd, Swish, "
                               "RMSNorm, Softmax fwd+bwd, fused CrossEntropy, multi-tensor AdamW)", "global_batch": R * world,
                   "parallelism": f"dp{world}"},
        "roofline": {"kernel": "map1_kernel<SwishF> (Swish forward)", "bound": "hbm", "achieved": sw["GBps"],
                     "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": sw["frac_of_8TBps"],
                     "traffic": read_traffic("swish_fwd_c3"), "traffic_source": traffic_source(),
                     "bytes_per_launch": bytes_per["swish_fwd"],
                     "avg_launch_ms": sw["ms"]},
        "extra": {"ops": res_ops},
    }


def cpu_c3(seconds):
    from oracle import neunet_oracle as O
    R, D = 8192, 4096
    rng = np.random.default_rng(1003)
    X = rng.standard_normal((R, D)).astype(np.float32)
    dY = rng.standard_normal((R, D)).astype(np.float32)
    w = np.ones(D, np.float32)
    labels = rng.integers(0, D, R).astype(np.int32)
    P = X.copy()
    m, v = np.zeros_like(P), np.zeros_like(P)
    t0 = time.perf_counter()
    O.swish_forward(X, 1.0); O.swish_backward(X, dY, 1.0)
    O.rmsnorm_forward(X, w, None); O.rmsnorm_backward(X, w, False, dY)
    y = O.softmax_forward(X, -1); O.softmax_backward(y, dY, -1)
    O.cross_entropy_forward_backward(X, labels, ignore_index=-100, reduction="mean")
    O.adamw_step(P, dY, m, v, 1, 1e-3, (0.9, 0.999), 1e-8, 1e-2)
    dt = time.perf_counter() - t0
    return {"value": round(R / dt, 1), "unit": "samples/s", "cores": blas_threads(), "kind": "port",
            "sample": f"1 full C3 pass (all ops, 8192x4096) via the NumPy oracle: {dt:.2f} s"}


# ------------------------------------------------------------------------------------------------ C4
C4 = dict(vocab=15000, d_model=512, n_heads=8, d_ff=2048, n_layers=6, seq=256)
if os.environ.get("NNHIP_BENCH_TOY", "0") == "1":
    # functional rehearsal of the N > 1 code path (8 ranks sharing one GPU over gloo, tests/test_dp_gpu.py): same recipe, toy sizes.
    # A line produced under this switch says so in config.workload and is not a measurement of anything.
    C4 = dict(vocab=640, d_model=128, n_heads=2, d_ff=256, n_layers=2, seq=64)


def c4_flops(B, T, c=C4):
    rows, D, F, V, L, H = B * T, c["d_model"], c["d_ff"], c["vocab"], c["n_layers"], c["n_heads"]
    lin = L * (4 * 2 * rows * D * D + 2 * 2 * rows * D * F) + 2 * rows * D * V
    att = L * 2 * (2 * B * H * T * T * (D // H))
    return 3 * (lin + att)          # fwd + bwd (dX and dW GEMMs)


def c4_batch(rng, B, T, vocab):
    ids = rng.integers(3, vocab, (B, T + 1)).astype(np.int32)
    for r in rng.choice(B, max(1, B // 10), replace=False):     # ~10 % of rows PAD-tailed
        ids[r, -int(rng.integers(8, T // 4)):] = 0
    return ids


def workload_c4(args, rank, world):
    """BASELINE C4: GPT-tiny (d_model 512, 6 layers, 8 heads, d_ff 2048, vocab 15000) training step on
    batch 64 x seq 256 per GPU: embedding -> 6 x [RMSNorm, attention, RMSNorm, FFN] -> vocab projection ->
    CrossEntropy(ignore PAD) -> backward -> gradient exchange -> fused Adam (lr 1.5e-4, betas .9/.98, eps 1e-9).
    N > 1: every rank back-propagates the SUM loss; the count of non-PAD targets is written by a kernel into the extra
    slot of the gradient bucket, all-reduced with the gradients, and the optimizer divides by it on load
    (grad_divisor) -- the global mean without a host read or a scale pass.  The bucket is cut into segments whose
    all-reduces (RCCL, own stream) overlap the rest of the backward pass; under hipGraph replay the backward pass is
    one graph per segment."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import gpt_tiny
    import neunet_hip
    import neunet_hip.nn as nn
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    from neunet_hip.distributed import collectives_live
    strong = getattr(args, "scaling", "weak") == "strong"
    T = C4["seq"]
    if strong:
        # the global batch divided over the ranks; a remainder goes to the first ranks (distributed.shard_batch): every rank
        # back-propagates the SUM loss of its own shard and the all-reduced target count divides, so uneven shards are exact
        from neunet_hip.distributed import shard_batch
        if args.c4_batch < world:
            raise ValueError(f"--scaling strong: the global batch ({args.c4_batch}) has fewer sequences than ranks ({world})")
        lo, hi = shard_batch(args.c4_batch, rank, world)
        B = hi - lo
    else:
        B = args.c4_batch
    global_batch = args.c4_batch if strong else B * world
    dp = world > 1 or collectives_live()                          # a gradient exchange is part of the step
    comm = None
    if dp and getattr(args, "comm", "torch") == "native":
        # the exchange through the library's own RCCL entry points (include/neunet_hip.h, ABI 208) instead of ProcessGroupNCCL
        from neunet_hip.distributed import NativeComm
        comm = NativeComm.from_env()
    np.random.seed(1004)                                          # identical init on every rank
    model = gpt_tiny.build_gpt(C4["vocab"], C4["d_model"], C4["n_heads"], C4["d_ff"], C4["n_layers"], pad_idx=0,
                               max_len=1024, fused=True)
    params = model.parameters()
    opt = Adam(params, lr=1.5e-4, betas=(0.9, 0.98), eps=1e-9)
    batch = c4_batch(np.random.default_rng(4000 + rank), B, T, C4["vocab"])
    ids = neunet_hip.Tensor(np.ascontiguousarray(batch[:, :-1]), dtype=np.int32, requires_grad=False, device="cuda")
    tgt_host = np.ascontiguousarray(batch[:, 1:]).reshape(-1)
    tgt = neunet_hip.Tensor(tgt_host, dtype=np.int32, requires_grad=False, device="cuda")
    loss_fn = nn.CrossEntropyLoss(ignore_index=0, reduction="sum" if dp else "mean")
    ev = EventTimer()
    state = {"bucket": None}

    def fwd_bwd():
        out, _ = model.forward(ids)
        out = out.reshape(out.shape[0] * out.shape[1], out.shape[2])
        loss = loss_fn(out, tgt)
        bk = state["bucket"]
        if dp and bk is not None:           # this rank's non-PAD count -> the bucket's extra slot (device side)
            call_hip_function("nnhipCrossEntropyDenominator", tgt.data, 4, tgt.data.numel(), 0, None, C4["vocab"], None,
                              bk.extra, get_current_stream_ptr())
        loss.backward()
        return loss

    # one throw-away step discovers which parameters receive gradients (cross_attn never does)
    fwd_bwd()
    active = [p for p in params if p.grad is not None]
    opt.zero_grad()
    overlap = dp and bool(args.overlap) and os.environ.get("NNHIP_DP_OVERLAP", "1") != "0"

    def make(overlap, use_graph, ingraph=False):
        """Bucket + step function for one exchange / launch mode, exercised once."""
        opt.zero_grad()
        bucket = GradBucket(active, extra_scalars=1, overlap=overlap, reduce_op=args.dp_op, comm=comm)
        state["bucket"] = bucket
        if dp:
            opt.grad_divisor = bucket.extra              # g / (all-reduced non-PAD count), inside the Adam kernel
        gstep = None
        if use_graph:
            gstep = GraphedTrainStep(fwd_bwd, opt, bucket, warmup=2, world=world, capture_collectives=ingraph)

            def step(timed):
                if timed:
                    a, b = ev.span()
                    a.record()
                state["loss"] = gstep()
                if timed:
                    b.record()
        else:
            def step(timed):
                if timed:
                    a, b = ev.span()
                    a.record()
                opt.zero_grad()
                state["loss"] = fwd_bwd()
                bucket.all_reduce()
                opt.step()
                if timed:
                    b.record()
        try:
            step(False)
            torch.cuda.synchronize()
        except Exception:
            if gstep is not None:
                gstep.release()
            raise
        return step, gstep, bucket

    # N > 1 has only ever run on gloo here (one GPU per box): if RCCL refuses the overlapped / captured exchange, fall back
    # to the plainer modes instead of losing the measurement (every rank takes the same path: the failure modes are
    # structural, not data-dependent).  N = 1 takes the first mode.
    modes = [(overlap, bool(args.graph), False)]
    if dp:
        if args.dp_ingraph and args.graph:
            modes.insert(0, (overlap, True, True))
        modes += [(False, bool(args.graph), False), (False, False, False)]
    step = gstep = bucket = None
    tried = []
    for i, (ov, gr, ig) in enumerate(modes):
        try:
            step, gstep, bucket = make(ov, gr, ig)
            overlap, args_graph = ov, gr
            break
        except Exception as exc:  # noqa: BLE001
            if i + 1 == len(modes):
                raise
            tried.append(f"overlap={ov} graph={gr} ingraph={ig}: {exc!r}"[:200])
            print(f"[bench] C4 step with overlap={ov} graph={gr} ingraph={ig} failed ({exc!r}); trying the next mode",
                  file=sys.stderr)
    use_graph = args_graph
    graph_mode = getattr(gstep, "mode", None) if use_graph else None
    ingraph_error = getattr(gstep, "ingraph_error", None) if use_graph else None

    dt = timed_region(step, args.steps, args.warmup, world)
    dev_ms = ev.median_ms()
    if getattr(args, "dump_outputs", None) and rank == 0:
        dump_outputs(args.dump_outputs, c4_step_outputs(model, state["loss"], active))
    # ---- the gradient exchange on its own (SURVEY 8e "report all-reduce time separately"; round-5 review item 4), --full only ------
    #   total   = every all-reduce of one step issued ALONE, event-bracketed on the stream it runs on, summed (median of 5 each)
    #   exposed = (the timed step) - (the same step, same launch mode, with the collectives muted): what the exchange adds to the
    #             step after overlap; None when the collectives are captured inside the step graph (they cannot be muted there)
    allreduce = None
    if dp and getattr(args, "full", False):
        try:
            pieces_ms = bucket.time_exchange_alone(5)
            exposed, dt_muted = None, None
            if not (use_graph and graph_mode == "ingraph"):
                bucket.mute = True
                try:
                    dt_muted = timed_region(step, args.steps, max(1, args.warmup // 2), world)
                finally:
                    bucket.mute = False
                exposed = max(0.0, (dt - dt_muted) / args.steps * 1e3)
            allreduce = {"total": round(sum(ms for _, ms in pieces_ms), 4), "exposed": None if exposed is None else round(exposed, 4),
                         "pieces": [{"floats": n, "ms_alone": round(ms, 4), "GBps_algorithmic": round(4.0 * n / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
                                    for n, ms in pieces_ms],
                         "ms_per_step_with_exchange": round(dt / args.steps * 1e3, 4),
                         "ms_per_step_collectives_muted": None if dt_muted is None else round(dt_muted / args.steps * 1e3, 4),
                         "how": "total: each all-reduce of a step issued on its own between two HIP events (median of 5), summed; exposed: timed step minus "
                                "the same K steps with GradBucket.mute (no collective issued), max over ranks both times; DESIGN 6 expects 0.25 ms "
                                "(direct, 7 xGMI links) to 1.6 ms (one-link ring) total for the 137 MB bucket at N = 8"}
        except Exception as exc:  # noqa: BLE001
            allreduce = {"error": repr(exc)[:300]}
    fl = c4_flops(B, T)
    ach = fl / (dev_ms * 1e-3) / 1e12
    n_grad = sum(int(np.prod(p.shape)) for p in active)
    pieces = len(getattr(gstep, "pieces", [])) if use_graph else 0
    if use_graph:
        gstep.release()
    comm_lib = None
    if comm is not None:
        from neunet_hip.distributed import NativeComm
        comm_lib = "%s (version %d)" % NativeComm.library()
        comm.destroy()
    return {
        "samples_per_step": global_batch, "dt": dt, "scaling": "strong" if strong else "weak",
        "config": {"workload": ("TOY SIZES (NNHIP_BENCH_TOY=1, functional rehearsal only) " if os.environ.get("NNHIP_BENCH_TOY", "0") == "1" else "")
                               + f"C4: GPT-tiny d{C4['d_model']} L{C4['n_layers']} H{C4['n_heads']} d_ff{C4['d_ff']} vocab{C4['vocab']} training step, "
                               f"batch {B} x seq {T} per GPU, Adam(1.5e-4), dropout 0", "global_batch": global_batch, "seq_len": T,
                   "parallelism": f"dp{world}", "launch": "hipGraph replay" if use_graph else "eager",
                   "scaling": ("strong: global batch %d divided over the ranks" % global_batch) if strong
                              else "weak: %d sequences per GPU" % B},
        "roofline": {"kernel": "whole step, GEMM flops only (fp32 MFMA gemm_f32_kernel family: Linear fwd/dX/dW + attention)",
                     "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4), "traffic": None, "flops_per_step": fl,
                     "avg_step_device_ms": round(dev_ms, 4)},
        "extra": {"tokens_per_s": round(global_batch * T * args.steps / dt, 1), "grad_floats": n_grad, "allreduce_ms": allreduce,
                  "dp_exchange": ("none" if not dp else
                                  (f"{len(bucket.segments)} bucket segments, async all-reduce overlapped with backward"
                                   + (f" ({pieces} graph pieces)" if use_graph else "") if overlap
                                   else "one blocking all-reduce of the flat bucket")),
                  "dp_mode": ({"forced_one_rank": world == 1, "overlap": bool(overlap), "launch": graph_mode or "eager",
                               "ingraph_error": ingraph_error, "modes_that_failed": tried, "reduce_op": args.dp_op,
                               "comm": ("nnhipAllReduce*F32 over " + comm_lib) if comm_lib else "torch.distributed"} if dp else None)},
    }


def cpu_c4(seconds, Bs=64, max_steps=1):
    """ONE FULL GPT-tiny training step (forward, backward, Adam on every parameter that has a gradient) of the NumPy oracle
    on the WHOLE per-GPU batch, 64 sequences x 256 tokens: ~18 s on the GPU box's host (profiles/cpu_c4_full_batch.json;
    rounds 1-2 timed 2 sequences, which understated OpenBLAS by 1.7x -- 2.0 vs 3.5 samples/s).  `--cpu-seconds` below 12
    falls back to that 2-sequence sample (3 steps)."""
    if seconds < 12.0 and Bs == 64:
        Bs, max_steps = 2, 3
    from oracle import neunet_oracle as O
    c = C4
    rng = np.random.default_rng(1004)
    D, F, V, L = c["d_model"], c["d_ff"], c["vocab"], c["n_layers"]
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1]))  # noqa: E731
    layers = [{"attn": [u(D, D), u(1, D), u(D, D), u(1, D), u(D, D), u(1, D), u(D, D), u(1, D)],
               "ffn": [u(F, D), u(1, F), u(D, F), u(1, D)], "norm1": np.ones(D, np.float32), "norm2": np.ones(D, np.float32)}
              for _ in range(L)]
    model = O.GPTTiny(rng.standard_normal((V, D)).astype(np.float32), layers, u(V, D), u(1, V), c["n_heads"], 0, 1024)
    batch = c4_batch(rng, Bs, c["seq"], V)

    def flat_params(m):
        ps = [m.emb]
        for Ly in m.layers:
            ps += Ly["attn"] + Ly["ffn"] + [Ly["norm1"], Ly["norm2"]]
        return ps + [m.Wout, m.bout]

    def flat_grads(g):
        gs = [g["emb"]]
        for Ly in g["layers"]:
            gs += Ly["attn"] + Ly["ffn"] + [Ly["norm1"], Ly["norm2"]]
        return gs + [g["Wout"], g["bout"]]

    ps = flat_params(model)
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    times = []
    t_all = time.perf_counter()
    for step in range(1, max_steps + 1):
        t0 = time.perf_counter()
        _, _, grads = model.forward_backward(batch[:, :-1], batch[:, 1:])
        for i, (p_, g_) in enumerate(zip(ps, flat_grads(grads))):
            ms[i], vs[i] = O.adam_step(p_, g_.reshape(p_.shape), ms[i], vs[i], step, 1.5e-4, (0.9, 0.98), 1e-9, 0.0)
        times.append(time.perf_counter() - t0)
        if time.perf_counter() - t_all > max(seconds, 10.0):
            break
    best = min(times)
    out = {"value": round(Bs / best, 3), "unit": "samples/s", "cores": blas_threads(), "kind": "port", "samples": len(times),
           "step_seconds_all": [round(t, 2) for t in times],
           "sample": f"n = {len(times)} (one full-batch oracle step is 10-20 s of host time: the bounded sample of the default run) -- {len(times)} FULL steps (forward + backward + Adam over all {sum(p.size for p in ps)} parameters) of the "
                     f"NumPy-oracle GPT-tiny on {Bs} sequences x {c['seq']} tokens ({Bs}/64 of one GPU's batch), min step "
                     f"{best:.2f} s, OpenBLAS threads={blas_threads()}, host cpus={os.cpu_count()}"}
    full = os.path.join(ROOT, "profiles", "cpu_c4_full_batch.json")
    if Bs != 64 and os.path.exists(full):
        try:
            fb = json.load(open(full))
            out["full_batch_reference"] = {k: fb[k] for k in ("value", "step_seconds", "cores", "collected") if k in fb}
            out["sample"] += (f"; ONE full-batch step (64 x 256) timed once on a box of this pool: {fb['step_seconds']:.1f} s = "
                              f"{fb['value']:.2f} samples/s ({fb.get('collected', '?')})")
        except Exception:
            pass
    else:
        out["step_seconds"] = round(best, 2)
        if os.path.exists(full) and max_steps == 1:
            # the live sample of a default run is ONE full step (10-20 s of host time is the bound of the contract); the n >= 3
            # collection of the SAME function on a box of this pool rides along so that the figure has something to be averaged
            # against (round-5 review: 18.52 s vs 19.10 s with nothing to average)
            try:
                fb = json.load(open(full))
                keep = ("value", "step_seconds", "step_seconds_all", "samples", "cores", "collected")
                out["full_batch_collection"] = {**{k: fb[k] for k in keep if k in fb},
                                                "source": "profiles/cpu_c4_full_batch.json (python bench.py --cpu-full-batch --cpu-full-steps 3 on a GPU box's host; not measured by this run)"}
                out["sample"] = "live: " + out["sample"] + f"; cached collection of the same step, n = {fb.get('samples', 1)}: " + \
                                ", ".join(f"{t:.2f}" for t in fb.get("step_seconds_all", [fb.get("step_seconds", float('nan'))])) + " s (profiles/cpu_c4_full_batch.json)"
            except Exception:
                pass
    return out


# ------------------------------------------------------------------------------------------------ notebook GPT
NB = dict(vocab=15000, d_model=512, n_heads=8, d_ff=2048, n_layers=8, batch=4, dropout=0.1)
NB_REFERENCE_IT_PER_S = (6.44, 6.67)     # examples/gpt.ipynb cell 16 output (tqdm, epochs 12-14), hardware unstated


def nb_batches(rng, n, B, vocab):
    """Batches shaped like the notebook's (cell 10): B prompts tokenised to <sos> ... <eos>, padded to the longest of the
    batch with PAD = 0 -- a different length every step."""
    out = []
    for _ in range(n):
        lens = rng.integers(24, 128, B)
        T = int(lens.max())
        ids = np.zeros((B, T), np.int32)
        for r, L in enumerate(lens):
            ids[r, :L] = rng.integers(3, vocab, L)
            ids[r, 0], ids[r, L - 1] = 1, 2
        out.append(ids)
    return out


def workload_nb(args, rank, world):
    """The reference's ONLY published training throughput: examples/gpt.ipynb's GPT (d512, 8 layers, 8 heads, d_ff 2048,
    vocab 15000, dropout 0.1, Adam 1.5e-4) on batches of 4 variable-length prompts, 6.44-6.67 it/s in the notebook's own
    tqdm output (cell 16; CuPy on an unnamed NVIDIA GPU).  Same model and loop body (cell 12) on the HIP path, device-side
    dropout masks; every batch has its own length, so the step is captured once per padded length (`--graph 0`: eager)."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import gpt_tiny
    import neunet_hip.nn as nn
    from neunet_hip.optim import Adam
    c = NB
    np.random.seed(1006)
    model = gpt_tiny.build_gpt(c["vocab"], c["d_model"], c["n_heads"], c["d_ff"], c["n_layers"], pad_idx=0, max_len=1024,
                               fused=True, dropout=c["dropout"])
    opt = Adam(model.parameters(), lr=1.5e-4, betas=(0.9, 0.98), eps=1e-9)
    loss_fn = nn.CrossEntropyLoss(ignore_index=0)
    steps = max(args.steps, 100)
    batches = nb_batches(np.random.default_rng(6000 + rank), 64, c["batch"], c["vocab"])
    it = [0]
    bucket = None
    from neunet_hip.distributed import GradBucket, collectives_live
    from neunet_hip.graph import GraphedTrainStep, attach_step_seed
    dp = world > 1 or collectives_live()
    use_graph = bool(args.graph) and not dp
    if dp:
        # data parallel: every rank its own 4 prompts, one all-reduce of the flat gradient bucket per step, mean over ranks
        # folded into the optimizer's gradient load (each rank's 'mean' loss is over its own tokens, as in the notebook)
        bucket = GradBucket([p for p in model.parameters()])
        opt.grad_scale = 1.0 / world

    def step_eager(timed):
        gpt_tiny.train_step(model, opt, loss_fn, batches[it[0] % len(batches)], bucket=bucket)
        it[0] += 1

    graphs = {}
    if use_graph:
        # One captured step per padded length.  A batch is padded to the next multiple of 8 columns with PAD = 0: padded keys
        # are masked in the attention, padded targets ignored by the loss, so every real token sees the same arithmetic as in
        # the notebook's pad-to-the-longest batch; the static id / target buffers are refilled before each replay (the host
        # batch crosses PCIe every step, as in the notebook's loop), dropout masks come from the device step seed.
        import neunet_hip
        step_seed = attach_step_seed(model)
        B = c["batch"]
        active = None

        def build(Tp):
            nonlocal active
            ids = neunet_hip.Tensor(np.zeros((B, Tp), np.int32), dtype=np.int32, requires_grad=False, device="cuda")
            tgt = neunet_hip.Tensor(np.zeros(B * Tp, np.int32), dtype=np.int32, requires_grad=False, device="cuda")
            ids.data[:, 0] = 1
            ids.data[:, 1] = 5
            tgt.data[0] = 5                                          # a valid token so that the warm-up loss is finite

            def fb():
                out, _ = model.forward(ids)
                loss = loss_fn(out.reshape(B * Tp, c["vocab"]), tgt)
                loss.backward()
                return loss

            if active is None:
                fb()
                active = [p for p in model.parameters() if p.grad is not None]
                opt.zero_grad()
                graphs["bucket"] = GradBucket(active)
            g = GraphedTrainStep(fb, opt, graphs["bucket"], warmup=1, step_seed=step_seed)
            return g, ids, tgt

        def padded(b):
            T = b.shape[1] - 1
            Tp = (T + 7) // 8 * 8
            x = np.zeros((b.shape[0], Tp), np.int32)
            y = np.zeros((b.shape[0], Tp), np.int32)
            x[:, :T], y[:, :T] = b[:, :-1], b[:, 1:]
            return Tp, x, y.reshape(-1)

        for b in batches:                                             # capture every length in the data before the clock starts
            Tp = padded(b)[0]
            if Tp not in graphs:
                graphs[Tp] = build(Tp)

    def step_graph(timed):
        Tp, x, y = padded(batches[it[0] % len(batches)])
        g, ids, tgt = graphs[Tp]
        ids.data.copy_(torch.from_numpy(x), non_blocking=True)
        tgt.data.copy_(torch.from_numpy(y), non_blocking=True)
        g()
        it[0] += 1

    eager_ips = None
    if use_graph:
        dte = timed_region(step_eager, 40, 5, world)
        eager_ips = 40 / dte
    step = step_graph if use_graph else step_eager
    dt = timed_region(step, steps, max(args.warmup, 10), world)
    for k, v in graphs.items():
        if isinstance(k, int):
            v[0].release()
    ips = steps / dt
    tokens = float(np.mean([b.shape[0] * (b.shape[1] - 1) for b in batches]))
    return {
        "samples_per_step": c["batch"] * world, "dt": dt * args.steps / steps,     # main() divides by args.steps
        "config": {"workload": "examples/gpt.ipynb GPT (d512 L8 H8 d_ff2048 vocab15000, dropout 0.1, Adam 1.5e-4), batch 4 "
                               "variable-length prompts (24-127 tokens, padded to the batch maximum)"
                               + (", one captured hipGraph per padded length (multiples of 8)" if use_graph else ", eager launches"),
                   "global_batch": c["batch"] * world, "parallelism": f"dp{world}",
                   "launch": f"hipGraph replay, {len([k for k in graphs if isinstance(k, int)])} length buckets" if use_graph else "eager"},
        "roofline": {"kernel": "whole step (launch bound: ~" + str(int(tokens)) + " tokens per step)", "bound": "mfma",
                     "achieved": None, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": None, "traffic": None},
        "extra": {"it_per_s": round(ips, 2), "it_per_s_eager": None if eager_ips is None else round(eager_ips, 2),
                  "timed_steps": steps, "mean_tokens_per_step": round(tokens, 1),
                  "reference_it_per_s": list(NB_REFERENCE_IT_PER_S),
                  "vs_reference_notebook": round(ips / NB_REFERENCE_IT_PER_S[1], 1),
                  "reference_note": "examples/gpt.ipynb cell 16 (tqdm it/s of the CuPy path on an unnamed NVIDIA GPU, real "
                                    "prompts): different hardware and data, same model / batch size / optimizer"},
    }


def cpu_nb(seconds):
    return cpu_c4(seconds)


# ------------------------------------------------------------------------------------------------ C5
def workload_c5(args, rank, world):
    """BASELINE C5: Conv2d MNIST classifier (examples/convolutional_digits_classifier.ipynb) training step,
    28x28x1, batch 256 per GPU: conv(1->8) LeakyReLU MaxPool conv(8->16) LeakyReLU MaxPool BatchNorm2d Linear Sigmoid,
    MSE, Adam(1e-3).  BatchNorm statistics are per replica under DP."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import conv_classifier
    import neunet_hip
    import neunet_hip.nn as nn
    from neunet_hip.distributed import GradBucket
    from neunet_hip.graph import GraphedTrainStep
    from neunet_hip.optim import Adam
    Bsz = 256
    np.random.seed(1005)
    model = conv_classifier.Conv2dClassifier()
    params = model.parameters()
    bucket = GradBucket(params)
    opt = Adam(params, lr=1e-3)
    opt.grad_scale = 1.0 / world
    rng = np.random.default_rng(5000 + rank)
    U = graph_unroll(args, world)                        # steps per captured graph, each reading its own static batch slot
    Xs = [neunet_hip.Tensor(rng.uniform(-1, 1, (Bsz, 1, 28, 28)).astype(np.float32), device="cuda", requires_grad=False) for _ in range(U)]
    Ts = [neunet_hip.Tensor(np.eye(10, dtype=np.float32)[rng.integers(0, 10, Bsz)], device="cuda", requires_grad=False)
          for _ in range(U)]
    loss_fn = nn.MSELoss()
    ev = EventTimer()
    launches = None

    def fwd_bwd(k=0):
        loss = loss_fn(model(Xs[k]), Ts[k])
        loss.backward()
        return loss

    if args.graph:
        gstep = GraphedTrainStep(fwd_bwd, opt, bucket, warmup=3, world=world, unroll=U, count_nodes=True)
        if gstep.kernel_nodes:
            launches = round(gstep.kernel_nodes / U, 2)
        tick = [0]
        n_calls = max(1, args.steps // U)
        every = 16 if n_calls >= 64 else max(1, n_calls // 4)      # short runs: still a few device-time samples

        def step(timed):
            # the device-time events go around every 16th step only: at ~0.06 ms per step two event records per step are a
            # measurable part of what they measure (host time and two more device-side nodes between the graph launches)
            tick[0] += 1
            sample = timed and tick[0] % every == 0
            if sample:
                a, b = ev.span()
                a.record()
            gstep()
            if sample:
                b.record()
    else:
        def step(timed):
            if timed:
                a, b = ev.span()
                a.record()
            opt.zero_grad()
            fwd_bwd()
            bucket.all_reduce()
            opt.step()
            if timed:
                b.record()

    dt = timed_region(step, args.steps // U, max(1, args.warmup // U), world, min_warm_s=0.5)      # one call = U steps
    if args.graph:
        gstep.release()
    wall_ms = dt / max(1, (args.steps // U) * U) * 1e3
    dev_ms_checked = device_step_ms(ev, U, wall_ms)
    dev_ms = dev_ms_checked if dev_ms_checked is not None else wall_ms
    conv_layers = c5_conv_layers(Bsz) if (rank == 0 or world == 1) else None
    # algorithmic HBM bytes of the two conv layers fwd + bwd: 4*(|X|+|O|+|W|) forward, x2 backward
    conv_bytes = 3 * 4.0 * ((Bsz * 784 + Bsz * 8 * 784 + 72) + (Bsz * 8 * 196 + Bsz * 16 * 196 + 1152))
    return {
        "samples_per_step": Bsz * world, "dt": dt,
        "config": {"workload": "C5: Conv2d MNIST classifier training step (conv-LeakyReLU-MaxPool x2, BatchNorm2d, Linear, "
                               "Sigmoid, MSE, Adam), 28x28x1, batch 256 per GPU; at these shapes (Cin, Cout <= 16, 3x3) the DIRECT conv kernels run "
                               "(conv + LeakyReLU + MaxPool forward as one kernel per layer, conv_direct_dgrad_quad / conv_mfma_wgrad backward), "
                               "not the implicit-GEMM MFMA ones",
                   "global_batch": Bsz * world, "parallelism": f"dp{world}",
                   "launch": (f"hipGraph replay, {U} steps per graph" if U > 1 else "hipGraph replay") if args.graph else "eager"},
        "roofline": {"kernel": "whole step vs the conv layers' algorithmic HBM bytes (K<=72, Cout<=16: HBM/latency bound)",
                     "bound": "hbm", "achieved": round(conv_bytes / (dev_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS,
                     "unit": "GB/s", "frac": round(conv_bytes / (dev_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 5), "traffic": None,
                     "avg_step_device_ms": round(dev_ms_checked, 4) if dev_ms_checked is not None else None},
        "extra": {"launches_per_step": launches, "conv_layers": conv_layers,
                  "bound_by": "dependent latency, not launch count and not bytes: 13 launches x ~5 us of first-load / reduction / store-drain chain each "
                              "+ ~1.5 us per boundary inside the 16-step graph.  Two negative results close the launch-count route (EXPERIMENTS.md, round 5): "
                              "the tail (BatchNorm + Linear + Sigmoid + MSE) as ONE launch with a ticket hand-off between channel blocks was slower "
                              "(0.0852 -> 0.0952 ms), and without any hand-off it is 11 launches at 0.0864 vs 0.0853 ms (kept as the tested opt-in "
                              "NNHIP_BN_HEAD_FUSION=1, reported under tail_one_launch_opt_in).  No further kernel work is planned unless a change shows <= 0.075 ms"},
    }


def c5_conv_layers(Bsz, iters=30):
    """The two conv layers of C5 on their own through the plain C-ABI entries (nnhipConv2dForward / nnhipConv2dBackward with dX,
    dW, db), median of HIP-event timed launches: algorithmic bytes 4(|X|+|O|+|W|) forward, 4(|dO|+|X|+|W|+|dX|+|dW|) backward
    against the 8 TB/s HBM peak (K <= 72, Cout <= 16 can never be MFMA bound).  The training step itself runs fused
    variants of these (conv + LeakyReLU + MaxPool forward, weight gradient off the pool's gradient)."""
    import ctypes
    import torch
    from neunet_hip._lib import Conv2dDesc, call_hip_function as call, get_current_stream_ptr
    st = get_current_stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(5)
    out = []
    for name, (Cin, H, Cout) in (("conv1 1->8 28x28", (1, 28, 8)), ("conv2 8->16 14x14", (8, 14, 16))):
        d = Conv2dDesc(Bsz, Cin, H, H, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
        X = torch.rand(Bsz, Cin, H, H, device="cuda", generator=g) * 2 - 1
        W = (torch.rand(Cout, Cin, 3, 3, device="cuda", generator=g) * 2 - 1) / 3
        b = torch.zeros(Cout, device="cuda")
        O_ = torch.empty(Bsz, Cout, H, H, device="cuda")
        dO = torch.rand(Bsz, Cout, H, H, device="cuda", generator=g) * 2 - 1
        dX, dW, db = torch.empty_like(X), torch.empty_like(W), torch.empty_like(b)

        def med(fn):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            ev = []
            for _ in range(iters):
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                e.record()
                ev.append((a, e))
            torch.cuda.synchronize()
            return float(np.median([a.elapsed_time(e) for a, e in ev]))

        tf = med(lambda: call("nnhipConv2dForward", X, W, b, O_, ctypes.byref(d), st))
        tb = med(lambda: call("nnhipConv2dBackward", X, W, dO, dX, dW, db, ctypes.byref(d), st))
        bf = 4.0 * (X.numel() + O_.numel() + W.numel())
        bb = 4.0 * (dO.numel() + X.numel() + W.numel() + dX.numel() + dW.numel())
        fl = 2.0 * Bsz * H * H * Cout * Cin * 9
        out.append({"layer": name, "fwd_ms": round(tf, 4), "bwd_ms": round(tb, 4),
                    "fwd_frac_of_hbm_peak": round(bf / (tf * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                    "bwd_frac_of_hbm_peak": round(bb / (tb * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                    "fwd_gflops": round(fl / (tf * 1e-3) / 1e9, 1), "bwd_gflops": round(2 * fl / (tb * 1e-3) / 1e9, 1)})
    return out


def cpu_c5(seconds):
    from oracle import neunet_oracle as O
    rng = np.random.default_rng(1005)
    u = lambda s, fan: rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(fan))  # noqa: E731
    params = [u((8, 1, 3, 3), 9), np.zeros(8, np.float32), u((16, 8, 3, 3), 72), np.zeros(16, np.float32),
              np.ones((1, 16), np.float32), np.zeros((1, 16), np.float32), u((10, 784), 784), u((1, 10), 784)]
    model = O.ConvClassifier(params)
    X = rng.uniform(-1, 1, (256, 1, 28, 28)).astype(np.float32)
    Tt = np.eye(10, dtype=np.float32)[rng.integers(0, 10, 256)]
    ms, vs = [np.zeros_like(q) for q in model.p], [np.zeros_like(q) for q in model.p]
    t = [0]

    def step():
        # forward + backward + Adam(1e-3) on all eight parameter tensors (neunet/optim.py:17-33): the whole training step
        _, _, grads = model.forward_backward(X, Tt)
        t[0] += 1
        for i, g in enumerate(grads):
            ms[i], vs[i] = O.adam_step(model.p[i], np.asarray(g, np.float32).reshape(model.p[i].shape), ms[i], vs[i], t[0], 1e-3)

    step()
    times, t0 = [], time.perf_counter()
    while (time.perf_counter() - t0 < min(seconds, 10.0) and len(times) < 20) or len(times) < 3:
        t1 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t1)
    best = min(times)
    return {"value": round(256 / best, 1), "unit": "samples/s", "cores": blas_threads(), "kind": "port", "samples": len(times),
            "sample": f"{len(times)} FULL training steps (forward + backward + Adam on all 8 parameter tensors) of the "
                      f"NumPy-oracle conv classifier at batch 256, min {best * 1e3:.1f} ms"}


def blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
    except Exception:
        return os.cpu_count() or 1


# ------------------------------------------------------------------------------------------------ headline
def c2_forward_roofline(iters=50, sustain_s=2.0):
    """The metric's "Linear fwd GFLOP/s vs MFMA peak" half: Linear(4096->4096) forward on a 4096-row batch, `iters`
    launches each bracketed by a HIP-event pair on the launch stream (burst figure = what the roofline object reports),
    then a >= `sustain_s` seconds back-to-back loop with one event pair around it (sustained clocks)."""
    import torch
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    n = 4096
    g = torch.Generator(device="cuda").manual_seed(1002)
    X = torch.rand(n, n, device="cuda", generator=g) * 2 - 1
    W = (torch.rand(n, n, device="cuda", generator=g) * 2 - 1) / 64
    b = (torch.rand(n, device="cuda", generator=g) * 2 - 1) / 64
    O_ = torch.empty(n, n, device="cuda")
    st = get_current_stream_ptr()

    def fwd():
        call_hip_function("nnhipLinearModuleForward", X, W, b, O_, n, n, n, st)

    for _ in range(10):
        fwd()
    torch.cuda.synchronize()
    t = EventTimer()
    for _ in range(iters):
        a, e = t.span()
        a.record()
        fwd()
        e.record()
    torch.cuda.synchronize()
    burst_ms = t.mean_ms()
    # sustained: calibrate the count from the burst time, one event pair around the whole loop
    reps = max(100, int(sustain_s * 1e3 / burst_ms))
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fwd()
    e.record()
    torch.cuda.synchronize()
    sus_ms = a.elapsed_time(e) / reps
    flops = 2.0 * n * n * n
    return {"flops": flops, "burst_ms": burst_ms, "sustained_ms": sus_ms, "sustained_launches": reps,
            "burst_tflops": flops / (burst_ms * 1e-3) / 1e12, "sustained_tflops": flops / (sus_ms * 1e-3) / 1e12}


def c4_family_rooflines(iters=20):
    """Every GEMM / attention launch of ONE C4 step at its own shape, launched on its own and timed with HIP events (median of
    `iters`): the q|k|v projection, the output projection, the two FFN layers, the vocabulary head (forward and input gradient
    each), the deferred parameter gradients of a decoder layer as the ONE grouped launch the step makes of them, and the fused
    attention.  `per_step` = how many times the step launches it.  The flop-weighted sum over this list is the headline's
    roofline figure (workload_headline)."""
    import torch
    from neunet_hip._lib import StridedView, call_hip_function as call, get_current_stream_ptr
    st = get_current_stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *sh: torch.rand(*sh, device="cuda", generator=g) * 2 - 1  # noqa: E731

    def med(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in ev]))

    M, D, F, V, Bq, T, H, L = 64 * C4["seq"], C4["d_model"], C4["d_ff"], C4["vocab"], 64, C4["seq"], C4["n_heads"], C4["n_layers"]
    fams = []

    instep = read_instep()

    def add(name, kernels, per_step, fl, ms, key=None):
        f = {"family": name, "kernels": kernels, "per_step": per_step, "flops": fl, "ms": round(ms, 4),
             "tflops": round(fl / (ms * 1e-3) / 1e12, 2), "frac_of_mfma_peak": round(fl / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)}
        # the same kernel(s) INSIDE the replayed step, from the committed rocprofv3 kernel trace (profiles/c4_instep_families.json,
        # tools/c4_instep.py): back to back with the rest of the step the launches are a few per cent slower than on their own
        us = sum(instep[k]["us"] for k in (key or ()) if k in instep) if key and all(k in instep for k in key) else None
        if us:
            f["instep_ms"] = round(us * 1e-3, 4)
            f["instep_frac_of_mfma_peak"] = round(fl / (us * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
        fams.append(f)

    def linear_fwd_dx(name, K, N, per_step, with_dw=False, keys=(None, None, None), swish=None):
        """swish = "fwd": the forward is the fused Linear->Swish with z saved (what the step launches for fc_1); swish = "dx": the
        input gradient carries the Swish backward of the PREVIOUS layer in its epilogue, in place over z (fc_2's dX)."""
        X, W, b = rnd(M, K), rnd(N, K) / 16, rnd(1, N)
        O_, dO, dX = torch.empty(M, N, device="cuda"), rnd(M, N), torch.empty(M, K, device="cuda")
        fl = 2.0 * M * K * N
        if swish == "fwd":
            Z = torch.empty(M, N, device="cuda")
            add(f"{name}: forward + Swish (swish'(z) saved for the backward pass), rows {M}", "gemm_pst_kernel<3> (Swish epilogue, two outputs)", per_step, fl,
                med(lambda: call("nnhipLinearSwishForward", X, W, b, O_, Z, M, K, N, 1.0, 2, st)), keys[0] and (keys[0],))
        else:
            add(f"{name}: forward, rows {M}", "gemm_pst_kernel / gemm_f32_kernel (k-major, k-major)", per_step, fl,
                med(lambda: call("nnhipLinearModuleForward", X, W, b, O_, M, K, N, st)), keys[0] and (keys[0],))
        if swish == "dx":
            Zin = rnd(M, K)
            add(f"{name}: input gradient x the saved swish'(z), in place over it", "gemm_pst_kernel<4> (multiply epilogue)", per_step, fl,
                med(lambda: call("nnhipLinearInputGradScaled", dO, W, Zin, Zin, M, K, N, st)), keys[1] and (keys[1],))
        else:
            add(f"{name}: input gradient", "gemm_pst_kernel / gemm_f32_kernel (k-major, outer-major)", per_step, fl,
                med(lambda: call("nnhipLinearModuleBackward", X, W, dO, dX, None, None, M, K, N, st)), keys[1] and (keys[1],))
        if with_dw:
            dW, db = torch.empty(N, K, device="cuda"), torch.empty(1, N, device="cuda")
            add(f"{name}: weight + bias gradient", "gemm_f32_group_kernel (uneven two-way split) + splitk_reduce", per_step, fl,
                med(lambda: call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, M, K, N, st)), keys[2])

    linear_fwd_dx(f"q|k|v projection {D}->{3 * D}", D, 3 * D, L, keys=("qkv_fwd", "qkv_dx", None))
    linear_fwd_dx(f"attention output projection {D}->{D}", D, D, L, keys=("out_fwd", "out_dx", None))
    linear_fwd_dx(f"FFN {D}->{F}", D, F, L, keys=("fc1_fwd_swish", "fc1_dx", None), swish="fwd")
    linear_fwd_dx(f"FFN {F}->{D}", F, D, L, keys=("fc2_fwd", "fc2_dx_swish", None), swish="dx")
    linear_fwd_dx(f"vocabulary head {D}->{V}", D, V, 1, with_dw=True, keys=("head_fwd", "head_dx", ("head_dw", "head_dw_reduce")))
    # what the step launches for a decoder layer's parameter gradients: the four dW+db GEMMs as ONE grid + ONE reduce
    # (deferred parameter gradients) -- C4's largest kernel by device time
    jobs = [(rnd(M, K), rnd(N, K) / 16, rnd(M, N), torch.empty(N, K, device="cuda"), torch.empty(1, N, device="cuda"), K, N)
            for (N, K) in ((D, F), (F, D), (D, D), (3 * D, D))]

    def grouped():
        call("nnhipWeightGradDefer", 1, st)
        for (X, W, dO, dW, db, K, N) in jobs:
            call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, M, K, N, st)
        call("nnhipWeightGradDefer", 0, st)

    add(f"dW+db of one decoder layer (4 GEMMs, rows {M}), deferred", "gemm_f32_group_kernel<32> + splitk_reduce_group_kernel", L,
        sum(2.0 * M * K * N for (*_, K, N) in jobs), med(grouped), ("layer_dw", "layer_dw_reduce"))
    del jobs
    qkv = rnd(Bq, T, 3 * D)
    dqkv = torch.empty_like(qkv)
    kval = torch.ones(Bq, T, dtype=torch.int32, device="cuda")
    ctx, dctx, lse = torch.empty(Bq, T, D, device="cuda"), rnd(Bq, T, D), torch.empty(Bq, H, T, 2, device="cuda")
    q_, k_, v_ = (qkv[..., i * D:(i + 1) * D] for i in range(3))
    dq_, dk_, dv_ = (dqkv[..., i * D:(i + 1) * D] for i in range(3))
    sc, dh = 1.0 / float(np.sqrt(D)), D // H
    afl = 4.0 * Bq * H * T * T * dh / 2                  # causal: half the score matrix; backward = 2.5 x forward
    add(f"fused attention forward B{Bq} T{T} H{H} dh{dh} (causal)", "attn_sb_fwd_kernel", L, afl,
        med(lambda: call("nnhipAttentionForward", StridedView(q_), StridedView(k_), StridedView(v_), kval, ctx, lse, Bq, H, T, T, dh,
                         3 * D, sc, 1, st)), ("attn_fwd",))
    add(f"fused attention backward B{Bq} T{T} H{H} dh{dh} (causal)", "attn_sb_bwd_kernel (one pass, 5 GEMMs per tile pair)", L, 2.5 * afl,
        med(lambda: call("nnhipAttentionBackward", StridedView(q_), StridedView(k_), StridedView(v_), kval, ctx, dctx, lse,
                         StridedView(dq_), StridedView(dk_), StridedView(dv_), Bq, H, T, T, dh, 3 * D, sc, 1, st)), ("attn_bwd",))
    return fams


def c4_weighted_roofline(fams):
    """Flop-weighted MFMA figure of one C4 step's GEMM + attention launches: sum(per_step x flops) / sum(per_step x ms)."""
    fl = sum(f["per_step"] * f["flops"] for f in fams)
    ms = sum(f["per_step"] * f["ms"] for f in fams)
    dom = max(fams, key=lambda f: f["per_step"] * f["ms"])
    return fl, ms, dom


def workload_headline(args, rank, world):
    """BASELINE.json's metric in one run: C4 GPT-tiny step (value), C2 Linear forward vs MFMA peak (roofline), C1
    MNIST-MLP samples/s and the C2 step (also).  Without --full: the C4 step alone, with the roofline of its own timed steps."""
    import copy
    res = workload_c4(args, rank, world)
    if not args.full:
        return res
    args = copy.copy(args)
    args.dump_outputs = None                          # the legs below run other steps: the dump is the headline step's
    c4_roof = res.pop("roofline")
    fwd = c2_forward_roofline()
    c2_obj = {
        "kernel": "gemm_f32_kernel<32,k-major,k-major> -- C2 Linear(4096->4096) forward, batch 4096 (BASELINE's 'Linear fwd GFLOP/s vs MFMA peak')",
        "bound": "mfma", "achieved": round(fwd["burst_tflops"], 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
        "frac": round(fwd["burst_tflops"] / PEAK_F32_MFMA_TFLOPS, 4), "traffic": read_traffic("gemm_fwd_c2"),
        "traffic_source": traffic_source(),
        "flops_per_launch": fwd["flops"], "avg_launch_ms": round(fwd["burst_ms"], 4),
        "sustained": {"tflops": round(fwd["sustained_tflops"], 2), "frac": round(fwd["sustained_tflops"] / PEAK_F32_MFMA_TFLOPS, 4),
                      "avg_launch_ms": round(fwd["sustained_ms"], 4), "launches": fwd["sustained_launches"]},
    }
    tr, alg = c2_obj["traffic"], 3 * 4096 * 4096 * 4
    if tr:
        c2_obj["traffic_over_algorithmic"] = round(tr / alg, 2)
        c2_obj["traffic_note"] = (f"L2<->fabric requests per launch (Infinity-Cache hits included) are {tr / alg:.2f}x the {alg / 1e6:.0f} MB of operands + result: "
                                  "the two resident blocks of a CU drift apart and each cohort streams its own panels (DESIGN 5.1g); MFMA-bound at N = 1")
    also = {"c4_gemm": {"what": "whole C4 step, GEMM-equivalent flops (Linear fwd/dX/dW + attention) / device step time",
                        "tflops": c4_roof["achieved"], "frac_of_mfma_peak": c4_roof["frac"],
                        "flops_per_step": c4_roof["flops_per_step"], "avg_step_device_ms": c4_roof["avg_step_device_ms"]},
            "c2_linear_forward": c2_obj}
    res["roofline"] = c2_obj          # replaced below by the C4 step's own kernels when they could be timed
    if rank == 0 or world == 1:
        try:
            fams = c4_family_rooflines()
            also["c4_families"] = fams
            fl, ms, dom = c4_weighted_roofline(fams)
            res["roofline"] = {
                "kernel": "the exact-fp32 MFMA kernels of the C4 step itself -- gemm_f32_group_kernel, gemm_f32_kernel, gemm_pst_kernel, attn_sb_* "
                          "(97 % of the step's device time) -- every launch of one step at its own shape, flop-weighted; largest single kernel: "
                          + dom["kernels"] + " (" + dom["family"] + ")",
                "bound": "mfma", "achieved": round(fl / (ms * 1e-3) / 1e12, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": round(fl / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                "traffic": None, "flops_per_step": fl, "kernel_ms_per_step": round(ms, 4),
                "how": "HIP events on the launch stream around each launch (median of 20), also.c4_families lists them; "
                       "profiles/r05*_c4_kernel_stats.md is the rocprofv3 view of the same kernels inside the step",
                "dominant_kernel": {"name": dom["kernels"], "what": dom["family"], "launches_per_step": dom["per_step"],
                                    "flops_per_launch": dom["flops"], "avg_launch_ms": dom["ms"], "tflops": dom["tflops"],
                                    "frac": dom["frac_of_mfma_peak"], "instep_ms": dom.get("instep_ms"),
                                    "instep_frac": dom.get("instep_frac_of_mfma_peak")},
                "c2_linear_forward": {k: c2_obj[k] for k in ("achieved", "frac", "avg_launch_ms", "traffic", "traffic_over_algorithmic") if k in c2_obj},
            }
            if all("instep_ms" in f for f in fams):
                ims = sum(f["per_step"] * f["instep_ms"] for f in fams)
                res["roofline"]["instep"] = {
                    "frac": round(fl / (ims * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4), "kernel_ms_per_step": round(ims, 4),
                    "what": "the same flop-weighted figure with every family's duration taken INSIDE the replayed step (rocprofv3 kernel trace, "
                            "profiles/c4_instep_families.json, collection " + str(read_instep().get("_collected")) + "; not measured by this run): "
                            "what the isolated HIP-event figures above flatter by a few per cent"}
            # fabric bytes of the dominant kernel as launched INSIDE the step (two decoder layers' eight dW GEMMs per launch):
            # committed PMC passes over `bench.py --workload c4` (tools/collect_profiles.sh), halved to the one-layer unit of
            # `dominant_kernel.flops_per_launch`; algorithmic = the eight operands read once + the four split-K slabs written
            tr2 = read_traffic("gemm_group_dw2_c4") if "dW+db of one decoder layer" in dom["family"] else None
            if tr2:
                rows_, cols_ = 64 * 256, (1536 + 512) + (512 + 512) + (2048 + 512) + (512 + 2048)
                outs_ = 512 * 1536 + 512 * 512 + 512 * 2048 + 2048 * 512
                alg = 4.0 * (rows_ * cols_ + 4 * outs_)
                res["roofline"]["traffic"] = round(tr2 / 2.0)
                res["roofline"]["traffic_what"] = ("fabric bytes per launch of the dominant kernel (one decoder layer's share of the two-layer "
                                                   "grouped dW launch), (2*FETCH_SIZE + WRITE_SIZE)*1024 / 2; " + (traffic_source() or ""))
                res["roofline"]["traffic_over_algorithmic"] = round(tr2 / 2.0 / alg, 2)
                res["roofline"]["dominant_kernel"]["algorithmic_bytes_per_launch"] = alg
        except Exception as exc:  # noqa: BLE001
            also["c4_families"] = {"error": repr(exc)[:300]}
    # C1: MNIST-MLP, sustained
    a1 = copy.copy(args)
    a1.steps, a1.warmup = args.c1_steps, 20
    def guarded(name, fn):
        # the headline value (C4) is already measured: a side workload that fails (N > 1 has only run on gloo here) is
        # reported as such instead of taking the JSON line down with it
        try:
            fn()
        except Exception as exc:  # noqa: BLE001
            also[name] = {"error": repr(exc)[:300]}
            print(f"[bench] also.{name} failed: {exc!r}", file=sys.stderr)

    def run_c1():
        r1 = workload_c1(a1, rank, world)
        also["c1"] = {"workload": r1["config"]["workload"], "samples_per_s": round(r1["samples_per_step"] * a1.steps / r1["dt"], 1),
                      "ms_per_step": round(r1["dt"] / a1.steps * 1e3, 5), "steps": a1.steps,
                      "device_ms_per_step": r1["roofline"].get("avg_step_device_ms"), "launch": r1["config"].get("launch"),
                      "launches_per_step": r1["extra"].get("launches_per_step"),
                      "optimizer_launch": r1["config"].get("optimizer_launch")}
    guarded("c1", run_c1)

    def run_c1_variants():
        # (a) with the per-step input copy the reference's benches include; (b) backward and Adam as two
        # launches (what the default was before round 5; NNHIP_AUTO_FUSE_STEP=0); (c) the round-3 opt-in
        for key, kw in (("with_input_copy", {"c1_input_copy": 1}), ("separate_optimizer_launch", {"c1_fuse_opt": 0}),
                        ("opt_in_fuse_backward", {"c1_fuse_opt": 1})):
            av = copy.copy(a1)
            for k, v in kw.items():
                setattr(av, k, v)
            rv = workload_c1(av, rank, world)
            also["c1"][key] = {"samples_per_s": round(rv["samples_per_step"] * av.steps / rv["dt"], 1),
                               "ms_per_step": round(rv["dt"] / av.steps * 1e3, 5),
                               "device_ms_per_step": rv["roofline"].get("avg_step_device_ms"),
                               "launches_per_step": rv["extra"].get("launches_per_step"),
                               "input": rv["config"]["input"], "optimizer_launch": rv["config"]["optimizer_launch"]}
        also["c1"]["input"] = "batches resident in HBM"
    if "error" not in also.get("c1", {"error": 1}):
        guarded("c1_variants", run_c1_variants)

    def run_c3():
        # BASELINE config 3 / north_star's HBM target (">= 60 % HBM-BW roofline on fused Swish/RMSNorm"): every op of the fused
        # micro-bench at rows 8192 x d 4096, HIP-event timed per launch inside one pass over all of them (cold caches: each
        # op streams 270-940 MB between two launches of itself)
        a3 = copy.copy(args)
        a3.steps, a3.warmup = 20, 5
        r3 = workload_c3(a3, rank, world)
        also["c3"] = {"workload": r3["config"]["workload"], "ms_per_pass": round(r3["dt"] / a3.steps * 1e3, 4),
                      "ops": r3["extra"]["ops"], "hbm_peak_GBps": PEAK_HBM_GBS, "mfma_peak_tflops": PEAK_F32_MFMA_TFLOPS,
                      "methodology": "scripts/benchmark_swish_cuda.py:65-69 shape: pre-allocated buffers, functional C-ABI calls, "
                                     "warm-up then timed iterations; bytes = algorithmic (SURVEY 8d), time = HIP events on the launch stream"}
    if os.environ.get("NNHIP_BENCH_C3", "1") != "0":
        guarded("c3", run_c3)

    def run_c5():
        a5 = copy.copy(args)
        a5.steps, a5.warmup = 480, 32
        r5 = workload_c5(a5, rank, world)
        also["c5"] = {"workload": r5["config"]["workload"], "samples_per_s": round(r5["samples_per_step"] * a5.steps / r5["dt"], 1),
                      "ms_per_step": round(r5["dt"] / a5.steps * 1e3, 5), "steps": a5.steps,
                      "device_ms_per_step": r5["roofline"].get("avg_step_device_ms"), "launch": r5["config"].get("launch"),
                      "launches_per_step": r5["extra"].get("launches_per_step"),
                      "conv_layers": r5["extra"].get("conv_layers"),
                      "frac_of_hbm_peak_on_conv_bytes": r5["roofline"]["frac"],
                      "bound_by": r5["extra"].get("bound_by")}
        # the opt-in one-launch tail (NNHIP_BN_HEAD_FUSION=1; round 5): fewer launches, measured beside the default
        import neunet_hip.nn.experimental.vision as _vis
        was = _vis._FUSE_TAIL
        _vis._FUSE_TAIL = True
        try:
            a5t = copy.copy(a5)
            r5t = workload_c5(a5t, rank, world)
            also["c5"]["tail_one_launch_opt_in"] = {"samples_per_s": round(r5t["samples_per_step"] * a5.steps / r5t["dt"], 1),
                                                    "ms_per_step": round(r5t["dt"] / a5.steps * 1e3, 5),
                                                    "launches_per_step": r5t["extra"].get("launches_per_step"),
                                                    "what": "NNHIP_BN_HEAD_FUSION=1: conv2's launch leaves partial batch statistics; BatchNorm2d + Linear + Sigmoid + MSELoss as one kernel"}
        finally:
            _vis._FUSE_TAIL = was
    if os.environ.get("NNHIP_BENCH_C5", "1") != "0":
        guarded("c5", run_c5)

    def run_strong():
        # SURVEY 8e wants both curves: the line's `value` is the weak-scaling step (64 sequences per GPU); this is the
        # strong-scaling one (the global batch of 64 divided over the ranks) -- or the reverse under --scaling strong
        a_s = copy.copy(args)
        a_s.scaling = "weak" if args.scaling == "strong" else "strong"
        a_s.steps, a_s.warmup = args.steps, max(2, args.warmup // 2)
        rs = workload_c4(a_s, rank, world)
        also["c4_" + a_s.scaling] = {"workload": rs["config"]["workload"], "scaling": rs["config"]["scaling"],
                                     "global_batch": rs["config"]["global_batch"],
                                     "samples_per_s": round(rs["samples_per_step"] * a_s.steps / rs["dt"], 2),
                                     "ms_per_step": round(rs["dt"] / a_s.steps * 1e3, 4),
                                     "dp_exchange": rs["extra"]["dp_exchange"]}
    if world > 1 and args.c4_batch >= world:
        guarded("c4_other_scaling", run_strong)
    # C2: the whole Linear training step
    a2 = copy.copy(args)
    a2.steps, a2.warmup = 20, 5

    def run_c2():
        r2 = workload_c2(a2, rank, world)
        also["c2"] = {"workload": r2["config"]["workload"], "samples_per_s": round(r2["samples_per_step"] * a2.steps / r2["dt"], 1),
                      "ms_per_step": round(r2["dt"] / a2.steps * 1e3, 4), "linear_fwd_tflops_in_step": r2["extra"]["linear_fwd_tflops"],
                      "linear_bwd_tflops_in_step": r2["extra"]["linear_bwd_tflops"]}
    guarded("c2", run_c2)

    def run_nb():
        an = copy.copy(args)
        an.steps, an.warmup = 100, 10
        rn = workload_nb(an, rank, world)
        also["nb"] = {"workload": rn["config"]["workload"], **rn["extra"]}
    if os.environ.get("NNHIP_BENCH_NB", "1") != "0":
        guarded("nb", run_nb)
    def run_ls_sweep():
        # The reference's own bench sweep (scripts/benchmark_linear_swish_cuda.py:127-138) with its methodology (:16-56, :59-118): module
        # API, and INSIDE the timed loop a device copy of x, a fresh Tensor, the module call -- plus a fresh random upstream gradient and
        # backward() for the f+b column; 20 warm-up + 60 timed iterations between two events (the reference: 50 + 200)
        import torch
        import neunet_hip
        import neunet_hip.nn as nn
        gsw = torch.Generator(device="cuda").manual_seed(5)
        rows_out = []

        def timed(fn, warm=20, iters=60):
            for _ in range(warm):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / iters

        for (Bn, I, Od) in [(32, 256, 512), (64, 256, 512), (128, 256, 512), (256, 512, 1024), (512, 512, 1024), (1024, 512, 1024),
                            (1024, 1024, 2048), (2048, 1024, 2048), (4096, 1024, 4096)]:
            np.random.seed(77)
            fused = nn.LinearSwish(I, Od, swish_beta=1.0)
            xd = torch.rand(Bn, I, device="cuda", generator=gsw) * 2 - 1

            def fwd():
                return fused(neunet_hip.Tensor(xd.clone(), device="cuda", requires_grad=False))

            def fwd_bwd():
                X = neunet_hip.Tensor(xd.clone(), device="cuda", requires_grad=True)
                out = fused(X)
                out.backward(torch.rand(Bn, Od, device="cuda", generator=gsw) * 2 - 1)
                fused.weight.grad = None
                fused.bias.grad = None

            f, fb = timed(fwd), timed(fwd_bwd)
            rows_out.append({"B": Bn, "in": I, "out": Od, "fwd_ms": round(f, 4), "fwd_bwd_ms": round(fb, 4),
                             "fwd_tflops_incl_host": round(2.0 * Bn * I * Od / (f * 1e-3) / 1e12, 2)})
        also["linear_swish_sweep"] = {
            "what": "the reference's Linear->Swish bench sweep (scripts/benchmark_linear_swish_cuda.py:127-138) through HIPLinearSwish with the reference's "
                    "methodology: per iteration a device copy of x, a fresh Tensor, the module call [+ random upstream gradient, backward()]; eager launches "
                    "from Python, so the small sizes measure the host (~0.05 ms per call), not the kernel",
            "rows": rows_out}
    if os.environ.get("NNHIP_BENCH_LS_SWEEP", "1") != "0" and (rank == 0 or world == 1) and os.environ.get("NNHIP_BENCH_TOY", "0") != "1":
        guarded("linear_swish_sweep", run_ls_sweep)
    # opt-in split-bf16 GEMM mode (fp32 operands split exactly into 3 bf16 pieces, 6 products on the bf16 matrix cores):
    # reported NEXT TO the exact-fp32 numbers above, never instead of them
    if os.environ.get("NNHIP_BENCH_BF16X3", "1") != "0":
        from neunet_hip._lib import call_hip_function
        call_hip_function("nnhipSetGemmMode", 1)

        def run_bf3():
            f3 = c2_forward_roofline(iters=30, sustain_s=1.0)
            a4 = copy.copy(args)
            a4.steps, a4.warmup = 10, 3
            r4 = workload_c4(a4, rank, world)
            also["bf16x3"] = {
                "what": "the same C2 forward GEMM and C4 step with nnhipSetGemmMode(1): every fp32 operand split exactly "
                        "into three bf16 pieces, six piece products accumulated in fp32 by v_mfma_f32_32x32x16_bf16 "
                        "(relative error ~2^-23 per product; parity tests hold the same 1e-4 tolerance). OPT-IN, not the default",
                "c2_linear_fwd_tflops_fp32_equiv": round(f3["burst_tflops"], 2),
                "c2_linear_fwd_sustained_tflops_fp32_equiv": round(f3["sustained_tflops"], 2),
                "c2_bf16_mfma_tflops": round(6 * f3["burst_tflops"], 1), "bf16_mfma_peak_tflops": 2500.0,
                "c2_frac_of_bf16_mfma_peak": round(6 * f3["burst_tflops"] / 2500.0, 4),
                "c4_samples_per_s": round(r4["samples_per_step"] * a4.steps / r4["dt"], 2),
                "c4_ms_per_step": round(r4["dt"] / a4.steps * 1e3, 4),
            }
        try:
            guarded("bf16x3", run_bf3)
        finally:
            call_hip_function("nnhipSetGemmMode", 0)
    res["extra"]["also"] = also
    return res


def cpu_headline(seconds):
    out = cpu_c4(seconds)
    c1 = cpu_c1(3.0)
    out["also_c1"] = {"value": c1["value"], "unit": c1["unit"], "samples": c1["samples"], "sample": c1["sample"]}
    try:
        c5 = cpu_c5(4.0)
        out["also_c5"] = {"value": c5["value"], "unit": c5["unit"], "samples": c5["samples"], "sample": c5["sample"]}
    except Exception as exc:  # noqa: BLE001
        out["also_c5"] = {"error": repr(exc)[:200]}
    return out


def respawn_under_torchrun(args):
    """`python bench.py --gpus N` without a torchrun environment: start N ranks (one per GPU) of this same script."""
    import socket
    import subprocess
    import torch
    ngpu = torch.cuda.device_count()
    if ngpu < args.gpus and os.environ.get("NNHIP_ALLOW_OVERSUBSCRIBE", "0") != "1":
        print(f"bench.py: --gpus {args.gpus} but only {ngpu} GPU(s) are visible (set NNHIP_ALLOW_OVERSUBSCRIBE=1 to run "
              f"{args.gpus} ranks on them over gloo for a functional check)", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if ngpu < args.gpus:
        env.setdefault("NNHIP_DIST_BACKEND", "gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def rccl_choices(log_path):
    """What RCCL says it chose: the algorithm / protocol lines of its TUNING log (NCCL_DEBUG=INFO, NCCL_DEBUG_SUBSYS=...,TUNING:
    "<coll>: <bytes> Bytes -> Algo <a> proto <p> time <t>") grouped by (collective, bytes), plus the channel / ring / tree summary of
    the communicator.  A ring on the full xGMI mesh is per-link bound: this is the line to read when N = 8 scales badly."""
    import re
    algos = {0: "TREE", 1: "RING", 2: "COLLNET_DIRECT", 3: "COLLNET_CHAIN", 4: "NVLS", 5: "NVLS_TREE", 6: "PAT"}
    protos = {0: "LL", 1: "LL128", 2: "SIMPLE"}
    out = {"log": log_path, "source": "NCCL_DEBUG=INFO NCCL_DEBUG_SUBSYS=INIT,GRAPH,TUNING written by RCCL on rank 0"}
    if not log_path or not os.path.exists(log_path):
        out["note"] = "no RCCL debug file (NCCL_DEBUG was set by the caller, or the backend is not nccl)"
        return out
    pat = re.compile(r"(\w+): (\d+) Bytes -> Algo (\d+) proto (\d+) time ([0-9.eE+-]+)")
    seen, version, channels = {}, None, None
    with open(log_path, errors="replace") as f:
        for ln in f:
            m = pat.search(ln)
            if m:
                key = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))
                seen[key] = seen.get(key, 0) + 1
            if version is None and ("RCCL version" in ln or "NCCL version" in ln):
                version = ln.strip().split("INFO", 1)[-1].strip()[:120]
            m2 = re.search(r"(\d+) coll channels", ln)
            if m2 and channels is None:
                channels = ln.strip().split("INFO", 1)[-1].strip()[:160]
    out["version"] = version
    out["channels"] = channels
    out["choices"] = [{"collective": c, "bytes": b, "algorithm": algos.get(a, str(a)), "protocol": protos.get(pr, str(pr)), "calls": n}
                      for (c, b, a, pr), n in sorted(seen.items(), key=lambda kv: -kv[0][1])[:12]]
    if not seen:
        out["note"] = "RCCL printed no TUNING line (a 1-rank communicator short-cuts the algorithm choice; gloo has none)"
    return out


def claim_stdout():
    """stdout must carry exactly ONE JSON line, but libraries write there too (RCCL prints a five-line version banner to
    stdout when its communicator comes up).  Point file descriptor 1 at stderr for the life of the process and hand
    back a handle on the real stdout for the JSON line."""
    sys.stdout.flush()
    real = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    return real


def main():
    args = parse()
    if args.cpu_full_batch:
        r = cpu_c4(1e9, Bs=64, max_steps=max(1, args.cpu_full_steps))
        r["collected"] = time.strftime("%Y-%m-%d") + " (round 6)"
        print(json.dumps(r), flush=True)
        return
    if args.dump_outputs and args.workload not in ("headline", "c4"):
        print(f"bench.py: --dump-outputs writes the C4 step's outputs (--workload headline or c4), not --workload {args.workload}",
              file=sys.stderr)
        sys.exit(2)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(respawn_under_torchrun(args))
    json_out = claim_stdout()
    rccl_log = None
    # (the GPU boxes of this pool export NCCL_DEBUG=VERSION: anything below INFO without a file of its own is raised to INFO + file)
    if (int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.force_dp) and \
            (os.environ.get("NCCL_DEBUG", "VERSION").upper() in ("VERSION", "WARN", "") and "NCCL_DEBUG_FILE" not in os.environ):
        # RCCL's own account of the communicator (ranks, rings/trees, transport) goes to a per-rank file -- its default
        # sink is stdout, which must carry exactly one JSON line -- and rank 0 echoes the topology lines to stderr below
        rccl_log = f"/tmp/nnhip_rccl.{os.getpid()}.log"
        os.environ.update(NCCL_DEBUG="INFO", NCCL_DEBUG_SUBSYS="INIT,GRAPH,TUNING", NCCL_DEBUG_FILE=rccl_log)
    import torch
    from neunet_hip.distributed import init_process_group
    import neunet_hip
    rank, world = init_process_group(force=args.force_dp)
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s)", file=sys.stderr)
        sys.exit(2)
    neunet_hip.load_library()
    # The line says `dtype: f32` and prices its kernels against the fp32 MFMA peak: that is only true in GEMM mode 0 (exact fp32,
    # v_mfma_f32_32x32x2_f32).  NNHIP_GEMM_MODE=bf16x3 in the environment would route every Linear GEMM through the split-bf16
    # kernel and produce a faster, mislabelled line (round-5 review): refuse instead.  The opt-in mode is measured by the headline
    # workload itself, under also.bf16x3, with the mode switched on and off around that leg only.
    from neunet_hip._lib import call_hip_function as _mode_call
    gemm_mode = int(_mode_call("nnhipGetGemmMode"))
    if gemm_mode != 0:
        if rank == 0:
            print(f"bench.py: nnhipGetGemmMode() = {gemm_mode} (NNHIP_GEMM_MODE={os.environ.get('NNHIP_GEMM_MODE')!r}): the bench line's `value` "
                  "and `dtype: f32` are defined for the exact-fp32 GEMM (mode 0) only; unset NNHIP_GEMM_MODE (the opt-in mode is "
                  "reported under also.bf16x3 by the default run)", file=sys.stderr)
        sys.exit(4)
    rccl_ranks = 1
    if world > 1 or args.force_dp:
        import torch.distributed as dist
        probe = torch.ones(1, device="cuda")
        dist.all_reduce(probe)                          # a real collective before anything is reported
        rccl_ranks = int(round(float(probe.item())))
        if rccl_ranks != world:
            # the one number that says the ranks really talk to each other: a wrong sum is a broken job, not a slow one
            print(f"bench.py: all-reduce of ones over {world} rank(s) on backend {dist.get_backend()} returned {probe.item()!r}", file=sys.stderr)
            sys.exit(3)
        if rank == 0:
            print(f"[bench] backend={dist.get_backend()} world={dist.get_world_size()} all-reduce(1)={rccl_ranks}",
                  file=sys.stderr)
            if rccl_log and os.path.exists(rccl_log):
                keep = ("nranks", "Ring", "Tree", "Channel", "via", "Using", "Connected", "comm ")
                with open(rccl_log, errors="replace") as f:
                    lines = [ln.rstrip() for ln in f if any(k in ln for k in keep)]
                for ln in lines[:60]:
                    print("[rccl] " + ln, file=sys.stderr)
    wl = {"headline": workload_headline, "c1": workload_c1, "c2": workload_c2, "c3": workload_c3, "c4": workload_c4,
          "c5": workload_c5, "nb": workload_nb}[args.workload]
    res = wl(args, rank, world)
    dt = res["dt"]
    value = res["samples_per_step"] * args.steps / dt
    out = {
        "metric": "samples/sec training step", "value": round(value, 2), "unit": "samples/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": res.get("scaling", "weak"),
        "vs_baseline": None, "dtype": "f32", "data": "synthetic", "config": res["config"],
        "roofline": res["roofline"], "rccl_ranks": rccl_ranks,
    }
    if world > 1 or args.force_dp:
        import torch.distributed as dist
        out["dist_backend"] = dist.get_backend()
        if rank == 0:
            out["rccl"] = rccl_choices(rccl_log)
    out.update(res.get("extra", {}))
    out["gemm_mode"] = int(_mode_call("nnhipGetGemmMode"))            # 0 = exact fp32; checked again AFTER the run: a leg that left
    if out["gemm_mode"] != 0:                                          # the opt-in mode switched on would have tainted what followed
        print("bench.py: the GEMM mode is not 0 at the end of the run", file=sys.stderr)
        sys.exit(4)
    try:
        from neunet_hip._lib import call_hip_function as _call
        out["gemm_lockstep"] = int(_call("nnhipGetGemmLockstep"))     # 1 by default when more than one rank exchanges gradients
    except Exception:  # noqa: BLE001
        pass
    if rank == 0:
        if args.full and not args.no_cpu_baseline:  # N > 1 too: timed on rank 0's host cores while the other ranks wait at the barrier
            out["cpu_baseline"] = {"headline": cpu_headline, "c1": cpu_c1, "c2": cpu_c2, "c3": cpu_c3, "c4": cpu_c4,
                                   "c5": cpu_c5, "nb": cpu_nb}[args.workload](args.cpu_seconds)
        print(json.dumps(out), file=json_out, flush=True)
    if world > 1 or args.force_dp:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
