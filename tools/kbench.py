#!/usr/bin/env python3
"""Per-kernel micro-benchmark through the C ABI (HIP events on the launch stream).  Developer tool for A/B
work on the GPU box:   python tools/kbench.py [--only gemm,swish,...] [--iters 30]
Prints one line per op: median / min ms and the algorithmic TFLOP/s or GB/s (SURVEY 8d figures)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "numpy-nn-model_amd"))

import torch  # noqa: E402

from neunet_hip import _lib  # noqa: E402
from neunet_hip._lib import Conv2dDesc, ConvTranspose2dDesc, call_hip_function as call  # noqa: E402
import ctypes  # noqa: E402


COLD = {"on": False, "scrub": None}


def bench(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if COLD["on"]:            # --cold: 1.5 GiB of unrelated traffic between launches (L2 / MALL hold none of the operands,
            COLD["scrub"].add_(1.0)   # and carry a dirty tail to write back, like the previous kernel of a real step)
        a.record()
        fn()
        b.record()
        ts.append((a, b))
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ts])
    return float(np.median(ms)), float(ms.min())


def bench_samples(fn, iters, warmup=5):
    """Like bench(), but returns every timed launch (ms): for percentiles over the repeats of alternating routes."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ts.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ts]


def report(name, med, mn, flops=None, nbytes=None):
    s = f"{name:34s} med {med:9.4f} ms  min {mn:9.4f} ms"
    if flops:
        s += f"  {flops / (med * 1e-3) / 1e12:8.2f} TFLOP/s ({flops / (med * 1e-3) / 1e12 / 157.3 * 100:5.1f}% of 157.3)"
    if nbytes:
        s += f"  {nbytes / (med * 1e-3) / 1e9:8.1f} GB/s ({nbytes / (med * 1e-3) / 1e9 / 8000 * 100:5.1f}% of 8 TB/s)"
    print(s, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--gemm-mode", type=int, default=0, help="0 = exact fp32 MFMA (default), 1 = split-bf16 (bf16x3)")
    ap.add_argument("--cold", action="store_true", help="scrub the caches between timed launches")
    args = ap.parse_args()
    if args.cold:
        COLD["on"], COLD["scrub"] = True, torch.zeros(3 * (1 << 27), device="cuda")
    call("nnhipSetGemmMode", args.gemm_mode)
    only = set(filter(None, args.only.split(",")))
    want = lambda k: not only or k in only  # noqa: E731
    st = _lib.get_current_stream_ptr()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: (torch.rand(*s, device=dev, generator=g) * 2 - 1)  # noqa: E731
    randn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731

    if want("gemm"):
        for (M, N, K) in [(4096, 4096, 4096), (8192, 4096, 4096), (16384, 512, 512), (16384, 2048, 512),
                          (16384, 512, 2048), (16384, 15000, 512)]:
            X, W, b = rnd(M, K), rnd(N, K) / 64, rnd(N)
            O_, dO, dX, dW, db = torch.empty(M, N, device=dev), rnd(M, N), torch.empty(M, K, device=dev), \
                torch.empty(N, K, device=dev), torch.empty(N, device=dev)
            fl = 2.0 * M * N * K
            tag = f"{M}x{K}->{N}"
            report(f"linear fwd {tag}", *bench(lambda: call("nnhipLinearModuleForward", X, W, b, O_, M, K, N, st), args.iters), flops=fl)
            report(f"linear dX  {tag}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, dX, None, None, M, K, N, st), args.iters), flops=fl)
            report(f"linear dW  {tag}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, None, dW, None, M, K, N, st), args.iters), flops=fl)
            report(f"linear dW+db {tag}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, M, K, N, st), args.iters), flops=fl)
            report(f"linear dX+dW+db {tag}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, dX, dW, db, M, K, N, st), args.iters), flops=2 * fl)
            report(f"linear db  {tag}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, None, None, db, M, K, N, st), args.iters), nbytes=4.0 * M * N)
            del X, W, O_, dO, dX, dW

    if "gemmfwd" in only:         # forward only, the two big shapes (tile-order / priority experiments)
        for (M, N, K) in [(4096, 4096, 4096), (8192, 4096, 4096), (16384, 2048, 512)]:
            X, W, b, O_ = rnd(M, K), rnd(N, K) / 64, rnd(N), torch.empty(M, N, device=dev)
            report(f"linear fwd {M}x{K}->{N}", *bench(lambda: call("nnhipLinearModuleForward", X, W, b, O_, M, K, N, st), args.iters), flops=2.0 * M * N * K)
            if M * N * K >= 2 ** 36:
                dO, dX, dW = rnd(M, N), torch.empty(M, K, device=dev), torch.empty(N, K, device=dev)
                report(f"linear dX  {M}x{K}->{N}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, dX, None, None, M, K, N, st), args.iters), flops=2.0 * M * N * K)
                report(f"linear dW  {M}x{K}->{N}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, None, dW, None, M, K, N, st), args.iters), flops=2.0 * M * N * K)
                del dO, dX, dW
            del X, W, O_

    if "headpad" in only:         # does the vocabulary head pay for rows of 15000 floats (60000 B: no multiple of a 128-B line)?
        for (M, N, K) in [(16384, 15000, 512), (16384, 15008, 512), (16384, 15104, 512)]:
            X, W, b = rnd(M, K), rnd(N, K) / 64, rnd(N)
            O_, dO, dX, dW, db = torch.empty(M, N, device=dev), rnd(M, N), torch.empty(M, K, device=dev), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
            fl = 2.0 * M * N * K
            report(f"linear fwd {M}x{K}->{N}", *bench(lambda: call("nnhipLinearModuleForward", X, W, b, O_, M, K, N, st), args.iters), flops=fl)
            report(f"linear dX  {M}x{K}->{N}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, dX, None, None, M, K, N, st), args.iters), flops=fl)
            report(f"linear dW+db {M}x{K}->{N}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, M, K, N, st), args.iters), flops=fl)
            del X, W, O_, dO, dX, dW

    if "dwsweep" in only:         # the parameter-gradient GEMMs of the C4 step (split-K candidates)
        for (M, N, K) in [(16384, 512, 512), (16384, 1536, 512), (16384, 2048, 512), (16384, 512, 2048), (16384, 15000, 512), (16384, 6144, 512)]:
            X, W, dO = rnd(M, K), rnd(N, K) / 64, rnd(M, N)
            dW, db = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
            report(f"linear dW+db {M}x{K}->{N}", *bench(lambda: call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, M, K, N, st), args.iters), flops=2.0 * M * N * K)
            del X, W, dO, dW

    if want("wgroup"):            # a GPT-tiny decoder layer's four dW+db GEMMs: four launches vs the deferred queue's one grid
        M = 16384
        jobs = []
        for (N, K) in [(512, 2048), (2048, 512), (512, 512), (1536, 512)]:      # out, in -- the order backward meets them
            jobs.append((rnd(M, K), rnd(N, K) / 64, rnd(M, N), torch.empty(N, K, device=dev), torch.empty(N, device=dev), K, N))
        fl = sum(2.0 * M * N * K for (*_, K, N) in jobs)

        def separate():
            for (X, W, dO, dW, db, K, N) in jobs:
                call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, M, K, N, st)

        def grouped():
            call("nnhipWeightGradDefer", 1, st)
            for (X, W, dO, dW, db, K, N) in jobs:
                call("nnhipLinearModuleBackward", X, W, dO, None, dW, db, M, K, N, st)
            call("nnhipWeightGradDefer", 0, st)

        report("4 x linear dW+db, GPT-tiny layer (4 launches + 4 reduces)", *bench(separate, args.iters), flops=fl)
        report("4 x linear dW+db, GPT-tiny layer (deferred: 1 grid + 1 reduce)", *bench(grouped, args.iters), flops=fl)
        del jobs

    R, D = 8192, 4096
    n = R * D
    if want("lswish"):
        X, W, b = rnd(R, D), rnd(D, D) / 64, rnd(D)
        O_, Z = torch.empty(R, D, device=dev), torch.empty(R, D, device=dev)
        report("linear_swish fwd (save z)", *bench(lambda: call("nnhipLinearSwishForward", X, W, b, O_, Z, R, D, D, 1.0, 1, st), args.iters), flops=2.0 * R * D * D)
        X5, W5, b5 = rnd(16384, 512), rnd(2048, 512) / 16, rnd(2048)
        O5, Z5 = torch.empty(16384, 2048, device=dev), torch.empty(16384, 2048, device=dev)
        report("linear_swish fwd 16384x512->2048 (save z)", *bench(lambda: call("nnhipLinearSwishForward", X5, W5, b5, O5, Z5, 16384, 512, 2048, 1.0, 1, st), args.iters), flops=2.0 * 16384 * 512 * 2048)
        report("linear fwd 16384x512->2048", *bench(lambda: call("nnhipLinearModuleForward", X5, W5, b5, O5, 16384, 512, 2048, st), args.iters), flops=2.0 * 16384 * 512 * 2048)
        dO5, W6 = rnd(16384, 512), rnd(512, 2048) / 16
        report("dZ = (dO W) swish'(z) 16384x512->2048 (in place)", *bench(lambda: call("nnhipLinearInputGradSwish", dO5, W6, Z5, Z5, 16384, 2048, 512, 1.0, st), args.iters), flops=2.0 * 16384 * 512 * 2048)
        dX5 = torch.empty(16384, 2048, device=dev)
        report("linear dX 16384x2048<-512 (plain)", *bench(lambda: call("nnhipLinearModuleBackward", Z5, W6, dO5, dX5, None, None, 16384, 2048, 512, st), args.iters), flops=2.0 * 16384 * 512 * 2048)
        report("linear_swish fwd (no z)", *bench(lambda: call("nnhipLinearSwishForward", X, W, b, O_, None, R, D, D, 1.0, 0, st), args.iters), flops=2.0 * R * D * D)
        del X, W, O_, Z
    x, dy, y, dx = randn(R, D), randn(R, D), torch.empty(R, D, device=dev), torch.empty(R, D, device=dev)
    if want("swish"):
        report("swish fwd 8192x4096", *bench(lambda: call("nnhipSwishForward", y, x, 1.0, n, st), args.iters), nbytes=8.0 * n)
        report("swish bwd 8192x4096", *bench(lambda: call("nnhipSwishBackward", dx, dy, x, 1.0, n, st), args.iters), nbytes=12.0 * n)
        report("relu fwd 8192x4096", *bench(lambda: call("nnhipReLUForward", y, x, n, st), args.iters), nbytes=8.0 * n)
        report("add 8192x4096", *bench(lambda: call("nnhipAdd", y, x, dy, n, st), args.iters), nbytes=12.0 * n)
    if want("swiglu"):
        o2, d2 = torch.empty(R, D // 2, device=dev), randn(R, D // 2)
        report("swiglu fwd 8192x(2x2048)", *bench(lambda: call("nnhipFusedSwishAndMul", o2, x, 1.0, D // 2, n // 2, st), args.iters), nbytes=12.0 * n / 2)
        report("swiglu bwd 8192x(2x2048)", *bench(lambda: call("nnhipFusedSwishAndMulBackward", dx, d2, x, 1.0, D // 2, n // 2, st), args.iters), nbytes=20.0 * n / 2)
    if want("softmax"):
        report("softmax fwd 8192x4096", *bench(lambda: call("nnhipSoftmaxForward", y, x, R, D, 1, st), args.iters), nbytes=8.0 * n)
        report("softmax bwd 8192x4096", *bench(lambda: call("nnhipSoftmaxBackward", dx, dy, y, R, D, 1, st), args.iters), nbytes=12.0 * n)
        xs = randn(64 * 8 * 256, 256)
        ys = torch.empty_like(xs)
        report("softmax fwd (64,8,256,256)", *bench(lambda: call("nnhipSoftmaxForward", ys, xs, xs.shape[0], 256, 1, st), args.iters), nbytes=8.0 * xs.numel())
    if want("rmsnorm"):
        w, std = torch.ones(D, device=dev), torch.empty(R, device=dev)
        dw = torch.empty(D, device=dev)
        report("rmsnorm fwd 8192x4096", *bench(lambda: call("nnhipRMSNormForward", x, w, None, y, std, None, R, D, 1e-6, st), args.iters), nbytes=8.0 * n)
        report("rmsnorm bwd 8192x4096", *bench(lambda: call("nnhipRMSNormBackward", dy, x, w, std, None, dx, dw, None, R, D, st), args.iters), nbytes=12.0 * n)
        x5, y5, dy5, dx5 = randn(16384, 512), torch.empty(16384, 512, device=dev), randn(16384, 512), torch.empty(16384, 512, device=dev)
        w5, s5, dw5 = torch.ones(512, device=dev), torch.empty(16384, device=dev), torch.empty(512, device=dev)
        report("rmsnorm fwd 16384x512", *bench(lambda: call("nnhipRMSNormForward", x5, w5, None, y5, s5, None, 16384, 512, 1e-6, st), args.iters), nbytes=8.0 * x5.numel())
        report("rmsnorm bwd 16384x512", *bench(lambda: call("nnhipRMSNormBackward", dy5, x5, w5, s5, None, dx5, dw5, None, 16384, 512, st), args.iters), nbytes=12.0 * x5.numel())
        add5 = randn(16384, 512)
        # the form the C4 step launches 12 times: the residual branch's gradient added in the same pass (16 B per element), dw finished later
        report("rmsnorm bwd 16384x512 +addend", *bench(lambda: call("nnhipRMSNormBackwardEx", dy5, x5, w5, s5, None, add5, dx5, dw5, None, 16384, 512, st), args.iters), nbytes=16.0 * x5.numel())
    if want("ce"):
        labels = torch.randint(0, D, (R,), device=dev, dtype=torch.int32)
        loss, lse = torch.empty(R, device=dev), torch.empty(R, device=dev)
        report("ce fwd+bwd 8192x4096", *bench(lambda: call("nnhipCrossEntropyForwardBackward", x, loss, lse, labels, D, -100, R, D, b"m", R, None, dx, st), args.iters), nbytes=8.0 * n)
        lo, cnt = torch.empty((), device=dev), torch.empty(1, device=dev, dtype=torch.int32)
        report("ce loss(mean) 1 launch 8192x4096", *bench(lambda: call("nnhipCrossEntropyLossEx", x, dx, loss, lse, labels, 4, None, D, -100, R, D, b"m", lo, cnt, st), args.iters), nbytes=8.0 * n)
        V = 15000
        xl, dxl = randn(16384, V), torch.empty(16384, V, device=dev)
        lab = torch.randint(0, V, (16384,), device=dev, dtype=torch.int32)
        l2, s2 = torch.empty(16384, device=dev), torch.empty(16384, device=dev)
        report("ce fwd+bwd 16384x15000", *bench(lambda: call("nnhipCrossEntropyForwardBackward", xl, l2, s2, lab, V, 0, 16384, V, b"m", 16384, None, dxl, st), args.iters), nbytes=8.0 * xl.numel())
        report("ce loss(mean) 1 launch 16384x15000", *bench(lambda: call("nnhipCrossEntropyLossEx", xl, dxl, l2, s2, lab, 4, None, V, 0, 16384, V, b"m", lo, cnt, st), args.iters), nbytes=8.0 * xl.numel())
        del xl, dxl
    if want("adamw"):
        p, m, v = randn(R, D), torch.zeros(R, D, device=dev), torch.zeros(R, D, device=dev)
        report("adamw single 8192x4096", *bench(lambda: call("nnhipFusedAdamWStep", p, dy, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, n, 0, 1.0, st), args.iters), nbytes=28.0 * n)
        opt = _lib.load_hip_function("nnhipCreateFusedOptimizer")()
        nt = 200
        ps = [randn(512, 1024) for _ in range(nt)]
        gs = [randn(512, 1024) for _ in range(nt)]
        ms = [torch.zeros(512, 1024, device=dev) for _ in range(nt)]
        vs = [torch.zeros(512, 1024, device=dev) for _ in range(nt)]
        arr = lambda ts: (ctypes.c_void_p * nt)(*[t.data_ptr() for t in ts])  # noqa: E731
        cp, cg, cm, cv = arr(ps), arr(gs), arr(ms), arr(vs)
        cs = (ctypes.c_int64 * nt)(*[t.numel() for t in ps])
        cast = lambda a, t: ctypes.cast(a, ctypes.POINTER(t))  # noqa: E731
        report("adamw multi 200x(512,1024)", *bench(lambda: call(
            "nnhipFusedAdamWMultiTensorStep", opt, nt, cast(cp, ctypes.c_void_p), cast(cg, ctypes.c_void_p),
            cast(cm, ctypes.c_void_p), cast(cv, ctypes.c_void_p), cast(cs, ctypes.c_int64), 1e-3, 0.9, 0.999, 1e-8, 1e-2,
            3, 0, 1.0, st), args.iters), nbytes=28.0 * nt * 512 * 1024)
    if want("attn"):
        # fused attention at the C4 shape (B64 T256 H8 dh64, pad+causal): Q/K/V as column blocks of one [B,T,3D] buffer
        for (B_, T_, H_, dh) in [(64, 256, 8, 64), (16, 1024, 8, 64), (64, 256, 4, 128)]:
            Dm = H_ * dh
            qkv = randn(B_, T_, 3 * Dm)
            dqkv = torch.empty_like(qkv)
            kvalid = torch.ones(B_, T_, dtype=torch.int32, device=dev)
            ctx, dctx = torch.empty(B_, T_, Dm, device=dev), randn(B_, T_, Dm)
            lse = torch.empty(B_, H_, T_, 2, device=dev)
            q_, k_, v_ = (qkv[..., i * Dm:(i + 1) * Dm] for i in range(3))
            dq_, dk_, dv_ = (dqkv[..., i * Dm:(i + 1) * Dm] for i in range(3))
            sc = 1.0 / float(np.sqrt(Dm))
            fwd_fl = 4.0 * B_ * H_ * T_ * T_ * dh / 2          # causal: half the score matrix
            f = lambda: call("nnhipAttentionForward", _lib.StridedView(q_), _lib.StridedView(k_), _lib.StridedView(v_), kvalid,  # noqa: E731
                             ctx, lse, B_, H_, T_, T_, dh, 3 * Dm, sc, 1, st)
            bw = lambda: call("nnhipAttentionBackward", _lib.StridedView(q_), _lib.StridedView(k_), _lib.StridedView(v_), kvalid,  # noqa: E731
                              ctx, dctx, lse, _lib.StridedView(dq_), _lib.StridedView(dk_), _lib.StridedView(dv_), B_, H_, T_, T_, dh,
                              3 * Dm, sc, 1, st)
            report(f"attn fwd B{B_} T{T_} H{H_} dh{dh} causal", *bench(f, args.iters), flops=fwd_fl)
            report(f"attn bwd B{B_} T{T_} H{H_} dh{dh} causal", *bench(bw, args.iters), flops=2.5 * fwd_fl)

    if "attnlayout" in only:
        # the same attention work (512 heads of T256 dh64) from three layouts: fused [B,T,3D] (row stride 6 KB, 256-B head
        # segments), separate [B,T,D] tensors (2 KB stride) and head-major [B*H,T,dh] (contiguous): is the strided gather the cost?
        T_, dh = 256, 64
        sc = 1.0 / float(np.sqrt(512))
        fwd_fl = 4.0 * 512 * T_ * T_ * dh / 2
        for name, B_, H_, packed in [("fused qkv [B,T,3D]", 64, 8, True), ("separate [B,T,D]", 64, 8, False), ("head-major [BH,T,dh]", 512, 1, False)]:
            Dm = H_ * dh
            kvalid = torch.ones(B_, T_, dtype=torch.int32, device=dev)
            ctx, dctx = torch.empty(B_, T_, Dm, device=dev), randn(B_, T_, Dm)
            lse = torch.empty(B_, H_, T_, 2, device=dev)
            if packed:
                qkv = randn(B_, T_, 3 * Dm); dqkv = torch.empty_like(qkv)
                q_, k_, v_ = (_lib.StridedView(qkv[..., i * Dm:(i + 1) * Dm]) for i in range(3))
                dq_, dk_, dv_ = (_lib.StridedView(dqkv[..., i * Dm:(i + 1) * Dm]) for i in range(3))
                LQ = 3 * Dm
            else:
                q_, k_, v_ = randn(B_, T_, Dm), randn(B_, T_, Dm), randn(B_, T_, Dm)
                dq_, dk_, dv_ = torch.empty_like(q_), torch.empty_like(q_), torch.empty_like(q_)
                LQ = Dm
            f = lambda: call("nnhipAttentionForward", q_, k_, v_, kvalid, ctx, lse, B_, H_, T_, T_, dh, LQ, sc, 1, st)  # noqa: E731
            bw = lambda: call("nnhipAttentionBackward", q_, k_, v_, kvalid, ctx, dctx, lse, dq_, dk_, dv_, B_, H_, T_, T_, dh, LQ, sc, 1, st)  # noqa: E731
            report(f"attn fwd {name}", *bench(f, args.iters), flops=fwd_fl)
            report(f"attn bwd {name}", *bench(bw, args.iters), flops=2.5 * fwd_fl)

    if want("lssweep"):
        # The reference's own Linear->Swish sweep (scripts/benchmark_linear_swish_cuda.py:127-138) with its methodology
        # (:16-56, :59-118): 50 warm-up + 200 timed iterations between two events, and INSIDE the timed loop a device copy
        # of x, a fresh Tensor, the module call (forward) or call + fresh random upstream gradient + backward.
        import neunet_hip
        import neunet_hip.nn as nn
        print("Linear->Swish sweep, reference methodology (module API, per-iteration device copy + Tensor + launch; "
              "ms per iteration):")
        print(f"{'B x In x Out':>20s} {'fwd fused':>10s} {'fwd 2-op':>10s} {'f+b fused':>10s} {'f+b 2-op':>10s} {'fwd kernel':>11s} {'TFLOP/s':>8s}")

        def timed(fn, warm=50, iters=200):
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
            fused = nn.LinearSwish(I, Od, swish_beta=1.0)
            lin, act = nn.Linear(I, Od), nn.Swish(1.0)
            lin.weight.data.copy_(fused.weight.data)
            lin.bias.data.copy_(fused.bias.data)
            xd = rnd(Bn, I)

            def f_fused():
                return fused(neunet_hip.Tensor(xd.clone(), device="cuda", requires_grad=False))

            def f_two():
                h = lin(neunet_hip.Tensor(xd.clone(), device="cuda", requires_grad=False))
                _ = h.data                                 # the plain GEMM, then the Swish pass: two launches
                return act(h)

            def fb(mod_call, params):
                X = neunet_hip.Tensor(xd.clone(), device="cuda", requires_grad=True)
                out = mod_call(X)
                out.backward(rnd(Bn, Od))
                for p_ in params:
                    p_.grad = None

            def two(X):
                h = lin(X)
                _ = h.data
                return act(h)

            t_ff, t_f2 = timed(f_fused), timed(f_two)
            t_bf = timed(lambda: fb(fused, (fused.weight, fused.bias)))
            t_b2 = timed(lambda: fb(two, (lin.weight, lin.bias)))
            O_ = torch.empty(Bn, Od, device=dev)
            tk, _ = bench(lambda: call("nnhipLinearSwishForward", xd, fused.weight.data, fused.bias.data, O_, None, Bn, I, Od, 1.0, 0, st), 50)
            print(f"{f'{Bn} x {I} x {Od}':>20s} {t_ff:10.4f} {t_f2:10.4f} {t_bf:10.4f} {t_b2:10.4f} {tk:11.4f} {2.0 * Bn * I * Od / (tk * 1e-3) / 1e12:8.2f}", flush=True)

    if want("convg"):
        # the implicit-GEMM conv kernels at MFMA-bound shapes (channels > 16: conv_mfma.hip)
        for (B, Cin, H, Cout) in [(64, 64, 56, 128), (128, 128, 28, 128), (64, 32, 56, 64), (64, 256, 14, 256), (32, 512, 7, 512)]:
            X = rnd(B, Cin, H, H)
            W = rnd(Cout, Cin, 3, 3) / 24
            bb = rnd(Cout)
            O_ = torch.empty(B, Cout, H, H, device=dev)
            dO = rnd(B, Cout, H, H)
            dX = torch.empty_like(X)
            d = Conv2dDesc(B, Cin, H, H, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
            fl = 2.0 * B * H * H * Cout * Cin * 9
            report(f"conv igemm fwd   {B}x{Cin}x{H}x{H}->{Cout}", *bench(lambda: call("nnhipConv2dForward", X, W, bb, O_, ctypes.byref(d), st), args.iters), flops=fl)
            report(f"conv igemm dgrad {B}x{Cin}x{H}x{H}->{Cout}", *bench(lambda: call("nnhipConv2dBackward", X, W, dO, dX, None, None, ctypes.byref(d), st), args.iters), flops=fl)
            dW, db = torch.empty_like(W), torch.empty_like(bb)
            report(f"conv wgrad+db    {B}x{Cin}x{H}x{H}->{Cout}", *bench(lambda: call("nnhipConv2dBackward", X, W, dO, None, dW, db, ctypes.byref(d), st), args.iters), flops=fl)

    if "convu" in only:           # the reference's DDPM U-Net body (scripts/torch_ddpm.py:451-452: channels 32..512 on 32x32 images), batch 64
        for (B, Cin, H, Cout) in [(64, 32, 32, 64), (64, 64, 16, 128), (64, 128, 8, 256), (64, 256, 4, 512), (64, 512, 2, 512), (64, 512, 4, 256), (64, 128, 16, 64)]:
            X, W, bb = rnd(B, Cin, H, H), rnd(Cout, Cin, 3, 3) / 24, rnd(Cout)
            O_, dO = torch.empty(B, Cout, H, H, device=dev), rnd(B, Cout, H, H)
            dX, dW, db = torch.empty_like(X), torch.empty_like(W), torch.empty_like(bb)
            d = Conv2dDesc(B, Cin, H, H, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
            fl = 2.0 * B * H * H * Cout * Cin * 9
            report(f"conv fwd      {B}x{Cin}x{H}x{H}->{Cout}", *bench(lambda: call("nnhipConv2dForward", X, W, bb, O_, ctypes.byref(d), st), args.iters), flops=fl)
            report(f"conv dgrad    {B}x{Cin}x{H}x{H}->{Cout}", *bench(lambda: call("nnhipConv2dBackward", X, W, dO, dX, None, None, ctypes.byref(d), st), args.iters), flops=fl)
            report(f"conv wgrad+db {B}x{Cin}x{H}x{H}->{Cout}", *bench(lambda: call("nnhipConv2dBackward", X, W, dO, None, dW, db, ctypes.byref(d), st), args.iters), flops=fl)

    if "convt" in only:
        # the up-block transforms of the reference's DDPM U-Net (examples/ddpm.ipynb cell 5: ConvTranspose2d(C, C, 4x4, stride 2,
        # padding 1)) at the batch convu uses: the UTKFace configuration's three, then the MNIST configuration's two.  The forward
        # on the stride-phase kernel and on the dgrad gather ALTERNATE in this process (`rounds` rounds each; the spread is
        # (max - min) / median of a route's round medians); their outputs are compared on the seeded inputs first.
        # FLOP/s on the algorithmic count 2 B H W Cin Cout kh kw.
        rounds = 5
        for (B, C, H) in [(64, 512, 4), (64, 256, 8), (64, 128, 16), (64, 64, 8), (64, 32, 16)]:
            X, W, bb = rnd(B, C, H, H), rnd(C, C, 4, 4) / (4 * C ** 0.5), rnd(C)
            O_, dO = torch.empty(B, C, 2 * H, 2 * H, device=dev), rnd(B, C, 2 * H, 2 * H)
            dX, dW, db = torch.empty_like(X), torch.empty_like(W), torch.empty_like(bb)
            d = ConvTranspose2dDesc(B, C, H, H, C, 4, 4, 2, 2, 1, 1, 1, 1, 1, 1, 0, 0)
            fl = 2.0 * B * H * H * C * C * 16
            tag = f"{B}x{C}x{H}x{H}->{2 * H}x{2 * H}"
            fwd = lambda: call("nnhipConvTranspose2dForward", X, W, bb, O_, ctypes.byref(d), st)  # noqa: E731
            outs = {}
            for route in (1, 2):
                prev = call("nnhipSetConvTransposeRoute", route)
                fwd()
                outs[route] = O_.clone()
                call("nnhipSetConvTransposeRoute", prev)
            diff = float((outs[1] - outs[2]).abs().max())
            ref = torch.nn.functional.conv_transpose2d(X.double(), W.double().flip(2, 3).transpose(0, 1), bb.double(), 2, 1)
            err = [float((outs[r].double() - ref).abs().max()) for r in (1, 2)]
            print(f"convT {tag}: |phase - gather| max {diff:.2e}; vs float64 phase {err[0]:.2e} gather {err[1]:.2e} (|O| max {float(ref.abs().max()):.2f})")
            meds = {1: [], 2: []}
            for _ in range(rounds):
                for route in (1, 2):
                    prev = call("nnhipSetConvTransposeRoute", route)
                    meds[route].append(bench(fwd, args.iters)[0])
                    call("nnhipSetConvTransposeRoute", prev)
            for route, name in ((1, "phase "), (2, "gather")):
                m = np.array(meds[route])
                report(f"convT fwd {name} {tag}", float(np.median(m)), float(m.min()), flops=fl)
                print(f"{'':34s} round medians {' '.join(f'{v:.4f}' for v in m)}  spread {(m.max() - m.min()) / np.median(m) * 100:.1f} %")
            report(f"convT dX         {tag}", *bench(lambda: call("nnhipConvTranspose2dBackward", X, W, dO, dX, None, None, ctypes.byref(d), st), args.iters), flops=fl)
            report(f"convT dW+db      {tag}", *bench(lambda: call("nnhipConvTranspose2dBackward", X, W, dO, None, dW, db, ctypes.byref(d), st), args.iters), flops=fl)

    if "bn1d" in only:
        # BatchNorm1d on [N, F]: the column-strip kernels (nnhipBatchNorm1d*, csrc/batchnorm1d.hip) against the only route the library
        # had before, the BatchNorm2d entries at (N, F, 1, 1).  The two routes ALTERNATE in this process (`rounds` rounds each);
        # per route and direction: the median of the round medians, and p10 - p90 of all timed launches.  GB/s on the algorithmic
        # bytes (forward: read X, write Y; backward: read dY and X, write dX).  The notebooks' shapes, then two large ones.
        rounds = 5
        for (N, F) in [(100, 2), (100, 256), (100, 512), (1024, 1024), (8192, 512)]:
            X, dY, w, b = randn(N, F) + 1.0, randn(N, F), rnd(F) + 1.5, rnd(F)
            Y, dX, dW, db = (torch.empty(N, F, device=dev), torch.empty(N, F, device=dev), torch.empty(F, device=dev), torch.empty(F, device=dev))
            sm, si, rm, rv = torch.empty(F, device=dev), torch.empty(F, device=dev), torch.zeros(F, device=dev), torch.ones(F, device=dev)
            routes = {
                "bn1d": (lambda: call("nnhipBatchNorm1dForward", X, w, b, Y, sm, si, rm, rv, N, F, 1e-5, 0.1, 1, st),
                         lambda: call("nnhipBatchNorm1dBackward", dY, X, w, sm, si, dX, dW, db, N, F, st)),
                "bn2d": (lambda: call("nnhipBatchNorm2dForward", X, w, b, Y, sm, si, rm, rv, N, F, 1, 1e-5, 0.1, 1, st),
                         lambda: call("nnhipBatchNorm2dBackward", dY, X, w, sm, si, dX, dW, db, N, F, 1, st)),
                # the read + write roof for the same bytes (tools/stream_roof.py's kernels at this footprint): one read and one
                # write per element beside the forward, two reads and one write beside the backward
                "stream": (lambda: call("nnhipReLUForward", Y, X, N * F, st), lambda: call("nnhipAdd", dX, dY, X, N * F, st))}
            outs = {}
            for name, (fwd, bwd) in list(routes.items())[:2]:
                fwd()
                bwd()
                outs[name] = (Y.clone(), dX.clone())
            print(f"bn1d {N}x{F}: |bn1d - bn2d| max: Y {float((outs['bn1d'][0] - outs['bn2d'][0]).abs().max()):.2e}, "
                  f"dX {float((outs['bn1d'][1] - outs['bn2d'][1]).abs().max()):.2e}")
            samples = {(name, k): [] for name in routes for k in (0, 1)}
            meds = {key: [] for key in samples}
            for _ in range(rounds):
                for name, fns in routes.items():
                    for k, fn in enumerate(fns):
                        ms = bench_samples(fn, args.iters)
                        samples[(name, k)].extend(ms)
                        meds[(name, k)].append(float(np.median(ms)))
            for k, direction in enumerate(("fwd", "bwd")):
                nbytes = 4.0 * N * F * (2 if k == 0 else 3)
                for name in routes:
                    allms, m = np.array(samples[(name, k)]), np.array(meds[(name, k)])
                    report(f"{name} {direction} {N}x{F}", float(np.median(m)), float(allms.min()), nbytes=nbytes)
                    print(f"{'':34s} p10 {np.percentile(allms, 10):.4f}  p90 {np.percentile(allms, 90):.4f} ms over {allms.size} launches; "
                          f"round medians {' '.join(f'{v:.4f}' for v in m)}")

    def alternate(routes, rounds, label, nbytes):
        """routes: {name: (forward fn, backward fn)}, alternating in this process for `rounds` rounds; per route and direction the
        median of the round medians, the fastest launch and p10 - p90 of all timed launches; GB/s on the algorithmic bytes."""
        samples = {(name, k): [] for name in routes for k in (0, 1)}
        meds = {key: [] for key in samples}
        for _ in range(rounds):
            for name, fns in routes.items():
                for k, fn in enumerate(fns):
                    ms = bench_samples(fn, args.iters)
                    samples[(name, k)].extend(ms)
                    meds[(name, k)].append(float(np.median(ms)))
        for k, direction in enumerate(("fwd", "bwd")):
            for name in routes:
                allms, m = np.array(samples[(name, k)]), np.array(meds[(name, k)])
                report(f"{name} {direction} {label}", float(np.median(m)), float(allms.min()), nbytes=nbytes)
                print(f"{'':34s} p10 {np.percentile(allms, 10):.4f}  p90 {np.percentile(allms, 90):.4f} ms over {allms.size} launches; "
                      f"round medians {' '.join(f'{v:.4f}' for v in m)}")

    if "avgpool" in only:
        # AvgPool2d (nnhipAvgPool2d*, csrc/avgpool.hip): LeNet-5's two pools at batch 256, a large 2x2/2 pool and a global pool.  The
        # tier the descriptor selects, the general tier forced on the same descriptor (nnhipSetAvgPool2dRoute), torch's avg_pool2d
        # (its backward through torch.ops.aten.avg_pool2d_backward) and the read + write roof for the same bytes (the library's ReLU
        # over (n_in + n_out) / 2 elements: tools/stream_roof.py's kernel at this footprint) ALTERNATE in this process.
        from neunet_hip._lib import Pool2dDesc
        F = torch.nn.functional
        tiers = {0: "general", 1: "tiles", 2: "global_wave", 3: "global_block"}
        for (B, C, H, W, k) in [(256, 6, 28, 28, 2), (256, 16, 10, 10, 2), (64, 64, 112, 112, 2), (256, 512, 7, 7, 7), (64, 64, 56, 56, 56)]:
            d = Pool2dDesc(B, C, H, W, k, k, k, k, 0, 0, 0, 0, 1, 1)
            X, dY = randn(B, C, H, W), randn(B, C, H // k, W // k)
            Y, dX = torch.empty_like(dY), torch.empty_like(X)
            n = (X.numel() + Y.numel()) // 2
            sa, sb = torch.empty(n, device=dev), randn(n)
            tier = tiers[call("nnhipAvgPool2dTier", ctypes.byref(d))]

            def forced(entry, dst, src):
                def run():
                    prev = call("nnhipSetAvgPool2dRoute", 1)
                    call(entry, dst, src, ctypes.byref(d), st)
                    call("nnhipSetAvgPool2dRoute", prev)
                return run

            routes = {tier: (lambda: call("nnhipAvgPool2dForward", Y, X, ctypes.byref(d), st),
                             lambda: call("nnhipAvgPool2dBackward", dX, dY, ctypes.byref(d), st)),
                      "general": (forced("nnhipAvgPool2dForward", Y, X), forced("nnhipAvgPool2dBackward", dX, dY)),
                      "torch": (lambda: F.avg_pool2d(X, k), lambda: torch.ops.aten.avg_pool2d_backward(dY, X, [k, k], [k, k], [0, 0], False, True, None)),
                      "stream": (lambda: call("nnhipReLUForward", sa, sb, n, st), lambda: call("nnhipReLUForward", sa, sb, n, st))}
            outs = {}
            for name in (tier, "general"):
                routes[name][0]()
                routes[name][1]()
                outs[name] = (Y.clone(), dX.clone())
            ref = (F.avg_pool2d(X.double(), k), torch.ops.aten.avg_pool2d_backward(dY.double(), X.double(), [k, k], [k, k], [0, 0], False, True, None))
            print(f"avgpool {B}x{C}x{H}x{W} k{k} [{tier}]: |{tier} - general| max Y {float((outs[tier][0] - outs['general'][0]).abs().max()):.2e} "
                  f"dX {float((outs[tier][1] - outs['general'][1]).abs().max()):.2e}; vs float64 Y {float((outs[tier][0].double() - ref[0]).abs().max()):.2e} "
                  f"dX {float((outs[tier][1].double() - ref[1]).abs().max()):.2e}")
            alternate(routes, 5, f"{B}x{C}x{H}x{W} k{k}", 4.0 * (X.numel() + Y.numel()))

    if "zeropad" in only:
        # ZeroPad2d: nnhipSliceBackward as the pad, nnhipSliceForward as the crop (what nn.ZeroPad2d launches), beside
        # torch.nn.functional.pad / a contiguous copy of the cropped view and the read + write roof for the same bytes.
        from neunet_hip.tensor_ops import _i64, contiguous_strides
        for (B, C, H, W, p) in [(256, 1, 28, 28, 2), (64, 64, 56, 56, 1)]:
            X, G = randn(B, C, H, W), randn(B, C, H + 2 * p, W + 2 * p)
            Y, dX = torch.empty_like(G), torch.empty_like(X)
            n = (X.numel() + Y.numel()) // 2
            sa, sb = torch.empty(n, device=dev), randn(n)
            shp, pshp = _i64(X.shape), _i64(Y.shape)
            start, step, strides = _i64((0, 0, p, p)), _i64((1, 1, 1, 1)), _i64(contiguous_strides(tuple(Y.shape)))
            off = p * (W + 2 * p) + p
            routes = {"slice": (lambda: call("nnhipSliceBackward", Y, X, 4, pshp, start, step, shp, st),
                                lambda: call("nnhipSliceForward", dX, G, off, 0, 4, shp, strides, st)),
                      "torch": (lambda: torch.nn.functional.pad(X, (p, p, p, p)), lambda: G[:, :, p:p + H, p:p + W].contiguous()),
                      "stream": (lambda: call("nnhipReLUForward", sa, sb, n, st), lambda: call("nnhipReLUForward", sa, sb, n, st))}
            routes["slice"][0]()
            routes["slice"][1]()
            print(f"zeropad {B}x{C}x{H}x{W} p{p}: pad == torch {bool(torch.equal(Y, torch.nn.functional.pad(X, (p, p, p, p))))}, "
                  f"crop == torch {bool(torch.equal(dX, G[:, :, p:p + H, p:p + W]))}")
            alternate(routes, 5, f"{B}x{C}x{H}x{W} p{p}", 4.0 * (X.numel() + Y.numel()))

    if "vq" in only:
        # The nearest-code search (nnhipVQNearest, csrc/vector_quantize.hip) against the composition a user would otherwise write on
        # torch: z @ E.T, the two norms, argmin, index_select -- an N x K matrix written and read back.  The two routes and a read-only
        # roof (a sum over z and one over the codebook: every operand byte once, nothing written) ALTERNATE in this process (`rounds`
        # rounds each); per route: the median of the round medians and p10 - p90 of all timed launches.  Flops: 2 N K D against the
        # fp32 MFMA peak.  The notebook's shape, two image-VQ-VAE shapes, and a wide / large-codebook one.
        rounds = 5
        for (N, D, K) in [(100, 2, 100), (8192, 64, 512), (32768, 64, 1024), (4096, 256, 8192)]:
            z, E = randn(N, D), rnd(K, D)
            idx, zq = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, D, device=dev)

            def composed():
                dist = (z * z).sum(1, keepdim=True) + (E * E).sum(1) - 2.0 * (z @ E.T)
                i = torch.argmin(dist, dim=1)
                return i, torch.index_select(E, 0, i)

            routes = {"vq": lambda: call("nnhipVQNearest", z, E, idx, zq, N, D, K, st), "torch": composed,
                      "read": lambda: (z.sum(), E.sum())}
            routes["vq"]()
            ti, _ = composed()
            print(f"vq {N}x{D} K={K}: indices equal to the torch composition's on {float((ti.to(torch.int32) == idx).float().mean()) * 100:.3f} % "
                  f"of the rows; N x K matrix {4.0 * N * K / 1e6:.2f} MB, codebook {4.0 * K * D / 1e6:.2f} MB")
            samples, meds = {name: [] for name in routes}, {name: [] for name in routes}
            for _ in range(rounds):
                for name, fn in routes.items():
                    ms = bench_samples(fn, args.iters)
                    samples[name].extend(ms)
                    meds[name].append(float(np.median(ms)))
            for name in routes:
                allms, m = np.array(samples[name]), np.array(meds[name])
                report(f"{name} {N}x{D} K={K}", float(np.median(m)), float(allms.min()), flops=None if name == "read" else 2.0 * N * K * D,
                       nbytes=4.0 * (N * D + K * D) if name == "read" else None)
                print(f"{'':34s} p10 {np.percentile(allms, 10):.4f}  p90 {np.percentile(allms, 90):.4f} ms over {allms.size} launches; "
                      f"round medians {' '.join(f'{v:.4f}' for v in m)}")

    def alternate(title, routes, rounds=5, nbytes=None):
        """The routes ALTERNATE in this process (`rounds` rounds each); per route the median of the round medians, the fastest launch,
        and p10 - p90 of all timed launches.  nbytes: {route: algorithmic bytes}."""
        samples, meds = {name: [] for name in routes}, {name: [] for name in routes}
        for _ in range(rounds):
            for name, fn in routes.items():
                ms = bench_samples(fn, args.iters)
                samples[name].extend(ms)
                meds[name].append(float(np.median(ms)))
        for name in routes:
            allms, m = np.array(samples[name]), np.array(meds[name])
            report(f"{name} {title}", float(np.median(m)), float(allms.min()), nbytes=(nbytes or {}).get(name))
            print(f"{'':34s} p10 {np.percentile(allms, 10):.4f}  p90 {np.percentile(allms, 90):.4f} ms over {allms.size} launches")

    if "act" in only:
        # Softplus, Softsign, Mish, TanhExp, ELU, SELU, log (nnhipActivationForward / Backward, csrc/elementwise.hip) beside nnhipTanhForward /
        # Backward on the same 2^26 elements: the same map kernels and the same bytes (8 B / element forward, 12 backward), so a kind
        # slower than Tanh is paying for its VALU work.
        n = 1 << 26
        X, dY, Y, dX = randn(n) * 2, randn(n), torch.empty(n, device=dev), torch.empty(n, device=dev)
        Xp = X.abs() + 0.05
        kinds = ("softplus", "softsign", "mish", "tanhexp", "elu", "selu", "log")
        fwd = {"tanh": lambda: call("nnhipTanhForward", Y, X, n, st)}
        bwd = {"tanh": lambda: call("nnhipTanhBackward", dX, dY, X, n, st)}
        for k, name in enumerate(kinds):
            src = Xp if name == "log" else X
            fwd[name] = lambda k=k, src=src: call("nnhipActivationForward", k, Y, src, 0.1, n, st)
            bwd[name] = lambda k=k, src=src: call("nnhipActivationBackward", k, dX, dY, src, 0.1, n, st)
        alternate("fwd 2^26", fwd, nbytes={name: 8.0 * n for name in fwd})
        alternate("bwd 2^26", bwd, nbytes={name: 12.0 * n for name in bwd})
        del X, dY, Y, dX, Xp

    if "tape" in only:
        # The Tensor arithmetic (csrc/tensor_ops.hip): same-shape mul / div beside nnhipMul; the inner-row and outer-column broadcasts
        # beside the same-shape kernel on the same output bytes and beside the torch expression; row / column / NCHW-channel reductions
        # beside torch.sum (algorithmic bytes: the input once); the fused broadcast backward (dB of a * b without the full-shape
        # gradient) beside the unfused pair (nnhipMul into a full-shape buffer, then the reduction).
        def i64(*v):
            return (ctypes.c_int64 * len(v))(*v)

        def i32(*v):
            return (ctypes.c_int32 * len(v))(*v)

        n = 1 << 26
        A, B, O = randn(n), randn(n).abs() + 0.5, torch.empty(n, device=dev)
        sh, s1 = i64(n), i64(1)
        alternate("same 2^26", {"nnhipMul": lambda: call("nnhipMul", O, A, B, n, st),
                                "mul": lambda: call("nnhipBroadcastBinaryForward", 2, O, A, B, 0.0, 1, sh, s1, s1, st),
                                "div": lambda: call("nnhipBroadcastBinaryForward", 3, O, A, B, 0.0, 1, sh, s1, s1, st),
                                "mul scalar": lambda: call("nnhipBroadcastBinaryForward", 2, O, A, None, 0.5, 1, sh, s1, s1, st)},
                  nbytes={"nnhipMul": 12.0 * n, "mul": 12.0 * n, "div": 12.0 * n, "mul scalar": 8.0 * n})
        del A, B, O
        N, F = 16384, 4096
        X, X2, row, col, O = randn(N, F), randn(N, F), randn(F), randn(N, 1), torch.empty(N, F, device=dev)
        sh2, full, srow, scol = i64(N, F), i64(F, 1), i64(0, 1), i64(1, 0)
        alternate(f"[{N},{F}] mul", {"same": lambda: call("nnhipBroadcastBinaryForward", 2, O, X, X2, 0.0, 2, sh2, full, full, st),
                                     "inner [F]": lambda: call("nnhipBroadcastBinaryForward", 2, O, X, row, 0.0, 2, sh2, full, srow, st),
                                     "outer [N,1]": lambda: call("nnhipBroadcastBinaryForward", 2, O, X, col, 0.0, 2, sh2, full, scol, st),
                                     "torch inner": lambda: torch.mul(X, row, out=O), "torch outer": lambda: torch.mul(X, col, out=O)},
                  nbytes={"same": 12.0 * N * F, "inner [F]": 8.0 * N * F, "outer [N,1]": 8.0 * N * F, "torch inner": 8.0 * N * F,
                          "torch outer": 8.0 * N * F})
        orow, ocol = torch.empty(N, device=dev), torch.empty(F, device=dev)
        alternate(f"[{N},{F}] sum", {"axis 1": lambda: call("nnhipReduceAxesForward", 0, orow, None, X, 2, sh2, full, i32(0, 1), st),
                                     "axis 0": lambda: call("nnhipReduceAxesForward", 0, ocol, None, X, 2, sh2, full, i32(1, 0), st),
                                     "var axis 1": lambda: call("nnhipReduceAxesForward", 2, orow, None, X, 2, sh2, full, i32(0, 1), st),
                                     "torch axis 1": lambda: torch.sum(X, 1, out=orow), "torch axis 0": lambda: torch.sum(X, 0, out=ocol)},
                  nbytes={k: 4.0 * N * F for k in ("axis 1", "axis 0", "var axis 1", "torch axis 1", "torch axis 0")})
        G = randn(N, F)
        drow, dcol = torch.empty(F, device=dev), torch.empty(N, 1, device=dev)

        def unfused(dst, axis):
            call("nnhipMul", O, G, X, N * F, st)
            call("nnhipReduceAxesForward", 0, dst, None, O, 2, sh2, full, i32(*axis), st)

        alternate(f"[{N},{F}] dB of a*b", {"fused [F]": lambda: call("nnhipBroadcastBinaryBackward", 2, None, drow, G, X, row, 0.0, 2, sh2, full, srow, st),
                                           "unfused [F]": lambda: unfused(drow, (1, 0)),
                                           "fused [N,1]": lambda: call("nnhipBroadcastBinaryBackward", 2, None, dcol, G, X, col, 0.0, 2, sh2, full, scol, st),
                                           "unfused [N,1]": lambda: unfused(dcol, (0, 1))},
                  nbytes={"fused [F]": 8.0 * N * F, "unfused [F]": 16.0 * N * F, "fused [N,1]": 8.0 * N * F, "unfused [N,1]": 16.0 * N * F})
        del X, X2, O, G
        shp = (64, 256, 56, 56)
        X4, oc = randn(*shp), torch.empty(256, device=dev)
        alternate("[64,256,56,56] sum (0,2,3)", {"general tier": lambda: call("nnhipReduceAxesForward", 0, oc, None, X4, 4, i64(*shp),
                                                                                i64(256 * 3136, 3136, 56, 1), i32(1, 0, 1, 1), st),
                                                 "torch": lambda: torch.sum(X4, (0, 2, 3), out=oc)},
                  rounds=2, nbytes={"general tier": 4.0 * X4.numel(), "torch": 4.0 * X4.numel()})
        del X4

    if "index" in only:
        # The indexing half of the tape (csrc/tensor_index.hip): every entry beside the torch expression of the same result (written into
        # a preallocated output where torch has an out= form, the bare expression otherwise: never an extra copy) and beside a plain
        # stream of the same footprint (`stream`: the float4 stream tools/stream_roof.py measures, nnhipReLUForward, over as many bytes
        # as the entry moves, half read and half written).
        def i64(*v):
            return (ctypes.c_int64 * max(len(v), 1))(*v)

        def stream_of(nbytes):
            """tools/stream_roof.py's 8 B / element stream over nbytes in all (half each way)."""
            half = int(nbytes // 8)
            s, d = torch.zeros(half, device=dev), torch.empty(half, device=dev)
            return lambda: call("nnhipReLUForward", d, s, half, st)

        n = 1 << 26
        A, B, O = randn(n), randn(n), torch.empty(n, device=dev)
        Ob = torch.empty(n, dtype=torch.bool, device=dev)
        C = (A > 0)
        sh, s1 = i64(n), i64(1)
        alternate("compare 2^26", {"nnhipCompare": lambda: call("nnhipCompare", 2, Ob, A, B, 0.0, 0, 0, 0, 1, sh, s1, s1, st),
                                   "torch": lambda: torch.gt(A, B, out=Ob), "stream": stream_of(9.0 * n)},
                  rounds=3, nbytes={k: 9.0 * n for k in ("nnhipCompare", "torch", "stream")})
        alternate("where 2^26", {"nnhipWhereForward": lambda: call("nnhipWhereForward", O, C, 3, A, B, 0.0, 0.0, 1, sh, s1, s1, s1, st),
                                 "torch": lambda: torch.where(C, A, B, out=O), "stream": stream_of(13.0 * n)},
                  rounds=3, nbytes={k: 13.0 * n for k in ("nnhipWhereForward", "torch", "stream")})
        del A, B, O, Ob, C
        # the notebook's masked scores: where(mask[:, None] == 0, -1e9, scores), scores [64,8,256,256], mask [64,1,256,256]
        shp, ms = (64, 8, 256, 256), (64, 1, 256, 256)
        S, G = randn(*shp), randn(*shp)
        Mk = (torch.rand(*ms, device=dev, generator=g) < 0.2)
        O, dS = torch.empty_like(S), torch.empty_like(S)
        neg, zero = torch.tensor(-1e9, device=dev), torch.zeros((), device=dev)
        ne = S.numel()
        sh4, full4, sm4 = i64(*shp), i64(8 * 65536, 65536, 256, 1), i64(65536, 0, 256, 1)
        alternate("where [64,8,256,256] mask [64,1,..]",
                  {"fwd": lambda: call("nnhipWhereForward", O, Mk, 3, None, S, -1e9, 0.0, 4, sh4, sm4, None, full4, st),
                   "torch fwd": lambda: torch.where(Mk, neg, S, out=O),
                   "bwd": lambda: call("nnhipWhereBackward", None, dS, G, Mk, 3, 4, sh4, sm4, None, full4, st),
                   "torch bwd": lambda: torch.where(Mk, zero, G, out=dS),
                   "stream": stream_of(8.125 * ne)},
                  rounds=3, nbytes={k: 8.125 * ne for k in ("fwd", "torch fwd", "bwd", "torch bwd", "stream")})
        del S, G, Mk, O, dS
        # x[:, -1], x[:, ::2] and flip(1) on [64, 256, 512]
        Bx, Tx, Dx = 64, 256, 512
        X = randn(Bx, Tx, Dx)
        cs = (Tx * Dx, Dx, 1)
        last, dlast = torch.empty(Bx, Dx, device=dev), randn(Bx, Dx)
        half, dhalf = torch.empty(Bx, Tx // 2, Dx, device=dev), randn(Bx, Tx // 2, Dx)
        FX, dX = torch.empty_like(X), torch.empty_like(X)
        nx = X.numel()
        alternate("x[:, -1] [64,256,512]",
                  {"fwd": lambda: call("nnhipSliceForward", last, X, (Tx - 1) * Dx, 0, 2, i64(Bx, Dx), i64(cs[0], 1), st),
                   "torch fwd": lambda: last.copy_(X[:, -1]),
                   "bwd": lambda: call("nnhipSliceBackward", dX, dlast, 3, i64(Bx, Tx, Dx), i64(0, Tx - 1, 0), i64(1, 1, 1), i64(Bx, 1, Dx), st),
                   "torch bwd": lambda: (dX.zero_(), dX[:, -1].copy_(dlast)),
                   "stream bwd": stream_of(4.0 * nx)},
                  rounds=3, nbytes={"fwd": 8.0 * Bx * Dx, "torch fwd": 8.0 * Bx * Dx, "bwd": 4.0 * nx, "torch bwd": 4.0 * nx, "stream bwd": 4.0 * nx})
        alternate("x[:, ::2] [64,256,512]",
                  {"fwd": lambda: call("nnhipSliceForward", half, X, 0, 0, 3, i64(Bx, Tx // 2, Dx), i64(cs[0], 2 * Dx, 1), st),
                   "torch fwd": lambda: half.copy_(X[:, ::2]),
                   "bwd": lambda: call("nnhipSliceBackward", dX, dhalf, 3, i64(Bx, Tx, Dx), i64(0, 0, 0), i64(1, 2, 1), i64(Bx, Tx // 2, Dx), st),
                   "torch bwd": lambda: (dX.zero_(), dX[:, ::2].copy_(dhalf)),
                   "stream fwd": stream_of(4.0 * nx), "stream bwd": stream_of(6.0 * nx)},
                  rounds=3, nbytes={"fwd": 4.0 * nx, "torch fwd": 4.0 * nx, "bwd": 6.0 * nx, "torch bwd": 6.0 * nx, "stream fwd": 4.0 * nx,
                                    "stream bwd": 6.0 * nx})
        alternate("flip(1) [64,256,512]",
                  {"fwd": lambda: call("nnhipSliceForward", FX, X, (Tx - 1) * Dx, 0, 3, i64(Bx, Tx, Dx), i64(cs[0], -Dx, 1), st),
                   "torch": lambda: torch.flip(X, (1,)), "stream": stream_of(8.0 * nx)},
                  rounds=3, nbytes={k: 8.0 * nx for k in ("fwd", "torch", "stream")})
        del X, FX, dX, half, dhalf
        # a row gather: 16384 ids from a 15000-row table of 512 floats, beside nnhipEmbeddingForward without pe
        V, Dm, Ni = 15000, 512, 16384
        W = randn(V, Dm)
        ids = torch.randint(0, V, (Ni,), device=dev, dtype=torch.int32, generator=g)
        out, dW, gO = torch.empty(Ni, Dm, device=dev), torch.empty(V, Dm, device=dev), randn(Ni, Dm)
        p1 = (ctypes.c_void_p * 4)(ids.data_ptr(), 0, 0, 0)
        gb = 8.0 * Ni * Dm
        alternate("rows [15000,512][16384 ids]",
                  {"nnhipIndexGather": lambda: call("nnhipIndexGather", out, W, 0, p1, 1, 1, i64(V), 1, Ni, Dm, st),
                   "nnhipEmbeddingForward": lambda: call("nnhipEmbeddingForward", out, W, ids, None, Ni, Dm, Ni, V, 1.0, st),
                   "torch": lambda: torch.index_select(W, 0, ids, out=out),
                   "bwd nnhipIndexAssign": lambda: call("nnhipIndexAssign", dW, gO, 0.0, 0, 0, 0, 1, p1, 1, 1, i64(V), 1, Ni, Dm, st),
                   "bwd nnhipEmbeddingBackward": lambda: call("nnhipEmbeddingBackward", dW, gO, ids, Ni, Dm, V, 1.0, st),
                   "stream": stream_of(gb)},
                  rounds=3, nbytes={"nnhipIndexGather": gb, "nnhipEmbeddingForward": gb, "torch": gb, "bwd nnhipIndexAssign": 8.0 * V * Dm,
                                    "bwd nnhipEmbeddingBackward": 8.0 * V * Dm, "stream": gb})
        del W, out, dW, gO
        # the element gather logp[arange(N), y] on [16384, 15000], forward and backward (the backward writes all of dX)
        Nr, Cc = 16384, 15000
        L = randn(Nr, Cc)
        ar = torch.arange(Nr, device=dev, dtype=torch.int64)
        y = torch.randint(0, Cc, (Nr,), device=dev, dtype=torch.int64, generator=g)
        pick, gp, dL = torch.empty(Nr, device=dev), randn(Nr), torch.empty_like(L)
        p2 = (ctypes.c_void_p * 4)(ar.data_ptr(), y.data_ptr(), 0, 0)
        nl = L.numel()
        alternate("elements [16384,15000][arange, y]",
                  {"fwd": lambda: call("nnhipIndexGather", pick, L, 0, p2, 2, 2, i64(Nr, Cc), 1, Nr, 1, st),
                   "torch fwd": lambda: L[ar, y],
                   "bwd": lambda: call("nnhipIndexAssign", dL, gp, 0.0, 0, 0, 0, 1, p2, 2, 2, i64(Nr, Cc), 1, Nr, 1, st),
                   "torch bwd": lambda: (dL.zero_(), dL.index_put_((ar, y), gp)),
                   "stream bwd": stream_of(4.0 * nl)},
                  rounds=2, nbytes={"fwd": 12.0 * Nr, "torch fwd": 12.0 * Nr, "bwd": 4.0 * nl, "torch bwd": 4.0 * nl, "stream bwd": 4.0 * nl})
        del L, dL

    if "logsoftmax" in only:
        # nnhipLogSoftmaxForward / Backward beside nnhipSoftmaxForward / Backward (csrc/rowops.hip): the same tiers and the same bytes
        for (rows, cols) in [(8192, 1024), (16384, 15000), (64, 50000)]:
            X, dY, Y, dX = randn(rows, cols), randn(rows, cols), torch.empty(rows, cols, device=dev), torch.empty(rows, cols, device=dev)
            fb, bb = 8.0 * rows * cols, 12.0 * rows * cols
            alternate(f"fwd {rows}x{cols}", {"softmax": lambda: call("nnhipSoftmaxForward", Y, X, rows, cols, 1, st),
                                             "logsoftmax": lambda: call("nnhipLogSoftmaxForward", Y, X, rows, cols, 1, st)},
                      nbytes={"softmax": fb, "logsoftmax": fb})
            call("nnhipLogSoftmaxForward", Y, X, rows, cols, 1, st)
            alternate(f"bwd {rows}x{cols}", {"softmax": lambda: call("nnhipSoftmaxBackward", dX, dY, Y, rows, cols, 1, st),
                                             "logsoftmax": lambda: call("nnhipLogSoftmaxBackward", dX, dY, Y, rows, cols, 1, st)},
                      nbytes={"softmax": bb, "logsoftmax": bb})
            del X, dY, Y, dX

    if "nll" in only:
        # The loss and backward of NLLLoss(LogSoftmax(x)) from the log-probabilities Y on: the fold (nnhipNLLLossForwardBackward with
        # pos_grad only, then nnhipLogSoftmaxNLLBackward: Y read once, dX written once) beside the unfolded pair (the NLL entry with
        # its dense gradient, then nnhipLogSoftmaxBackward: the dense gradient zero-filled and written, read back with Y, dX written --
        # 5 streams of N C floats where the fold moves 2) and beside nnhipCrossEntropyLossEx from the logits (forward included: X read,
        # the gradient written).
        rows, cols = 16384, 15000
        X = randn(rows, cols)
        Y, dX, dlogp = torch.empty_like(X), torch.empty_like(X), torch.empty_like(X)
        call("nnhipLogSoftmaxForward", Y, X, rows, cols, 1, st)
        labels = torch.randint(0, cols, (rows,), device=dev, dtype=torch.int32, generator=g)
        loss, pg = torch.empty((), device=dev), torch.empty(rows, device=dev)
        loss_rows, lse, count = torch.empty(rows, device=dev), torch.empty(rows, device=dev), torch.empty(1, dtype=torch.int32, device=dev)

        def fold():
            call("nnhipNLLLossForwardBackward", Y, labels, 4, None, -100, rows, cols, 1, b"m", loss, None, pg, st)
            call("nnhipLogSoftmaxNLLBackward", dX, Y, labels, 4, pg, None, rows, cols, st)

        def pair():
            call("nnhipNLLLossForwardBackward", Y, labels, 4, None, -100, rows, cols, 1, b"m", loss, dlogp, None, st)
            call("nnhipLogSoftmaxBackward", dX, dlogp, Y, rows, cols, 1, st)

        def fused_ce():
            call("nnhipCrossEntropyLossEx", X, dX, loss_rows, lse, labels, 4, None, cols, -100, rows, cols, b"m", loss, count, st)

        nc = 4.0 * rows * cols
        alternate(f"{rows}x{cols}", {"fold": fold, "pair": pair, "crossentropy": fused_ce},
                  nbytes={"fold": 2 * nc, "pair": 5 * nc, "crossentropy": 2 * nc})
        del X, Y, dX, dlogp

    if "gradnorm" in only:        # the one-launch global gradient norm (csrc/grad_norm.hip) on three parameter lists, beside a read-only
        #                            stream of the same bytes and torch's clip_grad_norm_; then the C4 step in graph mode, armed / unarmed
        sys.path.insert(0, os.path.join(ROOT, "examples"))
        import gpt_tiny
        import neunet_hip
        import neunet_hip.nn as nn
        from neunet_hip.distributed import GradBucket
        from neunet_hip.graph import GraphedTrainStep
        from neunet_hip.optim import Adam
        cast = lambda a, t: ctypes.cast(a, ctypes.POINTER(t))  # noqa: E731
        np.random.seed(1004)
        c4 = dict(vocab=15000, d_model=512, n_heads=8, d_ff=2048, n_layers=6, seq=256)      # bench.py: C4

        def c4_model():
            model = gpt_tiny.build_gpt(c4["vocab"], c4["d_model"], c4["n_heads"], c4["d_ff"], c4["n_layers"], pad_idx=0, max_len=1024, fused=True)
            ids_h = np.random.default_rng(4000).integers(3, c4["vocab"], (64, c4["seq"] + 1)).astype(np.int32)
            ids = neunet_hip.Tensor(np.ascontiguousarray(ids_h[:, :-1]), dtype=np.int32, requires_grad=False, device="cuda")
            tgt = neunet_hip.Tensor(np.ascontiguousarray(ids_h[:, 1:]).reshape(-1), dtype=np.int32, requires_grad=False, device="cuda")
            loss_fn = nn.CrossEntropyLoss(ignore_index=0)

            def fwd_bwd():
                out, _ = model.forward(ids)
                loss = loss_fn(out.reshape(out.shape[0] * out.shape[1], out.shape[2]), tgt)
                loss.backward()
                return loss

            return model, fwd_bwd

        model, fwd_bwd = c4_model()
        fwd_bwd()                                                    # which parameters receive gradients (cross_attn never does)
        c4_shapes = [tuple(p.data.shape) for p in model.parameters() if p.grad is not None]
        del model, fwd_bwd
        lists = {"C4 parameter list": c4_shapes, "one tensor 2^26": [(1 << 26,)], "README MLP": [(128, 784), (128,), (10, 128), (10,)]}
        opt = _lib.load_hip_function("nnhipCreateFusedOptimizer")()
        for tag, shapes in lists.items():
            gs = [randn(*s) for s in shapes]
            nt, numel = len(gs), sum(t.numel() for t in gs)
            flat = torch.cat([t.reshape(-1) for t in gs])            # the same bytes as one buffer: the read-only stream
            ptrs = (ctypes.c_void_p * nt)(*[t.data_ptr() for t in gs])
            sizes = (ctypes.c_int64 * nt)(*[t.numel() for t in gs])
            words = torch.zeros(4, device=dev)
            holders = [torch.nn.Parameter(torch.zeros(1, device=dev)) for _ in gs]
            for h, t in zip(holders, gs):
                h.data, h.grad = t, t.clone()
            name = f"{tag} ({nt} tensors, {numel} el)"
            for norm_id, ntag in ((0, "L2"), (1, "inf")):
                report(f"gradnorm {ntag} {name}", *bench(lambda: call("nnhipGradNormMultiTensor", opt, nt, cast(ptrs, ctypes.c_void_p),
                                                                        cast(sizes, ctypes.c_int64), norm_id, 1.0, None, 1, 1.0, words, st), args.iters), nbytes=4.0 * numel)
            report(f"read-only stream (torch.sum) {name}", *bench(lambda: torch.sum(flat), args.iters), nbytes=4.0 * numel)
            report(f"torch clip_grad_norm_ {name}", *bench(lambda: torch.nn.utils.clip_grad_norm_(holders, 1e30), args.iters), nbytes=4.0 * numel)
            report(f"scale in place {name}", *bench(lambda: call("nnhipScaleMultiTensor", opt, nt, cast(ptrs, ctypes.c_void_p), cast(sizes, ctypes.c_int64),
                                                                 words[1:2], st), args.iters), nbytes=8.0 * numel)
            del gs, flat, holders
        _lib.load_hip_function("nnhipDestroyFusedOptimizer")(opt)
        for armed in (False, True, False, True):                     # alternated: the second pair shows the run-to-run spread
            np.random.seed(1004)
            model, fwd_bwd = c4_model()
            adam = Adam(model.parameters(), lr=1.5e-4, betas=(0.9, 0.98), eps=1e-9)
            adam.max_grad_norm = 1.0 if armed else None
            fwd_bwd()
            active = [p for p in model.parameters() if p.grad is not None]
            adam.zero_grad()
            gstep = GraphedTrainStep(fwd_bwd, adam, GradBucket(active, extra_scalars=1), warmup=2, count_nodes=True)
            report(f"C4 step, graph, {'armed (max_grad_norm 1.0)' if armed else 'unarmed'}: {gstep.kernel_nodes} kernels",
                   *bench(lambda: gstep(), args.iters))
            if armed:
                print(f"    grad norm {adam.last_grad_norm.item():.4f}  divisor {adam._clip_words[1].item():.4f}", flush=True)
            gstep.release()
            del gstep, adam, model, fwd_bwd, active
            torch.cuda.empty_cache()

    if want("conv"):
        for (B, Cin, H, Cout) in [(256, 1, 28, 8), (256, 8, 14, 16)]:
            X = rnd(B, Cin, H, H)
            W = rnd(Cout, Cin, 3, 3)
            bb = rnd(Cout)
            O_ = torch.empty(B, Cout, H, H, device=dev)
            dO = rnd(B, Cout, H, H)
            dX, dW, db = torch.empty_like(X), torch.empty_like(W), torch.empty_like(bb)
            d = Conv2dDesc(B, Cin, H, H, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
            by = 4.0 * (X.numel() + O_.numel() + W.numel())
            report(f"conv fwd {B}x{Cin}x{H}x{H}->{Cout}", *bench(lambda: call("nnhipConv2dForward", X, W, bb, O_, ctypes.byref(d), st), args.iters), nbytes=by)
            report(f"conv bwd {B}x{Cin}x{H}x{H}->{Cout}", *bench(lambda: call("nnhipConv2dBackward", X, W, dO, dX, dW, db, ctypes.byref(d), st), args.iters), nbytes=by * 2)


if __name__ == "__main__":
    main()
