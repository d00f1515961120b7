// batchnorm1d.hip -- BatchNorm1d on X [N, F], row-major fp32 (neunet/nn/layers/batchnorm1d.py:46-99 forward, 15-41 backward): the
// layer between every pair of Linears of the reference's GAN / VAE / VQ-VAE MLPs (examples/gan.ipynb, examples/vae.ipynb).
//
// The BatchNorm2d kernels (pool_norm.hip) give a 1024-thread block to one channel and let the lanes of a wave walk the HW contiguous
// floats of one image; at HW = 1 that is one live lane per wave, one cache line per element and F blocks.  Here the block is
// turned on its side: FEATURES go along the lanes, so a wave load is a run of contiguous floats of one row, and ROWS go across
// lane groups and waves.  A block owns a strip of BN1_SW features; the 64 lanes of a wave are 64 / BN1_SW row groups of BN1_SW
// features, so the block holds BN1_RG = 16 * 64 / BN1_SW row slots and thread (slot, fl) takes rows slot, slot + BN1_RG, ... of
// feature strip * BN1_SW + fl.  A column is never split across blocks: N >> 10^4 with a handful of features is a few blocks
// walking long columns -- slow by construction (include/neunet_hip.h says so).
//
// Column sums: one accumulator per thread over its rows (a chain), then the lane groups of a wave are folded with xor shuffles
// (lanes fl, fl + SW, ... hold the same feature), then the sixteen waves' partials go through LDS and every thread adds them in
// wave order 0..15 -- a fixed order, no atomics, no workspace: reruns are bit-identical and the launch is legal in a stream capture.
//
// Two tiers behind bn1_fits_regs(): up to BN1_NE rows per thread the strip's column segment stays in registers between the
// passes (one read of X per direction); beyond, the looped kernels re-read it from L2 / HBM in the second and third pass and
// index in 64 bits.
#include <math.h>

#include "common.h"

namespace nnhip {

#ifndef BN1_STRIP
#define BN1_STRIP 16
#endif
constexpr int BN1_SW = BN1_STRIP;                   // features per block (strip width): 16, 32 or 64
constexpr int BN1_NW = 16;                          // waves per block
constexpr int BN1_LG = 64 / BN1_SW;                 // row groups per wave
constexpr int BN1_RG = BN1_NW * BN1_LG;             // row slots per block
constexpr int BN1_NE = 16;                          // rows per thread in the register tier
static_assert(BN1_SW == 16 || BN1_SW == 32 || BN1_SW == 64, "strip width");

// Register tier: every row has a slot (N <= BN1_RG * BN1_NE = 1024 rows at the default strip) and the byte offset the buffer loads
// take, (row * F + fl) * 4 in 32 bits, cannot wrap: N * F <= 2^29 floats (the bound bn_fits_fused() of pool_norm.hip has for the
// same reason).  Everything else takes the looped kernels.
static inline bool bn1_fits_regs(int64_t N, int64_t F) {
    return N <= (int64_t)BN1_RG * BN1_NE && N * F <= ((int64_t)1 << 29);
}

// The strips are laid over a 2-d grid: HIP wraps a grid of more than 2^32 threads along one axis silently (a 2^28-feature input
// is 2^24 blocks of 1024 threads), so x carries at most BN1_GX strips and y the rest; a block past the last strip has no live lane.
constexpr unsigned BN1_GX = 1u << 20;
static inline dim3 bn1_grid(int64_t F) {
    const int64_t strips = ceil_div(F, BN1_SW);
    return strips <= BN1_GX ? dim3((unsigned)strips) : dim3(BN1_GX, (unsigned)ceil_div(strips, BN1_GX));
}
struct Bn1Thread {
    int slot, fl, f;        // first row of this thread, feature within the strip, feature
    int64_t base;           // the strip's first feature
    bool col;               // f < F
};
__device__ __forceinline__ Bn1Thread bn1_thread(int F) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Bn1Thread t;
    t.fl = lane & (BN1_SW - 1);
    t.slot = wave * BN1_LG + lane / BN1_SW;
    t.base = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * BN1_SW;
    t.col = t.base + t.fl < F;
    t.f = t.col ? (int)(t.base + t.fl) : 0;
    return t;
}

// Column sum over the block: every thread of feature fl gets the same bits.  `red` is BN1_NW * BN1_SW floats.
__device__ __forceinline__ float bn1_colsum(float v, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = BN1_SW; o < 64; o <<= 1) v += __shfl_xor(v, o);
    __syncthreads();                                 // protect `red` against a previous use
    if (lane < BN1_SW) red[wave * BN1_SW + lane] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < BN1_NW; ++i) s += red[i * BN1_SW + (lane & (BN1_SW - 1))];
    return s;
}
// Two column sums with one pair of barriers.  `red` is 2 * BN1_NW * BN1_SW floats.
__device__ __forceinline__ void bn1_colsum2(float& a, float& b, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = BN1_SW; o < 64; o <<= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    __syncthreads();
    if (lane < BN1_SW) { red[wave * BN1_SW + lane] = a; red[(BN1_NW + wave) * BN1_SW + lane] = b; }
    __syncthreads();
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < BN1_NW; ++i) {
        sa += red[i * BN1_SW + (lane & (BN1_SW - 1))];
        sb += red[(BN1_NW + i) * BN1_SW + (lane & (BN1_SW - 1))];
    }
    a = sa;
    b = sb;
}

// ---- register tier ---------------------------------------------------------------------------------------------------------
// loads through a buffer descriptor (strip base in SGPRs + a 32-bit byte offset per element), as bn_ld() of pool_norm.hip: 32
// plain global loads in flight would hold 32 64-bit address pairs.  off < 0: no element -> 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bn1_rsrc(const float* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, 0xFFFFFFFF, 0x00020000);
}
__device__ __forceinline__ float bn1_ld(__amdgpu_buffer_rsrc_t rs, int off) {
    const float v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (off >= 0 ? off : 0) * 4, 0, 0));
    return off >= 0 ? v : 0.f;
}
// off[e]: element offset of row slot + BN1_RG * e from the strip's first element, or -1 (row >= N, or feature >= F)
__device__ __forceinline__ void bn1_offsets(int (&off)[BN1_NE], const Bn1Thread& t, int N, int F) {
#pragma unroll
    for (int e = 0; e < BN1_NE; ++e) {
        const int r = t.slot + BN1_RG * e;
        off[e] = (t.col && r < N) ? r * F + t.fl : -1;
    }
}

__global__ __launch_bounds__(1024) void bn1_fwd_reg_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ mean_out, float* __restrict__ inv_out,
                                                           float* __restrict__ run_mean, float* __restrict__ run_var, int N, int F,
                                                           float eps, float momentum) {
    __shared__ float red[BN1_NW * BN1_SW];
    const Bn1Thread t = bn1_thread(F);
    if (t.base >= F) return;                                  // a block of the 2-d grid past the last strip (uniform: before any barrier)
    const float n = (float)N;
    const __amdgpu_buffer_rsrc_t rx = bn1_rsrc(x + t.base);
    float* __restrict__ ys = y + t.base;
    int off[BN1_NE];
    bn1_offsets(off, t, N, F);
    float v[BN1_NE];
#pragma unroll
    for (int e = 0; e < BN1_NE; ++e) v[e] = bn1_ld(rx, off[e]);       // every load issued before the first value is used
    __builtin_amdgcn_sched_barrier(0);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < BN1_NE; ++e) s += v[e];
    const float mean = bn1_colsum(s, red) / n;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < BN1_NE; ++e)
        if (off[e] >= 0) { const float d = v[e] - mean; q += d * d; }
    const float var = bn1_colsum(q, red) / n;
    const float inv = 1.0f / sqrtf(var + eps);
    if (t.slot == 0 && t.col) {
        mean_out[t.f] = mean;
        inv_out[t.f] = inv;
        if (run_mean) {
            run_mean[t.f] = momentum * run_mean[t.f] + (1.0f - momentum) * mean;
            run_var[t.f] = momentum * run_var[t.f] + (1.0f - momentum) * var;
        }
    }
    float wc = 1.f, bc = 0.f;
    if (w && t.col) { wc = w[t.f]; bc = bias[t.f]; }
#pragma unroll
    for (int e = 0; e < BN1_NE; ++e)
        if (off[e] >= 0) {
            float u = (v[e] - mean) * inv;
            if (w) u = wc * u + bc;
            ys[off[e]] = u;
        }
}

// grad_X = (1/N) w inv (N g - sum g - xc inv^2 sum(g xc));  dW = sum(g xc inv) = inv sum(g xc);  db = sum g   (batchnorm1d.py:18-36)
__global__ __launch_bounds__(1024) void bn1_bwd_reg_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                           const float* __restrict__ mean, const float* __restrict__ inv,
                                                           const float* __restrict__ w, float* __restrict__ dx,
                                                           float* __restrict__ dw, float* __restrict__ db, int N, int F, float invN) {
    __shared__ float red[2 * BN1_NW * BN1_SW];
    const Bn1Thread t = bn1_thread(F);
    if (t.base >= F) return;                                  // a block of the 2-d grid past the last strip (uniform: before any barrier)
    float m = 0.f, iv = 0.f, wc = 1.f;
    if (t.col) { m = mean[t.f]; iv = inv[t.f]; if (w) wc = w[t.f]; }
    const __amdgpu_buffer_rsrc_t rg = bn1_rsrc(g + t.base), rx = bn1_rsrc(x + t.base);
    float* __restrict__ ds = dx + t.base;
    int off[BN1_NE];
    bn1_offsets(off, t, N, F);
    float gv[BN1_NE], xc[BN1_NE];
    // every load is issued before the first value is used (see bn_bwd_fused_kernel in pool_norm.hip: a select around the load put
    // it under a branch that ended in s_waitcnt vmcnt(0), one memory round trip per element)
#pragma unroll
    for (int e = 0; e < BN1_NE; ++e) {
        gv[e] = bn1_ld(rg, off[e]);                           // 0 for a slot without an element: both sums take 0
        xc[e] = bn1_ld(rx, off[e]);
    }
    __builtin_amdgcn_sched_barrier(0);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < BN1_NE; ++e) {
        xc[e] = off[e] >= 0 ? xc[e] - m : 0.f;
        s1 += gv[e] * xc[e];
        s2 += gv[e];
    }
    bn1_colsum2(s1, s2, red);
    if (t.slot == 0 && t.col && dw) { dw[t.f] = s1 * iv; db[t.f] = s2; }
    const float k = wc * iv, c2 = s2 * invN, c3 = iv * iv * s1 * invN;
#pragma unroll
    for (int e = 0; e < BN1_NE; ++e)
        if (off[e] >= 0) ds[off[e]] = k * (gv[e] - c2 - xc[e] * c3);
}

// ---- looped tier: any N; 64-bit indices; X is read again in every pass ---------------------------------------------------------
// TRAIN = false is the eval forward: the same entry without the reduction (mean / var from the running statistics).
template <bool TRAIN>
__global__ __launch_bounds__(1024) void bn1_fwd_loop_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ mean_out, float* __restrict__ inv_out,
                                                            float* __restrict__ run_mean, float* __restrict__ run_var, int N, int F,
                                                            float eps, float momentum) {
    __shared__ float red[BN1_NW * BN1_SW];
    const Bn1Thread t = bn1_thread(F);
    if (t.base >= F) return;                                  // a block of the 2-d grid past the last strip (uniform: before any barrier)
    const int rows = t.col ? N : 0;                           // a lane past the last feature walks no rows but meets every barrier
    const float* __restrict__ xc_ = x + t.f;
    float mean, inv;
    if constexpr (TRAIN) {
        const float n = (float)N;
        float s = 0.f;
#pragma unroll 4
        for (int64_t r = t.slot; r < rows; r += BN1_RG) s += xc_[r * F];
        mean = bn1_colsum(s, red) / n;
        float q = 0.f;
#pragma unroll 4
        for (int64_t r = t.slot; r < rows; r += BN1_RG) { const float d = xc_[r * F] - mean; q += d * d; }
        const float var = bn1_colsum(q, red) / n;
        inv = 1.0f / sqrtf(var + eps);
        if (t.slot == 0 && t.col && run_mean) {
            run_mean[t.f] = momentum * run_mean[t.f] + (1.0f - momentum) * mean;
            run_var[t.f] = momentum * run_var[t.f] + (1.0f - momentum) * var;
        }
    } else {
        mean = t.col ? run_mean[t.f] : 0.f;
        inv = t.col ? 1.0f / sqrtf(run_var[t.f] + eps) : 0.f;
    }
    if (t.slot == 0 && t.col) { mean_out[t.f] = mean; inv_out[t.f] = inv; }
    float wc = 1.f, bc = 0.f;
    if (w && t.col) { wc = w[t.f]; bc = bias[t.f]; }
    float* __restrict__ yc_ = y + t.f;
#pragma unroll 4
    for (int64_t r = t.slot; r < rows; r += BN1_RG) {
        float u = (xc_[r * F] - mean) * inv;
        if (w) u = wc * u + bc;
        yc_[r * F] = u;
    }
}

__global__ __launch_bounds__(1024) void bn1_bwd_loop_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ inv,
                                                            const float* __restrict__ w, float* __restrict__ dx,
                                                            float* __restrict__ dw, float* __restrict__ db, int N, int F, float invN) {
    __shared__ float red[2 * BN1_NW * BN1_SW];
    const Bn1Thread t = bn1_thread(F);
    if (t.base >= F) return;                                  // a block of the 2-d grid past the last strip (uniform: before any barrier)
    const int rows = t.col ? N : 0;
    float m = 0.f, iv = 0.f, wc = 1.f;
    if (t.col) { m = mean[t.f]; iv = inv[t.f]; if (w) wc = w[t.f]; }
    const float* __restrict__ gc_ = g + t.f;
    const float* __restrict__ xc_ = x + t.f;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
    for (int64_t r = t.slot; r < rows; r += BN1_RG) {
        const float gg = gc_[r * F], xc = xc_[r * F] - m;
        s1 += gg * xc;
        s2 += gg;
    }
    bn1_colsum2(s1, s2, red);
    if (t.slot == 0 && t.col && dw) { dw[t.f] = s1 * iv; db[t.f] = s2; }
    const float k = wc * iv, c2 = s2 * invN, c3 = iv * iv * s1 * invN;
    float* __restrict__ dc_ = dx + t.f;
#pragma unroll 4
    for (int64_t r = t.slot; r < rows; r += BN1_RG) {
        const float gg = gc_[r * F], xc = xc_[r * F] - m;
        dc_[r * F] = k * (gg - c2 - xc * c3);
    }
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipBatchNorm1dForward(const float* X, const float* weight, const float* bias, float* Y, float* save_mean,
                                       float* save_inv, float* running_mean, float* running_var, int64_t N, int64_t F, float eps,
                                       float momentum, int training, nnhipStream_t s) {
    NNHIP_CHECK_ARG(N >= 1 && F >= 1 && N < ((int64_t)1 << 31) && F < ((int64_t)1 << 31), NNHIP_EINVAL,
                    "nnhipBatchNorm1dForward: bad sizes (1 <= N < 2^31, 1 <= F < 2^31)");
    NNHIP_CHECK_ARG(X && Y && save_mean && save_inv, NNHIP_EINVAL, "nnhipBatchNorm1dForward: null pointer");
    NNHIP_CHECK_ARG((weight == nullptr) == (bias == nullptr), NNHIP_EINVAL, "nnhipBatchNorm1dForward: weight and bias go together");
    NNHIP_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), NNHIP_EINVAL,
                    "nnhipBatchNorm1dForward: running_mean and running_var go together");
    NNHIP_CHECK_ARG(training || (running_mean && running_var), NNHIP_EINVAL, "nnhipBatchNorm1dForward: eval needs running stats");
    hipStream_t st = (hipStream_t)s;
    const dim3 grid = bn1_grid(F), block(64 * BN1_NW);
    if (!training) {
        hipLaunchKernelGGL(bn1_fwd_loop_kernel<false>, grid, block, 0, st, X, Y, weight, bias, save_mean, save_inv, running_mean,
                           running_var, (int)N, (int)F, eps, momentum);
        NNHIP_LAUNCH_CHECK("bn1_fwd_loop_kernel<eval>");
    } else if (bn1_fits_regs(N, F)) {
        hipLaunchKernelGGL(bn1_fwd_reg_kernel, grid, block, 0, st, X, Y, weight, bias, save_mean, save_inv, running_mean, running_var,
                           (int)N, (int)F, eps, momentum);
        NNHIP_LAUNCH_CHECK("bn1_fwd_reg_kernel");
    } else {
        hipLaunchKernelGGL(bn1_fwd_loop_kernel<true>, grid, block, 0, st, X, Y, weight, bias, save_mean, save_inv, running_mean,
                           running_var, (int)N, (int)F, eps, momentum);
        NNHIP_LAUNCH_CHECK("bn1_fwd_loop_kernel");
    }
    return 0;
}

extern "C" int nnhipBatchNorm1dBackward(const float* dY, const float* X, const float* weight, const float* save_mean,
                                        const float* save_inv, float* dX, float* dW, float* db, int64_t N, int64_t F,
                                        nnhipStream_t s) {
    NNHIP_CHECK_ARG(N >= 1 && F >= 1 && N < ((int64_t)1 << 31) && F < ((int64_t)1 << 31), NNHIP_EINVAL,
                    "nnhipBatchNorm1dBackward: bad sizes (1 <= N < 2^31, 1 <= F < 2^31)");
    NNHIP_CHECK_ARG(dY && X && save_mean && save_inv && dX, NNHIP_EINVAL, "nnhipBatchNorm1dBackward: null pointer");
    NNHIP_CHECK_ARG((dW == nullptr) == (db == nullptr), NNHIP_EINVAL, "nnhipBatchNorm1dBackward: dW and db go together");
    hipStream_t st = (hipStream_t)s;
    const dim3 grid = bn1_grid(F), block(64 * BN1_NW);
    const float invN = 1.0f / (float)N;
    if (bn1_fits_regs(N, F)) {
        hipLaunchKernelGGL(bn1_bwd_reg_kernel, grid, block, 0, st, dY, X, save_mean, save_inv, weight, dX, dW, db, (int)N, (int)F, invN);
        NNHIP_LAUNCH_CHECK("bn1_bwd_reg_kernel");
    } else {
        hipLaunchKernelGGL(bn1_bwd_loop_kernel, grid, block, 0, st, dY, X, save_mean, save_inv, weight, dX, dW, db, (int)N, (int)F, invN);
        NNHIP_LAUNCH_CHECK("bn1_bwd_loop_kernel");
    }
    return 0;
}
