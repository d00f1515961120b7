// vector_quantize.hip -- what the VQ-VAE example needs besides its layers (examples/vqvae.ipynb, VQVAE.quantize / VQVAE.loss_function):
// the nearest-code search, and vq_loss + beta * commit_loss with both gradients.
//
// nnhipVQNearest.  The notebook writes the search as matmul(z, codebook.T), two row-norm sums, a broadcast add, argmin and an Embedding
// gather: an N x K distance matrix written and read back and about ten launches.  Here it is ONE launch that never holds more of that
// matrix than a lane's registers: a GEMM-shaped pass over the codebook with a running (score, index) minimum for an epilogue, in the
// order of np.argmin (arg_order.h: ties to the lower index, a NaN score beats any number, the first NaN wins).  Two tiers, chosen from
// D alone (NNHIP_VQ_NARROW_MAX_D, include/neunet_hip.h):
//
//   narrow, D <= 8 (the notebook: D = 2).  An MFMA k-extent of 4 would be mostly padding.  One lane per row with the row in registers;
//   the codebook goes through LDS in tiles of VQ_NARROW_CODES codes that every lane reads at the same address (a broadcast, no bank
//   conflict); the score is the DIRECT form sum_j (z_j - e_j)^2 as one subtraction and one fma per component, j rising.
//
//   wide, D > 8.  Exact-fp32 MFMA (16x16x4), operand layout of gemm_small.h: lane (l16, kq) holds 4 consecutive k of row / code l16.
//   A block of VQ_WAVES waves owns VQ_ROWS = 16 rows; every wave keeps the same z operand resident (registers up to
//   D = VQ_WIDE_RESIDENT_D, re-fetched per code tile beyond) and the waves split the codebook: wave w takes the super-tiles
//   w, w + VQ_WAVES, ... of VQ_TILES x 16 codes, one independent accumulator per code tile (four MFMA chains in flight per wave).
//   After a super-tile, accumulator register v of lane (l16, kq) holds z_row(4 kq + v) . e_code(16 t + l16); the score is the
//   EXPANSION |e|^2 - 2 z.e (|z|^2 is constant in a row) as fmaf(-2, acc, norm).  The norms come from the B operand the lane has
//   already loaded: one fma per loaded component in the k-loop, then two cross-lane adds over the four kq lanes per code tile -- the
//   same instruction sequence wherever a code sits, so duplicated codes score bit-identically and the tie rule holds.  Codes arrive
//   in rising index order per lane; the close is a (score, index) reduction over the 16 l16 lanes and then over the waves.
//   k tails (D % 4, D % 16) and rows / codes past the end read zeros through the out-of-range buffer-load idiom of gemm_small.h
//   (sg_rsrc / sg_fetch); codes past K score +inf; rows past N are not written.
//
// Rows are split over blocks and K is NEVER split across blocks: a few rows against a huge codebook is one block walking all of it,
// slow by construction.  No workspace, no atomics, no host synchronisation: legal inside a stream capture, reruns bit-identical.
#include <math.h>

#include "arg_order.h"
#include "common.h"
#include "gemm_small.h"

namespace nnhip {

constexpr int VQ_NARROW_MAX_D = NNHIP_VQ_NARROW_MAX_D;
constexpr int VQ_NARROW_CODES = 512;       // codes per LDS tile of the narrow tier (16 KB at D = 8)
constexpr int VQ_ROWS = 16;                // rows per block of the wide tier: one MFMA tile
constexpr int VQ_WAVES = 4;                // waves per block of the wide tier; they split the codebook
constexpr int VQ_TILES = 4;                // 16-code tiles per super-tile = independent accumulators per wave
constexpr int VQ_WIDE_RESIDENT_D = 256;    // the z operand stays in registers up to here: 16 k-groups = 64 registers per lane
// a wave's buffer offsets reach 16 D floats: beyond this D they no longer fit the 32-bit offset below SG_OOB and the operands are
// fetched through 64-bit addresses instead (same arithmetic, same results)
constexpr int64_t VQ_BUFFER_MAX_D = ((int64_t)1 << 26) - 1;

// ---------------------------------------------------------------------------------------------------------------- narrow tier
template <int D>
__global__ __launch_bounds__(256) void vq_narrow_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                         int32_t* __restrict__ idx, float* __restrict__ zq, int64_t N, int64_t K) {
    __shared__ float tile[VQ_NARROW_CODES * D];
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool mine = row < N;
    float r[D];
#pragma unroll
    for (int j = 0; j < D; ++j) r[j] = mine ? z[row * D + j] : 0.f;
    ArgBest b{INFINITY, 0x7fffffff};
    for (int64_t c0 = 0; c0 < K; c0 += VQ_NARROW_CODES) {
        const int nc = (int)(K - c0 < VQ_NARROW_CODES ? K - c0 : VQ_NARROW_CODES);
        __syncthreads();                                       // the previous tile has been read by every lane
        for (int e = threadIdx.x; e < nc * D; e += 256) tile[e] = cb[c0 * D + e];
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float t = r[j] - tile[c * D + j];
                s = fmaf(t, t, s);
            }
            const int32_t code = (int32_t)(c0 + c);
            if (arg_better_min(s, code, b.v, b.i)) { b.v = s; b.i = code; }
        }
    }
    if (!mine) return;
    idx[row] = b.i;                                            // code 0 beats the initial (+inf, INT_MAX) whatever it scores
    if (zq) {
#pragma unroll
        for (int j = 0; j < D; ++j) zq[row * D + j] = cb[(int64_t)b.i * D + j];
    }
}

// ------------------------------------------------------------------------------------------------------------------ wide tier
// 4 consecutive k (k0 .. k0 + 3) of the lane's row: zeros past D and for a row / code past the end
template <bool VEC, bool FLAT>
__device__ __forceinline__ float4 vq_fetch(__amdgpu_buffer_rsrc_t rs, const float* rowp, unsigned row_off, bool ok, unsigned k0, unsigned D) {
    if constexpr (!FLAT) {
        return sg_fetch<true, VEC>(rs, 0u, row_off, ok, k0, D);
    } else {
        float4 v;
        v.x = (ok && k0 < D) ? rowp[k0] : 0.f;
        v.y = (ok && k0 + 1 < D) ? rowp[k0 + 1] : 0.f;
        v.z = (ok && k0 + 2 < D) ? rowp[k0 + 2] : 0.f;
        v.w = (ok && k0 + 3 < D) ? rowp[k0 + 3] : 0.f;
        return v;
    }
}

// the B side of one k-group of a super-tile: VQ_TILES operand quads, one per 16-code tile
struct VqCodes {
    float4 q[VQ_TILES];
};

// NG > 0: D has exactly NG k-groups (16 (NG - 1) < D <= 16 NG <= VQ_WIDE_RESIDENT_D) and the z operand of all of them is resident;
// NG == 0: any D, every k-group's z quad is fetched again per super-tile.
// VEC: D % 4 == 0 and both operands 16-byte aligned (one 16-byte load per quad).  FLAT: see VQ_BUFFER_MAX_D.
template <int NG, bool VEC, bool FLAT>
__global__ __launch_bounds__(VQ_WAVES * 64) void vq_wide_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                                 int32_t* __restrict__ idx, float* __restrict__ zq, int64_t N,
                                                                 unsigned D, int64_t K) {
    __shared__ float sv[VQ_WAVES][VQ_ROWS];
    __shared__ int32_t si[VQ_WAVES][VQ_ROWS];
    __shared__ int32_t sfin[VQ_ROWS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave-uniform: the buffer descriptors below stay scalar
    const int l16 = lane & 15, kq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * VQ_ROWS;
    const int rows = (int)(N - row0 < VQ_ROWS ? N - row0 : VQ_ROWS);
    const unsigned groups = (D + 15u) >> 4;
    const unsigned row_off = (unsigned)l16 * D * 4u;                     // FLAT: unused (would wrap)
    const bool a_ok = l16 < rows;
    const float* zrow = z + (row0 + (a_ok ? l16 : 0)) * (int64_t)D;
    const __amdgpu_buffer_rsrc_t rsa = sg_rsrc(z + row0 * (int64_t)D, FLAT ? 0u : (unsigned)rows * D * 4u);

    float4 a[NG > 0 ? NG : 1];
    if constexpr (NG > 0) {
#pragma unroll
        for (int g = 0; g < NG; ++g) a[g] = vq_fetch<VEC, FLAT>(rsa, zrow, row_off, a_ok, 16u * g + 4u * kq, D);
    }

    ArgBest best[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) best[v] = ArgBest{INFINITY, 0x7fffffff};

    const int64_t supers = (K + 16 * VQ_TILES - 1) / (16 * VQ_TILES);
    for (int64_t st = wave; st < supers; st += VQ_WAVES) {
        const int64_t code0 = st * (16 * VQ_TILES);
        __amdgpu_buffer_rsrc_t rsb[VQ_TILES];
        const float* crow[VQ_TILES];
        bool b_ok[VQ_TILES];
#pragma unroll
        for (int t = 0; t < VQ_TILES; ++t) {
            const int64_t left = K - (code0 + 16 * t);                   // codes of this tile that exist (<= 0: none)
            const int nc = left >= 16 ? 16 : left > 0 ? (int)left : 0;
            rsb[t] = sg_rsrc(nc > 0 ? cb + (code0 + 16 * t) * (int64_t)D : cb, FLAT ? 0u : (unsigned)nc * D * 4u);
            b_ok[t] = l16 < nc;
            crow[t] = cb + (b_ok[t] ? code0 + 16 * t + l16 : 0) * (int64_t)D;
        }
        sg_f32x4 acc[VQ_TILES];
        float nrm[VQ_TILES];
#pragma unroll
        for (int t = 0; t < VQ_TILES; ++t) { acc[t] = sg_f32x4{0.f, 0.f, 0.f, 0.f}; nrm[t] = 0.f; }

        // one k-group ahead: the loads of group g + 1 are in flight under the 16 MFMAs of group g
        auto fetch_codes = [&](unsigned g) {
            VqCodes c;
#pragma unroll
            for (int t = 0; t < VQ_TILES; ++t) c.q[t] = vq_fetch<VEC, FLAT>(rsb[t], crow[t], row_off, b_ok[t], 16u * g + 4u * kq, D);
            return c;
        };
        auto step = [&](const float4& za, const VqCodes& c) {
#pragma unroll
            for (int t = 0; t < VQ_TILES; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(za.x, c.q[t].x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(za.y, c.q[t].y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(za.z, c.q[t].z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(za.w, c.q[t].w, acc[t], 0, 0, 0);
                nrm[t] = fmaf(c.q[t].w, c.q[t].w, fmaf(c.q[t].z, c.q[t].z, fmaf(c.q[t].y, c.q[t].y, fmaf(c.q[t].x, c.q[t].x, nrm[t]))));
            }
        };
        VqCodes cur = fetch_codes(0);
        if constexpr (NG > 0) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {                             // NG == groups: straight-line code, the buffers rename for free
                VqCodes nxt = cur;
                if (g + 1 < NG) nxt = fetch_codes((unsigned)g + 1);
                __builtin_amdgcn_sched_barrier(0);                       // or the scheduler sinks the loads to just before their use
                step(a[g], cur);
                cur = nxt;
            }
        } else {
            float4 za = vq_fetch<VEC, FLAT>(rsa, zrow, row_off, a_ok, 4u * kq, D);
            for (unsigned g = 0; g < groups; ++g) {
                const VqCodes nxt = fetch_codes(g + 1);                  // g + 1 == groups: k0 >= D, reads zeros
                const float4 zn = vq_fetch<VEC, FLAT>(rsa, zrow, row_off, a_ok, 16u * (g + 1) + 4u * kq, D);
                __builtin_amdgcn_sched_barrier(0);
                step(za, cur);
                cur = nxt;
                za = zn;
            }
        }
#pragma unroll
        for (int t = 0; t < VQ_TILES; ++t) {
            float n = nrm[t];                                            // the four kq lanes of a code hold a quarter of its norm each
            n += __shfl_xor(n, 16, 64);
            n += __shfl_xor(n, 32, 64);
            const int64_t code = code0 + 16 * t + l16;
            const int32_t ci = (int32_t)(code < K ? code : 0x7fffffff);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float s = code < K ? fmaf(-2.f, acc[t][v], n) : INFINITY;
                if (arg_better_min(s, ci, best[v].v, best[v].i)) { best[v].v = s; best[v].i = ci; }
            }
        }
    }
    // rows 4 kq + v: over the 16 l16 lanes (xor masks below 16 stay inside the kq group), then over the waves
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const float ov = __shfl_xor(best[v].v, m, 64);
            const int32_t oi = __shfl_xor(best[v].i, m, 64);
            if (arg_better_min(ov, oi, best[v].v, best[v].i)) { best[v].v = ov; best[v].i = oi; }
        }
        if (l16 == 0) { sv[wave][4 * kq + v] = best[v].v; si[wave][4 * kq + v] = best[v].i; }
    }
    __syncthreads();
    if (tid < VQ_ROWS) {
        ArgBest b{sv[0][tid], si[0][tid]};                               // wave 0 has scored code 0: never the initial pair
#pragma unroll
        for (int w = 1; w < VQ_WAVES; ++w)
            if (arg_better_min(sv[w][tid], si[w][tid], b.v, b.i)) { b.v = sv[w][tid]; b.i = si[w][tid]; }
        sfin[tid] = b.i;
        if (tid < rows) idx[row0 + tid] = b.i;
    }
    if (!zq) return;
    __syncthreads();
    for (int r = wave; r < rows; r += VQ_WAVES) {
        const float* src = cb + (int64_t)sfin[r] * D;
        float* dst = zq + (row0 + r) * (int64_t)D;
        for (unsigned c = lane; c < D; c += 64) dst[c] = src[c];
    }
}

// -------------------------------------------------------------------------------------------------------------------- the loss
constexpr int VQ_LOSS_THREADS = 1024;
// loss[0] = (1 + beta) sum (zq - ze)^2 / n ; dzq = 2 (zq - ze) / n ; dze = 2 beta (ze - zq) / n.  One block: the sum's order is fixed
// (a strided fma chain per thread, then block_sum of common.h) and there is nothing to hand from a first launch to a second.
__global__ __launch_bounds__(VQ_LOSS_THREADS) void vq_loss_kernel(const float* __restrict__ ze, const float* __restrict__ zq,
                                                                   float* __restrict__ loss, float* __restrict__ dze,
                                                                   float* __restrict__ dzq, int64_t n, float cq, float ce, float scale) {
    __shared__ float red[VQ_LOSS_THREADS / 64];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += VQ_LOSS_THREADS) {
        const float d = zq[i] - ze[i];
        s = fmaf(d, d, s);
        if (dzq) dzq[i] = d * cq;
        if (dze) dze[i] = -d * ce;
    }
    s = block_sum<VQ_LOSS_THREADS / 64>(s, red);
    if (threadIdx.x == 0) loss[0] = s * scale;
}

template <bool VEC, bool FLAT>
static void vq_wide_launch(const float* z, const float* cb, int32_t* idx, float* zq, int64_t N, int64_t D, int64_t K, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(N, VQ_ROWS)), block(VQ_WAVES * 64);
    const unsigned d = (unsigned)D;
#define VQ_WIDE(NG) hipLaunchKernelGGL((vq_wide_kernel<NG, VEC, FLAT>), grid, block, 0, st, z, cb, idx, zq, N, d, K)
#define VQ_WIDE_CASE(NG) case NG: VQ_WIDE(NG); break
    if constexpr (FLAT) {
        VQ_WIDE(0);
    } else {
        switch (D <= VQ_WIDE_RESIDENT_D ? (int)((D + 15) / 16) : 0) {          // one instantiation per number of k-groups
            VQ_WIDE_CASE(1); VQ_WIDE_CASE(2); VQ_WIDE_CASE(3); VQ_WIDE_CASE(4); VQ_WIDE_CASE(5); VQ_WIDE_CASE(6); VQ_WIDE_CASE(7); VQ_WIDE_CASE(8);
            VQ_WIDE_CASE(9); VQ_WIDE_CASE(10); VQ_WIDE_CASE(11); VQ_WIDE_CASE(12); VQ_WIDE_CASE(13); VQ_WIDE_CASE(14); VQ_WIDE_CASE(15);
            VQ_WIDE_CASE(16);
            default: VQ_WIDE(0); break;
        }
    }
#undef VQ_WIDE_CASE
#undef VQ_WIDE
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipVQNearest(const float* z, const float* codebook, int32_t* idx, float* zq, int64_t N, int64_t D, int64_t K,
                              nnhipStream_t s) {
    constexpr int64_t lim = (int64_t)1 << 31;
    NNHIP_CHECK_ARG(N >= 1 && N < lim && D >= 1 && D < lim && K >= 1 && K < lim, NNHIP_EINVAL, "nnhipVQNearest: bad sizes");
    NNHIP_CHECK_ARG(z && codebook && idx, NNHIP_EINVAL, "nnhipVQNearest: null pointer");
    hipStream_t st = (hipStream_t)s;
    if (D <= VQ_NARROW_MAX_D) {
        const dim3 grid((unsigned)ceil_div(N, 256)), block(256);
        switch ((int)D) {
#define VQ_NARROW(DD) case DD: hipLaunchKernelGGL(vq_narrow_kernel<DD>, grid, block, 0, st, z, codebook, idx, zq, N, K); break
            VQ_NARROW(1); VQ_NARROW(2); VQ_NARROW(3); VQ_NARROW(4); VQ_NARROW(5); VQ_NARROW(6); VQ_NARROW(7); VQ_NARROW(8);
#undef VQ_NARROW
        }
        NNHIP_LAUNCH_CHECK("vq_narrow_kernel");
        return 0;
    }
    if (D > VQ_BUFFER_MAX_D) vq_wide_launch<false, true>(z, codebook, idx, zq, N, D, K, st);
    else if (D % 4 == 0 && aligned16(z) && aligned16(codebook)) vq_wide_launch<true, false>(z, codebook, idx, zq, N, D, K, st);
    else vq_wide_launch<false, false>(z, codebook, idx, zq, N, D, K, st);
    NNHIP_LAUNCH_CHECK("vq_wide_kernel");
    return 0;
}

extern "C" int nnhipVQLossForwardBackward(const float* z_e, const float* z_q, float beta, float* loss, float* dz_e, float* dz_q,
                                          int64_t n, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n > 0, NNHIP_EINVAL, "nnhipVQLossForwardBackward: n must be > 0");
    NNHIP_CHECK_ARG(z_e && z_q && loss, NNHIP_EINVAL, "nnhipVQLossForwardBackward: null pointer");
    const float cq = 2.0f / (float)n;
    hipLaunchKernelGGL(vq_loss_kernel, dim3(1), dim3(VQ_LOSS_THREADS), 0, (hipStream_t)s, z_e, z_q, loss, dz_e, dz_q, n, cq, beta * cq,
                       (1.0f + beta) / (float)n);
    NNHIP_LAUNCH_CHECK("vq_loss_kernel");
    return 0;
}
