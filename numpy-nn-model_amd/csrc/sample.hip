// sample.hip -- device-side top-k sampling (ABI 213): temperature, top-k and the multinomial draw of the reference's GPT-2 script
// (examples/gpt2/gpt2_infer.py:331-338: last / max(T, 1e-6), np.argpartition, softmax_np, np.random.choice) without handing the
// logits to the host.  The random number is a counter-based hash of (seed + a device word, row) -- the construction that makes
// nnhipDropout graph-safe -- so a captured decode step draws a fresh token on every replay.
//
// Everything is decided by ONE total order on the elements of a row, the one nnhipArgmaxF32 uses (embedding.hip: arg_better): a
// NaN beats any number, a larger value beats a smaller one, ties go to the lower index.  Each element becomes a 63-bit integer
// `comp` = (order-preserving key of the value) << 31 | (2^31 - 1 - index): comp is unique within a row, a larger comp is a better
// element, and 0 is free to mean "no element".  Top-k is then an exact radix select on integers, the candidates' order a sort of
// integers: no floating-point comparison or reduction order can change which tokens are candidates or where they sit in the CDF.
//
// Two launches, nothing else (a captured step stays "kernels only"):
//   sample_chunk_topk_kernel  block (row, chunk of 2048): the chunk in registers -> its top min(k, n) by radix select (8 bits per
//                             pass, 256-bin LDS histogram of integer counts) -> comps into the library workspace
//   sample_draw_kernel        block per row: radix select of the final k from chunks x k comps, bitonic sort in LDS (descending),
//                             e_j = exp((x_j - x_0) / t), the SEQUENTIAL float32 sum c_j in sorted order, the uniform, the draw.
#include <math.h>

#include "common.h"

namespace nnhip {

constexpr int SM_CHUNK = 2048;        // elements per block of the first kernel: 256 threads x 8 consecutive floats
constexpr int SM_STAGE = 4096;        // comps the draw kernel keeps in LDS (32 KiB); longer lists are re-read from the workspace
typedef unsigned long long u64;

__device__ __forceinline__ u64 sm_comp(float x, int64_t idx) {
    const unsigned b = __float_as_uint(x);
    unsigned key;
    if (x != x) key = 0xFFFFFFFFu;                                  // every NaN: above +inf (0xFF800000), equal among themselves
    else if (x == 0.f) key = 0x80000000u;                           // -0 == +0 in arg_better: one key
    else key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);          // -inf -> 0x007FFFFF: a real element's comp is never 0
    return ((u64)key << 31) | (u64)(0x7FFFFFFFu - (unsigned)idx);
}
__device__ __forceinline__ float sm_value(u64 comp) {
    const unsigned key = (unsigned)(comp >> 31);
    if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}
__device__ __forceinline__ int32_t sm_index(u64 comp) { return (int32_t)(0x7FFFFFFFu - (unsigned)(comp & 0x7FFFFFFFu)); }

struct SelectLds {
    unsigned hist[256];
    unsigned digit, above, count;
};

// Exact top-`want` of the block's comps (each thread presents its own through `each`; 0 = no element): returns the threshold T
// with exactly `want` comps >= T.  Most significant digit first; a pass histograms the digit of the comps that still match the
// digits chosen so far, wave 0 walks the 256 counts from the top to the digit holding the want-th element.  `matched` = how many
// comps match the chosen digits (~0u: unknown): when that equals `want` all of them are in and the remaining passes are skipped.
// blockDim.x == 256; want >= 1 and at most the number of non-zero comps; all threads call it, all get T.
template <class Each>
__device__ __forceinline__ u64 sm_radix_select(Each&& each, unsigned want, unsigned matched, SelectLds& L) {
    const int tid = threadIdx.x, lane = tid & 63;
    u64 prefix = 0;
    for (int shift = 56;; shift -= 8) {
        if (want == matched) return prefix ? prefix : 1;
        const u64 himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        L.hist[tid] = 0;
        __syncthreads();
        each([&](u64 c) {
            if (c != 0 && ((c ^ prefix) & himask) == 0) atomicAdd(&L.hist[(unsigned)(c >> shift) & 255u], 1u);
        });
        __syncthreads();
        if (tid < 64) {                                             // lane l owns digits 255 - 4l .. 252 - 4l, in that order
            unsigned c[4], s = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = L.hist[255 - 4 * lane - j]; s += c[j]; }
            unsigned incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            unsigned excl = incl - s;                               // comps with a larger digit than this lane's first
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (excl < want && want <= excl + c[j]) { L.digit = 255 - 4 * lane - j; L.above = excl; L.count = c[j]; }
                excl += c[j];
            }
        }
        __syncthreads();
        want -= L.above;
        matched = L.count;
        prefix |= (u64)L.digit << shift;
        if (shift == 0) return prefix;
    }
}

// ws[(row * chunks + chunk) * kc + s], s < kc: the chunk's best min(kc, elements in the chunk) comps in no particular order, then 0s.
// A row starts wherever r * ld puts it (50257 floats: 16-byte aligned in one row of four): the chunks are cut on the 16-byte grid
// of the ROW's address (virtual position v = a + element, a = the row's misalignment in floats), so every float4 is aligned; the
// two partial vectors at the row's ends are read float by float, and nothing outside [row, row + n) is touched.
__global__ __launch_bounds__(256) void sample_chunk_topk_kernel(const float* __restrict__ logits, int64_t n, int64_t ld, int chunks,
                                                                int kc, u64* __restrict__ ws) {
    __shared__ SelectLds L;
    __shared__ unsigned slot;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const float* row = logits + r * ld;
    const int64_t a = (int64_t)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u);
    u64* dst = ws + (size_t)blockIdx.x * kc;
    const int64_t vlo = ch * SM_CHUNK > a ? ch * SM_CHUNK : a, vhi = (ch + 1) * SM_CHUNK < a + n ? (ch + 1) * SM_CHUNK : a + n;
    const int64_t valid = vhi > vlo ? vhi - vlo : 0;
    const unsigned want = (unsigned)(valid < kc ? valid : kc);
    for (int s = (int)want + tid; s < kc; s += 256) dst[s] = 0;
    if (want == 0) return;

    u64 comp[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t i = ch * SM_CHUNK + tid * 8 + h * 4 - a;      // element index of the vector's first float
        if (i >= 0 && i + 4 <= n) {
            const float4 q = *reinterpret_cast<const float4*>(row + i);
            comp[h * 4 + 0] = sm_comp(q.x, i);
            comp[h * 4 + 1] = sm_comp(q.y, i + 1);
            comp[h * 4 + 2] = sm_comp(q.z, i + 2);
            comp[h * 4 + 3] = sm_comp(q.w, i + 3);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) comp[h * 4 + e] = (i + e >= 0 && i + e < n) ? sm_comp(row[i + e], i + e) : 0ull;
        }
    }
    if (tid == 0) slot = 0;
    const u64 T = sm_radix_select([&](auto&& f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f(comp[e]);
    }, want, (unsigned)valid, L);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (comp[e] >= T && comp[e] != 0) {                         // exactly `want` of them
            const unsigned s = atomicAdd(&slot, 1u);
            if (s < want) dst[s] = comp[e];
        }
}

// One block per row.  list = the row's m comps (zeros among them), k = min(top_k, n) <= 1024 of them are real at least.
__global__ __launch_bounds__(256) void sample_draw_kernel(int32_t* __restrict__ out_ids, float* __restrict__ u_out,
                                                          const u64* __restrict__ ws, int64_t m, int k, float t, unsigned seed,
                                                          const unsigned* __restrict__ seed_dev) {
    __shared__ u64 stage[SM_STAGE];
    __shared__ u64 sel[NNHIP_SAMPLE_MAX_K];
    __shared__ float cum[NNHIP_SAMPLE_MAX_K];
    __shared__ SelectLds L;
    __shared__ unsigned slot;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const u64* list = ws + (size_t)r * m;
    if (m <= SM_STAGE) {
        for (int i = tid; i < (int)m; i += 256) stage[i] = list[i];
        list = stage;
    }
    if (tid == 0) slot = 0;
    __syncthreads();
    const u64 T = sm_radix_select([&](auto&& f) {
        for (int64_t i = tid; i < m; i += 256) f(list[i]);
    }, (unsigned)k, ~0u, L);
    __syncthreads();
    for (int64_t i = tid; i < m; i += 256) {
        const u64 c = list[i];
        if (c >= T && c != 0) {                                     // exactly k of them
            const unsigned s = atomicAdd(&slot, 1u);
            if (s < (unsigned)k) sel[s] = c;
        }
    }
    int P = 1;
    while (P < k) P <<= 1;
    for (int i = k + tid; i < P; i += 256) sel[i] = 0;
    __syncthreads();
    // bitonic sort, descending: comp order = (value descending, index ascending), the padding zeros last
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += 256) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const u64 x = sel[lo], y = sel[hi];
                if ((x < y) == desc) { sel[lo] = y; sel[hi] = x; }
            }
            __syncthreads();
        }
    const u64 best = sel[0];
    const float x0 = sm_value(best);
    const float tt = fmaxf(t, 1e-6f);
    for (int j = tid; j < k; j += 256) cum[j] = expf((sm_value(sel[j]) - x0) / tt);
    __syncthreads();
    if (tid == 0) {
        // the seed word is rewritten between launches (a position counter): agent-scope load, never a scalar-cache line
        const unsigned sd = seed + (seed_dev ? (unsigned)ld_dev_i32(reinterpret_cast<const int*>(seed_dev)) : 0u);
        const float u = (float)(at_hash(at_rowkey(sd, (unsigned)r), 0u) >> 8) * 5.9604644775390625e-08f;      // [0, 1)
        int pick = 0;
        if (x0 == x0 && fabsf(x0) != INFINITY) {                    // else: a NaN, or +-inf on top -- argmax's answer
            float c = 0.f;
            int last = 0;
            for (int j = 0; j < k; ++j) {                           // sequential on purpose: the order of the sum is the contract
                const float e = cum[j];
                if (e > 0.f) last = j;
                c += e;
                cum[j] = c;
            }
            const float target = u * c;
            pick = -1;
            for (int j = 0; j < k; ++j)
                if (cum[j] > target) { pick = j; break; }
            if (pick < 0) pick = last;
        }
        out_ids[r] = sm_index(sel[pick]);
        if (u_out) u_out[r] = u;
    }
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipSampleTopK(int32_t* out_ids, float* u_out, const float* logits, int64_t rows, int64_t n, int64_t ld,
                               int32_t top_k, float temperature, uint32_t seed, const uint32_t* seed_dev, nnhipStream_t s) {
    NNHIP_CHECK_ARG(rows >= 0, NNHIP_EINVAL, "nnhipSampleTopK: negative size");
    NNHIP_CHECK_ARG(top_k >= 1, NNHIP_EINVAL, "nnhipSampleTopK: top_k must be at least 1 (greedy decoding is nnhipArgmaxF32)");
    NNHIP_CHECK_ARG(top_k <= NNHIP_SAMPLE_MAX_K, NNHIP_EINVAL, "nnhipSampleTopK: top_k above NNHIP_SAMPLE_MAX_K = %d", NNHIP_SAMPLE_MAX_K);
    NNHIP_CHECK_ARG(temperature >= 0.f, NNHIP_EINVAL, "nnhipSampleTopK: temperature is NaN or negative");
    NNHIP_CHECK_ARG(ld >= n, NNHIP_EINVAL, "nnhipSampleTopK: row stride ld smaller than n");
    NNHIP_CHECK_ARG(n < ((int64_t)1 << 31), NNHIP_EINVAL, "nnhipSampleTopK: row longer than int32 indices can address");
    if (rows == 0) return 0;
    NNHIP_CHECK_ARG(n >= 1, NNHIP_EINVAL, "nnhipSampleTopK: attempt to sample from an empty row");
    NNHIP_CHECK_ARG(out_ids && logits, NNHIP_EINVAL, "nnhipSampleTopK: null pointer");
    NNHIP_CHECK_ARG(aligned4(logits) && aligned4(out_ids) && aligned4(u_out) && aligned4(seed_dev), NNHIP_EALIGN,
                    "nnhipSampleTopK: pointer not 4-byte aligned");
    const int k = (int)(top_k < n ? top_k : n);
    const int64_t chunks = ceil_div(n + 3, SM_CHUNK);               // + 3: a misaligned row's first vector starts up to 3 floats early
    NNHIP_CHECK_ARG(rows * chunks < ((int64_t)1 << 31), NNHIP_EINVAL, "nnhipSampleTopK: too many rows");
    u64* ws = static_cast<u64*>(workspace((size_t)rows * chunks * k * sizeof(u64)));
    NNHIP_CHECK_ARG(ws != nullptr, NNHIP_ENOMEM, "nnhipSampleTopK: workspace allocation failed");
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(sample_chunk_topk_kernel, dim3((unsigned)(rows * chunks)), dim3(256), 0, st, logits, n, ld, (int)chunks, k, ws);
    NNHIP_LAUNCH_CHECK("sample_chunk_topk_kernel");
    hipLaunchKernelGGL(sample_draw_kernel, dim3((unsigned)rows), dim3(256), 0, st, out_ids, u_out, ws, chunks * k, k, temperature, seed,
                       seed_dev);
    NNHIP_LAUNCH_CHECK("sample_draw_kernel");
    return 0;
}
