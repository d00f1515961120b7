// grad_norm.hip -- the global gradient norm (L2 or max) of all tensors in ONE launch, finished inside that launch, and the in-place
// scale of all tensors by a device divisor.  Net-new (the reference has no gradient clipping): the piece that computes the one-float
// device word every update kernel here already divides the gradient by (adam_device.h: adam_dev_resolve).
//
// The block <-> (tensor, chunk) map is the optimizer plan's (optim.hip: fused_optimizer_plan, one pointer table, the handle's slot 1).
// A block reduces its chunk to one value, leaves it in its slot of the handle's partials buffer, and draws an arrival ticket; the
// block that draws the last ticket combines the slots in a fixed order and writes the result words.  No float atomics: the same
// gradients give the same bits, whatever order the blocks ran in.
#include <math.h>

#include "common.h"
#include "optim_rules_device.h"   // fused_optimizer_plan / _state / _norm_scratch

namespace nnhip {

typedef float gn_f4 __attribute__((ext_vector_type(4)));

// What a block folds its elements into.  L2: the float32 sum of squares.  INF: the largest |g| as its BIT PATTERN under unsigned
// max -- for sign-cleared floats the unsigned order is the float order, with every NaN above inf: a NaN wins by itself (fmaxf would
// drop it) and the result is exact.
template <int NORM> struct GnOp;
template <> struct GnOp<NNHIP_NORM_L2> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ void take(T& a, float x) {
#pragma clang fp contract(off)
        a = a + x * x;                  // no fma: the sum's rounding sequence is part of the contract (tests/gradclip_ref.py restates it)
    }
    static __device__ __forceinline__ T join(T a, T b) { return a + b; }
    static __device__ __forceinline__ unsigned bits(T a) { return __float_as_uint(a); }
};
template <> struct GnOp<NNHIP_NORM_INF> {
    typedef unsigned T;
    static __device__ __forceinline__ T zero() { return 0u; }
    static __device__ __forceinline__ void take(T& a, float x) { const unsigned b = __float_as_uint(x) & 0x7fffffffu; a = a > b ? a : b; }
    static __device__ __forceinline__ T join(T a, T b) { return a > b ? a : b; }
    static __device__ __forceinline__ unsigned bits(T a) { return a; }
};

template <int CTRL, class T>
__device__ __forceinline__ T gn_dpp(T v) {
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <class T>
__device__ __forceinline__ T gn_lane(T v, int lane) { return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane)); }
// common.h's wave_sum with the operation as a parameter: a balanced pairwise tree over the 64 lanes (lanes 2k and 2k + 1 first).
template <class Op>
__device__ __forceinline__ typename Op::T gn_wave(typename Op::T v) {
    v = Op::join(v, gn_dpp<kDppXor1>(v));
    v = Op::join(v, gn_dpp<kDppXor2>(v));
    v = Op::join(v, gn_dpp<kDppHalfMirror>(v));
    v = Op::join(v, gn_dpp<kDppMirror>(v));
    return Op::join(Op::join(gn_lane(v, 0), gn_lane(v, 16)), Op::join(gn_lane(v, 32), gn_lane(v, 48)));
}

// The plan blob with one pointer table: [g*  n][sizes int64 n][blk_tensor int32 nblk][blk_chunk int32 nblk].
struct GnChunk { float* g; int cnt; };
__device__ __forceinline__ GnChunk gn_chunk(const unsigned char* __restrict__ blob, int n, int nblk, int chunk) {
    float* const* G = reinterpret_cast<float* const*>(blob);
    const int64_t* sizes = reinterpret_cast<const int64_t*>(blob + sizeof(void*) * n);
    const int32_t* blk_tensor = reinterpret_cast<const int32_t*>(blob + sizeof(void*) * n + sizeof(int64_t) * n);
    const int32_t* blk_chunk = blk_tensor + nblk;
    const int ti = blk_tensor[blockIdx.x];
    const int64_t off = (int64_t)blk_chunk[blockIdx.x] * chunk;
    int64_t cnt = sizes[ti] - off;
    if (cnt > chunk) cnt = chunk;
    return {G[ti] + off, (int)cnt};
}

// words: {norm of the effective gradient, divisor for the update, non-finite flag, max_norm for device-driven stepping}.
// Element e of a chunk belongs to lane (e / 4) % 256 and to that lane's accumulator e % 4, on the 16-byte-load path and on the
// scalar-load path alike, so both give the same bits; a lane takes its elements in increasing order.
// dev_state != null (step == 0): grad_scale comes from the handle's device state and max_norm from words[3], as lr does for the
// update kernels -- a captured launch would freeze the host values.
template <int NORM>
__global__ __launch_bounds__(256) void grad_norm_multi_kernel(const unsigned char* __restrict__ blob, int n, int nblk, int chunk,
                                                              float* partials, unsigned* ticket, const float* dev_state,
                                                              const float* divisor_in, float grad_scale, float max_norm, float* words) {
    typedef GnOp<NORM> Op;
    typedef typename Op::T T;
    // [0..3] the waves' values, [4] "this block drew the last ticket", [8..15] four doubles for the finish: ONE LDS object
    __shared__ __attribute__((aligned(8))) unsigned sh[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (nblk > 0) {
        const GnChunk c = gn_chunk(blob, n, nblk, chunk);
        const float* g = c.g;                    // (not __restrict__-const data for the finisher: that is `partials`, below)
        const int nv = c.cnt >> 2, tail = c.cnt & 3;
        T a0 = Op::zero(), a1 = Op::zero(), a2 = Op::zero(), a3 = Op::zero();
        // chunk offsets are multiples of 2048 elements, so 16-B alignment of the chunk == of the tensor
        if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {
            const gn_f4* g4 = reinterpret_cast<const gn_f4*>(g);
#pragma unroll 4
            for (int i = tid; i < nv; i += 256) {
                const gn_f4 x = g4[i];           // plain loads: the update launch reads the gradient next, out of L2 / MALL where it fits
                Op::take(a0, x.x); Op::take(a1, x.y); Op::take(a2, x.z); Op::take(a3, x.w);
            }
        } else {
#pragma unroll 4
            for (int i = tid; i < nv; i += 256) {
                const float x0 = g[4 * i], x1 = g[4 * i + 1], x2 = g[4 * i + 2], x3 = g[4 * i + 3];
                Op::take(a0, x0); Op::take(a1, x1); Op::take(a2, x2); Op::take(a3, x3);
            }
        }
        if (tail && tid == (nv & 255)) {         // the lane whose next float4 the 1..3 leftover elements would have started
            Op::take(a0, g[4 * nv]);
            if (tail > 1) Op::take(a1, g[4 * nv + 1]);
            if (tail > 2) Op::take(a2, g[4 * nv + 2]);
        }
        const T a = gn_wave<Op>(Op::join(Op::join(a0, a1), Op::join(a2, a3)));
        if (lane == 0) sh[w] = Op::bits(a);
        __syncthreads();
        // ---- publish the block's value, draw a ticket: agent-scope release / acquire, correct wherever the blocks run ----
        if (tid == 0) {
            const T b = Op::join(Op::join(Op::join(__builtin_bit_cast(T, sh[0]), __builtin_bit_cast(T, sh[1])), __builtin_bit_cast(T, sh[2])),
                                 __builtin_bit_cast(T, sh[3]));
            reinterpret_cast<unsigned*>(partials)[blockIdx.x] = Op::bits(b);       // plain store
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // after the fence, before the ticket: always
            const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool last = t == (unsigned)nblk - 1u;
            sh[4] = last ? 1u : 0u;
            if (last) {                          // every other block's slot is published: drop this CU's stale lines, then read
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
        if (sh[4] == 0u) return;
    } else if (blockIdx.x != 0) {
        return;
    }
    // ---- the last block to arrive: combine the slots in a fixed order -- lane t takes blocks t, t + 256, ... in increasing order,
    // the lanes combine in a butterfly, the four waves in order; L2 in double (exact next to the float32 partials) ----
    double* shd = reinterpret_cast<double*>(sh + 8);
    float root;
    if constexpr (NORM == NNHIP_NORM_L2) {
        double s = 0.0;
        for (int b = tid; b < nblk; b += 256) s += (double)partials[b];
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k);
        if (lane == 0) shd[w] = s;
        __syncthreads();
        root = (float)sqrt(((shd[0] + shd[1]) + shd[2]) + shd[3]);
    } else {
        unsigned m = 0u;
        for (int b = tid; b < nblk; b += 256) { const unsigned v = reinterpret_cast<unsigned*>(partials)[b]; m = m > v ? m : v; }
        m = gn_wave<Op>(m);
        if (lane == 0) sh[8 + w] = m;
        __syncthreads();
        unsigned r = sh[8];
#pragma unroll
        for (int i = 1; i < 4; ++i) r = r > sh[8 + i] ? r : sh[8 + i];
        root = __uint_as_float(r);
    }
    if (tid != 0) return;
    {
#pragma clang fp contract(off)
        float gs = dev_state ? ld_dev_f32(dev_state + 2) : grad_scale;
        const float d_in = divisor_in ? ld_dev_f32(divisor_in) : 1.f;
        if (divisor_in) gs = gs / d_in;                                            // adam_dev_resolve's expression
        const float norm = fabsf(gs) * root;
        const float mx = dev_state ? ld_dev_f32(words + 3) : max_norm;
        const float ratio = (norm + 1e-6f) / mx;
        const float coef = (ratio > 1.f || ratio != ratio) ? ratio : 1.f;          // max(1, ratio) that keeps a NaN, as torch's clamp
        words[0] = norm;
        words[1] = d_in * coef;
        words[2] = (norm - norm == 0.f) ? 0.f : 1.f;                               // NaN or inf
    }
    if (nblk > 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch starts from zero
}

// g[i] /= divisor[0], every tensor, one launch, on the norm's plan.
__global__ __launch_bounds__(256) void grad_scale_multi_kernel(const unsigned char* __restrict__ blob, int n, int nblk, int chunk,
                                                               const float* __restrict__ divisor) {
    const float d = ld_dev_f32(divisor);
    const GnChunk c = gn_chunk(blob, n, nblk, chunk);
    float* g = c.g;
    const int tid = threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {
        gn_f4* g4 = reinterpret_cast<gn_f4*>(g);
        const int nv = c.cnt >> 2;
#pragma unroll 4
        for (int i = tid; i < nv; i += 256) {
            gn_f4 x = g4[i];
            x.x = x.x / d; x.y = x.y / d; x.z = x.z / d; x.w = x.w / d;
            g4[i] = x;
        }
        for (int j = (nv << 2) + tid; j < c.cnt; j += 256) g[j] = g[j] / d;
    } else {
        for (int j = tid; j < c.cnt; j += 256) g[j] = g[j] / d;
    }
}

// The argument checks both entries share; the plan (slot 1) on success.
static int gn_plan(void* opt, const char* who, int32_t n_tensors, const float* const* g, const int64_t* sizes, hipStream_t st,
                   const unsigned char** blob, int* nblk, int* chunk) {
    *blob = nullptr; *nblk = 0; *chunk = 0;
    NNHIP_CHECK_ARG(n_tensors >= 0, NNHIP_EINVAL, "%s: negative n_tensors", who);
    if (n_tensors == 0) return 0;
    NNHIP_CHECK_ARG(g && sizes, NNHIP_EINVAL, "%s: null table", who);
    for (int i = 0; i < n_tensors; ++i) {
        NNHIP_CHECK_ARG(sizes[i] >= 0, NNHIP_EINVAL, "%s: negative size", who);
        NNHIP_CHECK_ARG(sizes[i] == 0 || g[i] != nullptr, NNHIP_EINVAL, "%s: null tensor pointer", who);
        NNHIP_CHECK_ARG(aligned4(g[i]), NNHIP_EALIGN, "%s: misaligned tensor pointer (4 bytes required)", who);
    }
    const void* const* const tables[1] = {reinterpret_cast<const void* const*>(g)};
    return fused_optimizer_plan(opt, who, n_tensors, 1, tables, sizes, st, blob, nblk, chunk, 1);
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipGradNormMultiTensor(void* opt, int32_t n_tensors, const float* const* g, const int64_t* sizes, int32_t norm_type,
                                        double max_norm, const float* divisor_in_or_null, int32_t step, float grad_scale, float* words,
                                        nnhipStream_t s) {
    static const char* who = "nnhipGradNormMultiTensor";
    NNHIP_CHECK_ARG(opt != nullptr, NNHIP_EINVAL, "%s: null optimizer handle", who);
    NNHIP_CHECK_ARG(words != nullptr, NNHIP_EINVAL, "%s: null words", who);
    NNHIP_CHECK_ARG(aligned4(words) && aligned4(divisor_in_or_null), NNHIP_EALIGN, "%s: misaligned words / divisor pointer (4 bytes required)", who);
    if (int rc = device_error_status(who)) return rc;                              // an earlier kernel raised the device error word
    NNHIP_CHECK_ARG(norm_type == NNHIP_NORM_L2 || norm_type == NNHIP_NORM_INF, NNHIP_EINVAL, "%s: unknown norm_type %d", who, (int)norm_type);
    NNHIP_CHECK_ARG(step >= 0, NNHIP_EINVAL, "%s: negative step", who);
    NNHIP_CHECK_ARG(step == 0 || max_norm > 0.0, NNHIP_EINVAL, "%s: max_norm must be > 0 (and not NaN)", who);
    float* dstate = nullptr;
    const float* bound_div = nullptr;            // the handle's bound divisor is the UPDATE's business: the norm takes divisor_in
    if (int rc = fused_optimizer_state(opt, step, &dstate, &bound_div)) {
        set_last_error("%s: step == 0 needs nnhipFusedOptimizerSetStep and SetHyper first", who);
        return rc;
    }
    hipStream_t st = (hipStream_t)s;
    const unsigned char* blob = nullptr;
    int nblk = 0, chunk = 0;
    if (int rc = gn_plan(opt, who, n_tensors, g, sizes, st, &blob, &nblk, &chunk)) return rc;
    unsigned* ticket = nullptr;
    float* partials = nullptr;
    if (nblk > 0)
        if (int rc = fused_optimizer_norm_scratch(opt, who, nblk, st, &ticket, &partials)) return rc;
    // nothing to reduce: still one (one-block) launch that writes the identity words -- a captured step looks the same every time
    const dim3 grid((unsigned)(nblk > 0 ? nblk : 1));
    if (norm_type == NNHIP_NORM_L2)
        hipLaunchKernelGGL(grad_norm_multi_kernel<NNHIP_NORM_L2>, grid, dim3(256), 0, st, blob, (int)n_tensors, nblk, chunk, partials, ticket,
                           (const float*)dstate, divisor_in_or_null, grad_scale, (float)max_norm, words);
    else
        hipLaunchKernelGGL(grad_norm_multi_kernel<NNHIP_NORM_INF>, grid, dim3(256), 0, st, blob, (int)n_tensors, nblk, chunk, partials, ticket,
                           (const float*)dstate, divisor_in_or_null, grad_scale, (float)max_norm, words);
    NNHIP_LAUNCH_CHECK("grad_norm_multi_kernel");
    return 0;
}

extern "C" int nnhipScaleMultiTensor(void* opt, int32_t n_tensors, float* const* g, const int64_t* sizes, const float* divisor_dev,
                                     nnhipStream_t s) {
    static const char* who = "nnhipScaleMultiTensor";
    NNHIP_CHECK_ARG(opt != nullptr, NNHIP_EINVAL, "%s: null optimizer handle", who);
    NNHIP_CHECK_ARG(divisor_dev != nullptr, NNHIP_EINVAL, "%s: null divisor", who);
    NNHIP_CHECK_ARG(aligned4(divisor_dev), NNHIP_EALIGN, "%s: misaligned divisor pointer (4 bytes required)", who);
    if (int rc = device_error_status(who)) return rc;
    hipStream_t st = (hipStream_t)s;
    const unsigned char* blob = nullptr;
    int nblk = 0, chunk = 0;
    if (int rc = gn_plan(opt, who, n_tensors, g, sizes, st, &blob, &nblk, &chunk)) return rc;
    if (nblk == 0) return 0;
    hipLaunchKernelGGL(grad_scale_multi_kernel, dim3((unsigned)nblk), dim3(256), 0, st, blob, (int)n_tensors, nblk, chunk, divisor_dev);
    NNHIP_LAUNCH_CHECK("grad_scale_multi_kernel");
    return 0;
}
