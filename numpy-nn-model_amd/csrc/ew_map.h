// ew_map.h -- the float4 grid-stride map skeleton of the elementwise kernels (elementwise.hip: activations, add, mul, scale;
// tensor_ops.hip: the same-shape and scalar tiers of the broadcasting binary ops).  One definition, so that a same-shape
// Tensor.add through either entry runs the same code and gives the same bits.
#pragma once
#include <stdlib.h>

#include "common.h"

namespace nnhip {

constexpr int EW_THREADS = 256;
constexpr int EW_MAX_BLOCKS = 1 << 20;  // one 4-float4 span per thread at any realistic size; the loop is a backstop

inline int ew_blocks(int64_t n_items) {
    int64_t b = ceil_div(n_items > 0 ? n_items : 1, EW_THREADS);
    return (int)(b < EW_MAX_BLOCKS ? b : EW_MAX_BLOCKS);
}

// Generic unary/binary maps over float4 with scalar tail -----------------------------------------
// Each block walks contiguous 256*EW_U-float4 spans; the EW_U loads of a span are issued together
// (EW_U x 16 B in flight per lane) before any math, then EW_U stores.
constexpr int EW_U = 4;

typedef float ew_f4 __attribute__((ext_vector_type(4)));
// Streaming accesses.  Non-temporal LOADS (bit 0, the default for tensors of >= 128 MB) read the inputs without allocating
// in L2, which leaves L2 to the write-back of the previous kernel's output: cold C3 pass Swish forward 0.58-0.64 -> 0.74-0.78
// of the HBM spec, backward 0.62 -> 0.69-0.77; back-to-back on hot buffers forward -4 %, backward +22 %.  Non-temporal
// STORES (bit 1) win back-to-back (backward 6.8 TB/s) but lose cold (forward 0.58 -> 0.51) -- the consumer of an output is
// usually the next kernel.  NNHIP_EW_NT overrides (developer switch).
__device__ __forceinline__ float4 ew_load(const float4* p, int nt) {
    if (nt & 1) { const ew_f4 t = __builtin_nontemporal_load(reinterpret_cast<const ew_f4*>(p)); return make_float4(t.x, t.y, t.z, t.w); }
    return *p;
}
__device__ __forceinline__ void ew_store(float4* p, float4 v, int nt) {
    if (nt & 2) { ew_f4 t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w; __builtin_nontemporal_store(t, reinterpret_cast<ew_f4*>(p)); }
    else *p = v;
}
static int ew_nt(int64_t n) {
    static const int forced = env_int("NNHIP_EW_NT", -1);
    if (forced >= 0) return forced;
    return n * 4 >= ((int64_t)128 << 20) ? 1 : 0;
}
template <class F>
__device__ __forceinline__ void map1_body(float* out, const float* a, int64_t n, bool vec, const F& f, int nt) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        const int64_t nv = n >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(a);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (int64_t base = (int64_t)blockIdx.x * (EW_THREADS * EW_U); base < nv; base += gsz * EW_U) {
            float4 x[EW_U];
#pragma unroll
            for (int u = 0; u < EW_U; ++u) {
                const int64_t i = base + u * EW_THREADS + threadIdx.x;
                if (i < nv) x[u] = ew_load(a4 + i, nt);
            }
#pragma unroll
            for (int u = 0; u < EW_U; ++u) {
                const int64_t i = base + u * EW_THREADS + threadIdx.x;
                if (i < nv) {
                    float4 y;
                    y.x = f(x[u].x); y.y = f(x[u].y); y.z = f(x[u].z); y.w = f(x[u].w);
                    ew_store(o4 + i, y, nt);
                }
            }
        }
        for (int64_t i = (nv << 2) + gid; i < n; i += gsz) out[i] = f(a[i]);
    } else {
        for (int64_t i = gid; i < n; i += gsz) out[i] = f(a[i]);
    }
}
template <class F>
__global__ __launch_bounds__(EW_THREADS) void map1_kernel(float* out, const float* a, int64_t n,
                                                          bool vec, F f, int nt) {
    map1_body(out, a, n, vec, f, nt);
}
// The same map with the functor's scalar operand `f.s` read from a one-element DEVICE tensor when `sp` is not NULL: the value
// never visits the host, so the launch is legal inside a stream capture and needs no synchronisation.
template <class F>
__global__ __launch_bounds__(EW_THREADS) void map1s_kernel(float* out, const float* a, int64_t n,
                                                           bool vec, F f, const float* sp, int nt) {
    if (sp) f.s = ld_dev_f32(sp);
    map1_body(out, a, n, vec, f, nt);
}

template <class F>
__global__ __launch_bounds__(EW_THREADS) void map2_kernel(float* out, const float* a, const float* b, int64_t n,
                                                          bool vec, F f, int nt) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        const int64_t nv = n >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (int64_t base = (int64_t)blockIdx.x * (EW_THREADS * EW_U); base < nv; base += gsz * EW_U) {
            float4 x[EW_U], z[EW_U];
#pragma unroll
            for (int u = 0; u < EW_U; ++u) {
                const int64_t i = base + u * EW_THREADS + threadIdx.x;
                if (i < nv) { x[u] = ew_load(a4 + i, nt); z[u] = ew_load(b4 + i, nt); }
            }
#pragma unroll
            for (int u = 0; u < EW_U; ++u) {
                const int64_t i = base + u * EW_THREADS + threadIdx.x;
                if (i < nv) {
                    float4 y;
                    y.x = f(x[u].x, z[u].x); y.y = f(x[u].y, z[u].y); y.z = f(x[u].z, z[u].z); y.w = f(x[u].w, z[u].w);
                    ew_store(o4 + i, y, nt);
                }
            }
        }
        for (int64_t i = (nv << 2) + gid; i < n; i += gsz) out[i] = f(a[i], b[i]);
    } else {
        for (int64_t i = gid; i < n; i += gsz) out[i] = f(a[i], b[i]);
    }
}

struct AddF { __device__ float operator()(float a, float b) const { return a + b; } };
struct MulF { __device__ float operator()(float a, float b) const { return a * b; } };

template <class F>
static int launch_map1(float* out, const float* a, int64_t n, F f, hipStream_t st, const char* nm) {
    if (n == 0) return 0;
    const bool vec = aligned16(out) && aligned16(a);
    hipLaunchKernelGGL(map1_kernel<F>, dim3(ew_blocks(vec ? ceil_div(n >> 2, EW_U) : n)), dim3(EW_THREADS), 0, st,
                       out, a, n, vec, f, ew_nt(n));
    NNHIP_LAUNCH_CHECK(nm);
    return 0;
}
template <class F>
static int launch_map1s(float* out, const float* a, int64_t n, F f, const float* sp, hipStream_t st, const char* nm) {
    if (n == 0) return 0;
    const bool vec = aligned16(out) && aligned16(a);
    hipLaunchKernelGGL(map1s_kernel<F>, dim3(ew_blocks(vec ? ceil_div(n >> 2, EW_U) : n)), dim3(EW_THREADS), 0, st,
                       out, a, n, vec, f, sp, ew_nt(n));
    NNHIP_LAUNCH_CHECK(nm);
    return 0;
}
template <class F>
static int launch_map2(float* out, const float* a, const float* b, int64_t n, F f, hipStream_t st,
                       const char* nm) {
    if (n == 0) return 0;
    const bool vec = aligned16(out) && aligned16(a) && aligned16(b);
    hipLaunchKernelGGL(map2_kernel<F>, dim3(ew_blocks(vec ? ceil_div(n >> 2, EW_U) : n)), dim3(EW_THREADS), 0, st,
                       out, a, b, n, vec, f, ew_nt(n));
    NNHIP_LAUNCH_CHECK(nm);
    return 0;
}

}  // namespace nnhip
