// tensor_index.hip -- the rest of the Tensor tape (ABI 224): comparisons and logical ops, where, basic and integer-array indexing with
// their backward, flip, __setitem__ (basic, integer-array and boolean-mask keys).  neunet/autograd.py:642-808, 895-923.
//
// Everything here is a copy, a select or a comparison: exact, so the tests ask for bit equality with NumPy.  The only sums are the
// gradients of a broadcast `where` operand, and those are the reduction kernels of tensor_ops.h with the select as their load functor.
// Shapes, strides and index descriptions reach every kernel by value (tensor_ops.h: TDims and the small structs below): no upload, every
// entry may be captured.  No float atomics; the one integer atomicMax (positions, for last-write-wins) has an order-free result.
//
// Tiers (nnhipTensorOpsLastTier reports them):
//   compare / logical / where forward
//     vec4      every tensor operand has the output's shape and is contiguous, n % 4 == 0, inputs 16-byte aligned: four results per
//               lane -- comparisons store them as ONE 32-bit word, where as one float4
//     general   broadcasting, odd sizes, odd alignment: one result per lane, offsets from the collapsed groups (64-bit divisions)
//   where backward: tensor_ops.h's launch_ew (the operand was not broadcast) or launch_reduce (it was: its gradient is summed over
//               the broadcast axes inside the launch that forms it)
//   slice forward (getitem with a basic key, flip, and their mirror images): a strided copy from x + offset with SIGNED strides.
//               4-byte elements are launch_ew's copy (float32 and int32 by bits: vec2d when at most two groups remain and the innermost
//               stride is 1 -- x[:, -1], x[:, ::2] --, else general -- a flipped middle axis keeps three groups);
//               1- and 8-byte elements take the typed general kernel
//   slice backward: ONE launch walks dX in memory order and writes every element once -- grad where the element lies on the selected
//               lattice, 0 elsewhere; float4 stores when the innermost group is taken whole (slice-vec), else one element per lane
//   strided assign (setitem with a basic key): lanes walk the selected region, stores go to out + offset with signed strides
//   gather (getitem with integer arrays on adjacent axes): x [outer, D1..Dk, inner] -> out [outer, M, inner]
//     row       inner >= 16: a wave per output row, lanes along inner, 16 bytes per lane when 4-byte elements allow
//     element   inner == 1: a lane per output
//     general   in between: a lane per output element
//   index assign (the gather's backward and setitem with the same key): a `last` table over D1*..*Dk in the library workspace, filled
//               with -1 on EVERY call, atomicMax of the positions 0..M-1, then one pass over the destination: three launches.  The
//               reference ASSIGNS (`_grad[index] = grad`), so the last occurrence in C order wins -- embedding.hip's scheme.
//   masked assign (setitem with a boolean mask): one launch, a lane per destination element, no compaction
// An index outside its axis (a device index tensor cannot be checked without a host read in the middle of a step) reads as 0 in the
// gather and is skipped by the assign: nnhipEmbeddingForward's rule.  Negative indices wrap inside the kernels.
#include <string.h>

#include "tensor_ops.h"

namespace nnhip {

// ---- typed loads ---------------------------------------------------------------------------------------------------------------
template <class C>
__device__ __forceinline__ C ti_load(const void* p, int dt, int64_t i) {
    switch (dt) {
        case NNHIP_DT_F32: return (C)static_cast<const float*>(p)[i];
        case NNHIP_DT_I32: return (C)static_cast<const int32_t*>(p)[i];
        case NNHIP_DT_I64: return (C)static_cast<const int64_t*>(p)[i];
        default: return (C)static_cast<const uint8_t*>(p)[i];
    }
}
template <class T> struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) Pack4 { T v[4]; };
template <class C, class T>
__device__ __forceinline__ void ti_unpack4(const void* p, int64_t i4, C x[4]) {
    const Pack4<T> v = static_cast<const Pack4<T>*>(p)[i4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = (C)v.v[k];
}
template <class C>
__device__ __forceinline__ void ti_load4(const void* p, int dt, int64_t i4, C x[4]) {
    switch (dt) {
        case NNHIP_DT_F32: ti_unpack4<C, float>(p, i4, x); break;
        case NNHIP_DT_I32: ti_unpack4<C, int32_t>(p, i4, x); break;
        case NNHIP_DT_I64: ti_unpack4<C, int64_t>(p, i4, x); break;
        default: ti_unpack4<C, uint8_t>(p, i4, x); break;
    }
}
// truth = value != 0: a NaN is true, -0.0 is false (NumPy)
__device__ __forceinline__ bool ti_truth(const void* p, int dt, int64_t i) {
    if (dt == NNHIP_DT_F32) return static_cast<const float*>(p)[i] != 0.0f;
    return ti_load<int64_t>(p, dt, i) != 0;
}
__device__ __forceinline__ void ti_truth4(const void* p, int dt, int64_t i4, bool t[4]) {
    if (dt == NNHIP_DT_F32) {
        float x[4];
        ti_unpack4<float, float>(p, i4, x);
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = x[k] != 0.0f;
    } else {
        int64_t x[4];
        ti_load4<int64_t>(p, dt, i4, x);
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = x[k] != 0;
    }
}
// A NaN makes every kind false except NE; -0.0 == 0.0 (IEEE comparisons, which is what NumPy does)
template <class C>
__device__ __forceinline__ bool ti_cmp(int kind, C a, C b) {
    switch (kind) {
        case NNHIP_CMP_EQ: return a == b;
        case NNHIP_CMP_NE: return a != b;
        case NNHIP_CMP_GT: return a > b;
        case NNHIP_CMP_GE: return a >= b;
        case NNHIP_CMP_LT: return a < b;
        default: return a <= b;
    }
}
__device__ __forceinline__ bool ti_logic(int kind, bool a, bool b) {
    return kind == NNHIP_LOGICAL_AND ? (a && b) : (kind == NNHIP_LOGICAL_OR ? (a || b) : !a);
}
__device__ __forceinline__ uint32_t ti_word(const bool r[4]) {
    return (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
}

// ---- comparisons: C is the type the comparison is made in (float | int64 | double) -----------------------------------------------------
template <class C>
__global__ __launch_bounds__(256) void cmp_vec4_kernel(uint32_t* __restrict__ out, const void* __restrict__ a, const void* __restrict__ b,
                                                       C sv, int dt, int kind, int64_t n4) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += gsz) {
        C x[4] = {sv, sv, sv, sv}, y[4] = {sv, sv, sv, sv};
        if (a) ti_load4<C>(a, dt, i, x);
        if (b) ti_load4<C>(b, dt, i, y);
        bool r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = ti_cmp<C>(kind, x[k], y[k]);
        out[i] = ti_word(r);
    }
}
template <class C>
__global__ __launch_bounds__(256) void cmp_general_kernel(uint8_t* __restrict__ out, const void* __restrict__ a, const void* __restrict__ b,
                                                          C sv, int dt, int kind, TDims d, int64_t n) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        int64_t o0, o1, o2;
        to_offsets(d, i, o0, o1, o2);
        const C x = a ? ti_load<C>(a, dt, o0) : sv, y = b ? ti_load<C>(b, dt, o1) : sv;
        out[i] = ti_cmp<C>(kind, x, y) ? 1 : 0;
    }
}
__global__ __launch_bounds__(256) void logical_vec4_kernel(uint32_t* __restrict__ out, const void* __restrict__ a, const void* __restrict__ b,
                                                           int dta, int dtb, int kind, int64_t n4) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += gsz) {
        bool x[4], y[4] = {false, false, false, false}, r[4];
        ti_truth4(a, dta, i, x);
        if (b) ti_truth4(b, dtb, i, y);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = ti_logic(kind, x[k], y[k]);
        out[i] = ti_word(r);
    }
}
__global__ __launch_bounds__(256) void logical_general_kernel(uint8_t* __restrict__ out, const void* __restrict__ a, const void* __restrict__ b,
                                                              int dta, int dtb, int kind, TDims d, int64_t n) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        int64_t o0, o1, o2;
        to_offsets(d, i, o0, o1, o2);
        const bool x = ti_truth(a, dta, o0), y = b ? ti_truth(b, dtb, o1) : false;
        out[i] = ti_logic(kind, x, y) ? 1 : 0;
    }
}

// ---- where ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void where_vec4_kernel(float4* __restrict__ out, const void* __restrict__ cond, int cdt,
                                                         const float* __restrict__ a, const float* __restrict__ b, float sa, float sb, int64_t n4) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += gsz) {
        bool t[4];
        ti_truth4(cond, cdt, i, t);
        const float4 x = a ? reinterpret_cast<const float4*>(a)[i] : make_float4(sa, sa, sa, sa);
        const float4 y = b ? reinterpret_cast<const float4*>(b)[i] : make_float4(sb, sb, sb, sb);
        out[i] = make_float4(t[0] ? x.x : y.x, t[1] ? x.y : y.y, t[2] ? x.z : y.z, t[3] ? x.w : y.w);
    }
}
// d.s[0]: cond, d.s[1]: a, d.s[2]: b
__global__ __launch_bounds__(256) void where_general_kernel(float* __restrict__ out, const void* __restrict__ cond, int cdt,
                                                            const float* __restrict__ a, const float* __restrict__ b, float sa, float sb,
                                                            TDims d, int64_t n) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        int64_t o0, o1, o2;
        to_offsets(d, i, o0, o1, o2);
        out[i] = ti_truth(cond, cdt, o0) ? (a ? a[o1] : sa) : (b ? b[o2] : sb);
    }
}
// the gradient's select on (g, cond, -): SEL true -> the operand taken where cond holds.  A select, never a multiply: an inf or a NaN in g
// where the operand did not supply the value gives exactly 0.  CT: the condition's dtype; an int32 condition travels behind the float
// pointer and is tested by its bits, a byte condition is read by tensor_ops.h's byte loader.
template <int CT, bool SEL> struct WSel {
    static constexpr bool U0 = true, U1 = true, U2 = false, BYTE1 = CT == NNHIP_DT_U8;
    __device__ float operator()(float g, float c, float) const {
        const bool t = CT == NNHIP_DT_I32 ? __float_as_int(c) != 0 : c != 0.0f;
        return t == SEL ? g : 0.0f;
    }
};

// ---- typed copies -------------------------------------------------------------------------------------------------------------------
// out contiguous over d.ext, in at d.s[0] (signed)
template <class T>
__global__ __launch_bounds__(256) void copy_general_kernel(T* __restrict__ out, const T* __restrict__ in, TDims d, int64_t n) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        int64_t o0, o1, o2;
        to_offsets(d, i, o0, o1, o2);
        out[i] = in[o0];
    }
}
// the selected region is d.ext; out at d.s[0] (signed, never 0), in at d.s[1] (0 on broadcast axes) or the scalar
template <class T>
__global__ __launch_bounds__(256) void assign_kernel(T* __restrict__ out, const T* __restrict__ in, T sv, TDims d, int64_t n) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        int64_t o0, o1, o2;
        to_offsets(d, i, o0, o1, o2);
        out[o0] = in ? in[o1] : sv;
    }
}

// ---- slice backward ---------------------------------------------------------------------------------------------------------------
// dX's groups (outermost first): extent, and the lattice start + j * step, 0 <= j < count, with the gradient's stride per j
struct SliceDims {
    int nd;
    int64_t ext[TO_MAXG], start[TO_MAXG], step[TO_MAXG], count[TO_MAXG], gs[TO_MAXG];
};
// VEC: the innermost group is taken whole (start 0, step 1, count == ext), ext % 4 == 0, both bases 16-byte aligned; n counts float4s
template <bool VEC>
__global__ __launch_bounds__(256) void slice_bwd_kernel(float* __restrict__ dX, const float* __restrict__ g, SliceDims d, int64_t n) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    const int last = d.nd - 1;
    const int64_t e_last = VEC ? d.ext[last] / 4 : d.ext[last];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        int64_t rem = i / e_last, go = 0;
        const int64_t c_last = i - rem * e_last;
        bool on = true;
        if (VEC) {
            go = 4 * c_last;
        } else {
            const int64_t r = c_last - d.start[last], q = r / d.step[last];
            on = q * d.step[last] == r && q >= 0 && q < d.count[last];
            go = q * d.gs[last];
        }
#pragma unroll
        for (int k = TO_MAXG - 2; k >= 0; --k) {
            if (k < last) {
                const int64_t qq = rem / d.ext[k], c = rem - qq * d.ext[k];
                const int64_t r = c - d.start[k], q = r / d.step[k];
                on = on && q * d.step[k] == r && q >= 0 && q < d.count[k];
                go += q * d.gs[k];
                rem = qq;
            }
        }
        if (VEC) reinterpret_cast<float4*>(dX)[i] = on ? *reinterpret_cast<const float4*>(g + go) : make_float4(0.f, 0.f, 0.f, 0.f);
        else dX[i] = on ? g[go] : 0.0f;
    }
}

// ---- integer-array indexing -----------------------------------------------------------------------------------------------------------
struct GIdx {
    const void* p[NNHIP_INDEX_MAX_ARRAYS];      // k index arrays of M elements each (broadcast on the host side of the call)
    int64_t dim[NNHIP_INDEX_MAX_ARRAYS];        // the extents D1..Dk they index
    int k, dt;                                  // dt: NNHIP_DT_I32 or NNHIP_DT_I64
};
// position m -> row of the flattened [D1*..*Dk] axis, or -1 when an index lies outside its axis (negative indices wrap)
__device__ __forceinline__ int64_t gi_row(const GIdx& gi, int64_t m) {
    int64_t lin = 0;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NNHIP_INDEX_MAX_ARRAYS; ++j) {
        if (j < gi.k) {
            int64_t v = gi.dt == NNHIP_DT_I64 ? static_cast<const int64_t*>(gi.p[j])[m] : (int64_t)static_cast<const int32_t*>(gi.p[j])[m];
            if (v < 0) v += gi.dim[j];
            ok = ok && v >= 0 && v < gi.dim[j];
            lin = lin * gi.dim[j] + v;
        }
    }
    return ok ? lin : -1;
}
// row: a wave per output row (o, m); V: the lane's unit (T itself, or a 16-byte pack of four 4-byte elements)
template <class V>
__global__ __launch_bounds__(256) void gather_row_kernel(V* __restrict__ out, const V* __restrict__ x, GIdx gi, int64_t outer, int64_t M,
                                                         int64_t P, int64_t inner_v) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= outer * M) return;                     // wave-uniform
    const int lane = threadIdx.x & 63;
    const int64_t o = row / M, m = row - o * M;
    const int64_t r = gi_row(gi, m);
    V* dst = out + row * inner_v;
    const V* src = x + (o * P + (r >= 0 ? r : 0)) * inner_v;
    for (int64_t c = lane; c < inner_v; c += 64) dst[c] = r >= 0 ? src[c] : V{};
}
// element (inner == 1) and general (1 < inner < 16): a lane per output element
template <class T, bool INNER1>
__global__ __launch_bounds__(256) void gather_elem_kernel(T* __restrict__ out, const T* __restrict__ x, GIdx gi, int64_t outer, int64_t M,
                                                          int64_t P, int64_t inner) {
    const int64_t n = outer * M * inner, gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        int64_t row = i, c = 0;
        if (!INNER1) { row = i / inner; c = i - row * inner; }
        const int64_t o = row / M, m = row - o * M;
        const int64_t r = gi_row(gi, m);
        out[i] = r >= 0 ? x[(o * P + r) * inner + c] : T{};
    }
}
__global__ __launch_bounds__(256) void index_fill_kernel(int32_t* __restrict__ p, int64_t n, int32_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ __launch_bounds__(256) void index_last_kernel(GIdx gi, int64_t M, int32_t* __restrict__ last) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int64_t r = gi_row(gi, m);
    if (r >= 0) atomicMax(&last[r], (int32_t)m);
}
// one pass over dst [outer, P, inner]: row (o, p) <- src row (o, last[p]) (or the scalar) when last[p] >= 0; otherwise zero (ZERO:
// the gather's backward, every element is written) or left alone (setitem)
template <class V, bool ZERO>
__global__ __launch_bounds__(256) void index_assign_row_kernel(V* __restrict__ dst, const V* __restrict__ src, V sv, const int32_t* __restrict__ last,
                                                               int64_t outer, int64_t M, int64_t P, int64_t inner_v) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= outer * P) return;
    const int lane = threadIdx.x & 63;
    const int64_t o = row / P, p = row - o * P;
    const int32_t l = last[p];
    if (l < 0 && !ZERO) return;
    V* d = dst + row * inner_v;
    const V* s = src ? src + (o * M + (l >= 0 ? l : 0)) * inner_v : nullptr;
    for (int64_t c = lane; c < inner_v; c += 64) d[c] = l >= 0 ? (s ? s[c] : sv) : V{};
}
template <class T, bool ZERO>
__global__ __launch_bounds__(256) void index_assign_elem_kernel(T* __restrict__ dst, const T* __restrict__ src, T sv, const int32_t* __restrict__ last,
                                                                int64_t outer, int64_t M, int64_t P, int64_t inner) {
    const int64_t n = outer * P * inner, gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        const int64_t row = i / inner, c = i - row * inner;
        const int64_t o = row / P, p = row - o * P;
        const int32_t l = last[p];
        if (l >= 0) dst[i] = src ? src[(o * M + l) * inner + c] : sv;
        else if (ZERO) dst[i] = T{};
    }
}
// dst [rows, inner], mask [rows] bytes: dst[r, c] = mask[r] ? (val ? val[c] : sv) : unchanged
template <class T>
__global__ __launch_bounds__(256) void masked_assign_kernel(T* __restrict__ dst, const uint8_t* __restrict__ mask, const T* __restrict__ val, T sv,
                                                            int64_t rows, int64_t inner) {
    const int64_t n = rows * inner, gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        const int64_t r = i / inner, c = i - r * inner;
        if (mask[r]) dst[i] = val ? val[c] : sv;
    }
}

// ---- host helpers ---------------------------------------------------------------------------------------------------------------------
struct U128 { uint32_t v[4]; } __attribute__((aligned(16)));      // four 4-byte elements by bits

static int64_t dt_size(int dt) { return dt == NNHIP_DT_I64 ? 8 : (dt == NNHIP_DT_U8 ? 1 : 4); }
static bool dt_ok(int dt) { return dt >= NNHIP_DT_F32 && dt <= NNHIP_DT_U8; }
static bool dt_aligned(const void* p, int dt) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(dt_size(dt) - 1)) == 0; }
#define TI_PTR(fn, p, dt)                                                               \
    do {                                                                                \
        NNHIP_CHECK_ARG((p) != nullptr, NNHIP_EINVAL, fn ": null pointer");              \
        NNHIP_CHECK_ARG(dt_aligned(p, dt), NNHIP_EALIGN, fn ": misaligned pointer");     \
    } while (0)

template <class C>
static int compare_launch(int kind, uint8_t* out, const void* a, const void* b, C sv, int dt, const TDims& d, int64_t n, hipStream_t st) {
    const bool vec = n % 4 == 0 && aligned4(out) && (!a || ((is_full(d, 0) || n == 1) && aligned16(a))) &&
                     (!b || ((is_full(d, 1) || n == 1) && aligned16(b)));
    if (vec) {
        note_tier(NNHIP_TIER_IDX_VEC4);
        hipLaunchKernelGGL(cmp_vec4_kernel<C>, dim3(grid_for(n / 4)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(out), a, b, sv, dt, kind, n / 4);
    } else {
        note_tier(NNHIP_TIER_IDX_GENERAL);
        hipLaunchKernelGGL(cmp_general_kernel<C>, dim3(grid_for(n)), dim3(256), 0, st, out, a, b, sv, dt, kind, d, n);
    }
    NNHIP_LAUNCH_CHECK("compare");
    return 0;
}

template <class G>
static int where_grad(float* dst, const TIn& in, const int64_t* shape, const int64_t* const* strides, const int64_t* op_stride, int rank,
                      hipStream_t st) {
    int32_t red[TO_MAXRANK];
    bool any = false;
    for (int i = 0; i < rank; ++i) { red[i] = shape[i] > 1 && op_stride[i] == 0; any = any || red[i]; }
    TDims d;
    int64_t n;
    if (collapse(rank, shape, strides, 2, any ? red : nullptr, d, n) != 0) { set_last_error("nnhipWhereBackward: more than %d axis groups", TO_MAXG); return NNHIP_EINVAL; }
    if (!any) return launch_ew(dst, in, d, n, G{}, st, "where_backward");
    return launch_reduce<G, SumC, false>(in, d, dst, nullptr, 1.0f, G{}, st, "where_backward_reduce");
}

template <class T>
static int copy_typed(void* out, const void* in, const TDims& d, int64_t n, hipStream_t st) {
    note_tier(NNHIP_TIER_IDX_GENERAL);
    hipLaunchKernelGGL(copy_general_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, static_cast<T*>(out), static_cast<const T*>(in), d, n);
    NNHIP_LAUNCH_CHECK("slice_copy");
    return 0;
}
template <class T>
static int assign_typed(void* out, const void* in, T sv, const TDims& d, int64_t n, hipStream_t st) {
    note_tier(NNHIP_TIER_IDX_GENERAL);
    hipLaunchKernelGGL(assign_kernel<T>, dim3(grid_for(n)), dim3(256), 0, st, static_cast<T*>(out), static_cast<const T*>(in), sv, d, n);
    NNHIP_LAUNCH_CHECK("strided_assign");
    return 0;
}
template <class T>
static T scalar_as(double v, int64_t iv, int is_int) { return is_int ? (T)iv : (T)v; }
template <>
uint8_t scalar_as<uint8_t>(double v, int64_t iv, int is_int) { return (is_int ? iv != 0 : v != 0.0) ? 1 : 0; }      // bool storage

static int check_index(const char* fn, const void* const* idx, int idx_dtype, int k, const int64_t* dims, int64_t outer, int64_t M, int64_t inner,
                       GIdx& gi, int64_t& P) {
    NNHIP_CHECK_ARG(k >= 1 && k <= NNHIP_INDEX_MAX_ARRAYS, NNHIP_EINVAL, "%s: %d index arrays (1..%d)", fn, k, NNHIP_INDEX_MAX_ARRAYS);
    NNHIP_CHECK_ARG(idx_dtype == NNHIP_DT_I32 || idx_dtype == NNHIP_DT_I64, NNHIP_EINVAL, "%s: index arrays are int32 or int64", fn);
    NNHIP_CHECK_ARG(idx && dims, NNHIP_EINVAL, "%s: null index description", fn);
    NNHIP_CHECK_ARG(outer >= 0 && M >= 0 && inner >= 0, NNHIP_EINVAL, "%s: negative size", fn);
    NNHIP_CHECK_ARG(M < ((int64_t)1 << 31), NNHIP_EINVAL, "%s: more index positions than int32 can address", fn);
    gi = GIdx{};
    gi.k = k; gi.dt = idx_dtype;
    P = 1;
    for (int j = 0; j < k; ++j) {
        NNHIP_CHECK_ARG(dims[j] >= 0, NNHIP_EINVAL, "%s: negative extent", fn);
        gi.dim[j] = dims[j];
        gi.p[j] = idx[j];
        P *= dims[j];
        if (M > 0) {
            NNHIP_CHECK_ARG(idx[j] != nullptr, NNHIP_EINVAL, "%s: null index array", fn);
            NNHIP_CHECK_ARG(dt_aligned(idx[j], idx_dtype), NNHIP_EALIGN, "%s: misaligned index array", fn);
        }
    }
    return 0;
}

template <class T, bool ZERO>
static int index_assign_pass(void* dst, const void* src, T sv, const int32_t* last, int64_t outer, int64_t M, int64_t P, int64_t inner, hipStream_t st) {
    const int64_t rows = outer * P;
    if (inner >= 16) {
        NNHIP_CHECK_ARG(ceil_div(rows, 4) < ((int64_t)1 << 31), NNHIP_EINVAL, "nnhipIndexAssign: too many rows");
        bool vec = false;
        if constexpr (sizeof(T) == 4) {
            vec = inner % 4 == 0 && aligned16(dst) && (!src || aligned16(src));
            if (vec) {
                const U128 sv4{{(uint32_t)sv, (uint32_t)sv, (uint32_t)sv, (uint32_t)sv}};
                note_tier(NNHIP_TIER_IDX_ROW_VEC);
                hipLaunchKernelGGL((index_assign_row_kernel<U128, ZERO>), dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, st, static_cast<U128*>(dst),
                                   static_cast<const U128*>(src), sv4, last, outer, M, P, inner / 4);
            }
        }
        if (!vec) {
            note_tier(NNHIP_TIER_IDX_ROW);
            hipLaunchKernelGGL((index_assign_row_kernel<T, ZERO>), dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, st, static_cast<T*>(dst),
                               static_cast<const T*>(src), sv, last, outer, M, P, inner);
        }
    } else {
        note_tier(inner == 1 ? NNHIP_TIER_IDX_ELEMENT : NNHIP_TIER_IDX_GENERAL);
        hipLaunchKernelGGL((index_assign_elem_kernel<T, ZERO>), dim3(grid_for(rows * inner)), dim3(256), 0, st, static_cast<T*>(dst),
                           static_cast<const T*>(src), sv, last, outer, M, P, inner);
    }
    NNHIP_LAUNCH_CHECK("index_assign");
    return 0;
}
template <class T>
static int index_assign_typed(void* dst, const void* src, T sv, int zero_fill, const int32_t* last, int64_t outer, int64_t M, int64_t P, int64_t inner,
                              hipStream_t st) {
    return zero_fill ? index_assign_pass<T, true>(dst, src, sv, last, outer, M, P, inner, st)
                     : index_assign_pass<T, false>(dst, src, sv, last, outer, M, P, inner, st);
}

template <class T>
static int gather_typed(void* out, const void* x, const GIdx& gi, int64_t outer, int64_t M, int64_t P, int64_t inner, hipStream_t st) {
    const int64_t rows = outer * M;
    if (inner >= 16) {
        NNHIP_CHECK_ARG(ceil_div(rows, 4) < ((int64_t)1 << 31), NNHIP_EINVAL, "nnhipIndexGather: too many rows");
        if (sizeof(T) == 4 && inner % 4 == 0 && aligned16(out) && aligned16(x)) {
            note_tier(NNHIP_TIER_IDX_ROW_VEC);
            hipLaunchKernelGGL(gather_row_kernel<U128>, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, st, static_cast<U128*>(out),
                               static_cast<const U128*>(x), gi, outer, M, P, inner / 4);
        } else {
            note_tier(NNHIP_TIER_IDX_ROW);
            hipLaunchKernelGGL(gather_row_kernel<T>, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, st, static_cast<T*>(out),
                               static_cast<const T*>(x), gi, outer, M, P, inner);
        }
    } else if (inner == 1) {
        note_tier(NNHIP_TIER_IDX_ELEMENT);
        hipLaunchKernelGGL((gather_elem_kernel<T, true>), dim3(grid_for(rows)), dim3(256), 0, st, static_cast<T*>(out), static_cast<const T*>(x), gi,
                           outer, M, P, inner);
    } else {
        note_tier(NNHIP_TIER_IDX_GENERAL);
        hipLaunchKernelGGL((gather_elem_kernel<T, false>), dim3(grid_for(rows * inner)), dim3(256), 0, st, static_cast<T*>(out),
                           static_cast<const T*>(x), gi, outer, M, P, inner);
    }
    NNHIP_LAUNCH_CHECK("index_gather");
    return 0;
}

}  // namespace nnhip

using namespace nnhip;

// by element size: float32 and int32 share the 4-byte instances (copies by bits)
#define TI_BY_SIZE(dt, CALL)                                     \
    switch (dt_size(dt)) {                                       \
        case 8: { using T = uint64_t; return CALL; }             \
        case 1: { using T = uint8_t; return CALL; }              \
        default: { using T = uint32_t; return CALL; }            \
    }

extern "C" int nnhipCompare(int kind, uint8_t* out, const void* a, const void* b, double scalar, int64_t scalar_i64, int scalar_is_int, int dtype,
                            int rank, const int64_t* shape, const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t s) {
    NNHIP_CHECK_ARG(kind >= NNHIP_CMP_EQ && kind <= NNHIP_CMP_LE, NNHIP_EINVAL, "nnhipCompare: unknown kind %d", kind);
    NNHIP_CHECK_ARG(dt_ok(dtype), NNHIP_EINVAL, "nnhipCompare: unknown dtype %d", dtype);
    TO_CHECK_DIMS("nnhipCompare", rank, shape);
    NNHIP_CHECK_ARG(a != nullptr || b != nullptr, NNHIP_EINVAL, "nnhipCompare: null pointer (both operands)");
    NNHIP_CHECK_ARG(rank == 0 || ((stride_a || !a) && (stride_b || !b)), NNHIP_EINVAL, "nnhipCompare: null strides");
    int64_t zeros[TO_MAXRANK] = {0};
    const int64_t* strides[2] = {a ? stride_a : zeros, b ? stride_b : zeros};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 2, nullptr, d, n) == 0, NNHIP_EINVAL, "nnhipCompare: more than %d axis groups", TO_MAXG);
    if (n == 0) return 0;
    NNHIP_CHECK_ARG(out != nullptr, NNHIP_EINVAL, "nnhipCompare: null pointer");
    if (a) TI_PTR("nnhipCompare", a, dtype);
    if (b) TI_PTR("nnhipCompare", b, dtype);
    hipStream_t st = (hipStream_t)s;
    const bool has_scalar = !a || !b;
    // NumPy 2: a Python scalar against float32 is rounded to float32 first; an integer tensor against a Python int compares in int64,
    // against a Python float in double.  Two tensors share a dtype (the host refuses mixed pairs).
    if (dtype == NNHIP_DT_F32) return compare_launch<float>(kind, out, a, b, scalar_is_int ? (float)scalar_i64 : (float)scalar, dtype, d, n, st);
    if (has_scalar && !scalar_is_int) return compare_launch<double>(kind, out, a, b, scalar, dtype, d, n, st);
    return compare_launch<int64_t>(kind, out, a, b, scalar_i64, dtype, d, n, st);
}

extern "C" int nnhipLogical(int kind, uint8_t* out, const void* a, const void* b, int dtype_a, int dtype_b, int rank, const int64_t* shape,
                            const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t s) {
    NNHIP_CHECK_ARG(kind >= NNHIP_LOGICAL_AND && kind <= NNHIP_LOGICAL_NOT, NNHIP_EINVAL, "nnhipLogical: unknown kind %d", kind);
    const bool unary = kind == NNHIP_LOGICAL_NOT;
    NNHIP_CHECK_ARG(dt_ok(dtype_a) && (unary || dt_ok(dtype_b)), NNHIP_EINVAL, "nnhipLogical: unknown dtype");
    TO_CHECK_DIMS("nnhipLogical", rank, shape);
    NNHIP_CHECK_ARG(rank == 0 || (stride_a && (unary || stride_b)), NNHIP_EINVAL, "nnhipLogical: null strides");
    if (unary) b = nullptr;
    int64_t zeros[TO_MAXRANK] = {0};
    const int64_t* strides[2] = {stride_a, b ? stride_b : zeros};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 2, nullptr, d, n) == 0, NNHIP_EINVAL, "nnhipLogical: more than %d axis groups", TO_MAXG);
    if (n == 0) return 0;
    NNHIP_CHECK_ARG(out != nullptr, NNHIP_EINVAL, "nnhipLogical: null pointer");
    TI_PTR("nnhipLogical", a, dtype_a);
    if (!unary) TI_PTR("nnhipLogical", b, dtype_b);
    hipStream_t st = (hipStream_t)s;
    const bool vec = n % 4 == 0 && aligned4(out) && (is_full(d, 0) || n == 1) && aligned16(a) && (!b || ((is_full(d, 1) || n == 1) && aligned16(b)));
    if (vec) {
        note_tier(NNHIP_TIER_IDX_VEC4);
        hipLaunchKernelGGL(logical_vec4_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(out), a, b, dtype_a, dtype_b, kind, n / 4);
    } else {
        note_tier(NNHIP_TIER_IDX_GENERAL);
        hipLaunchKernelGGL(logical_general_kernel, dim3(grid_for(n)), dim3(256), 0, st, out, a, b, dtype_a, dtype_b, kind, d, n);
    }
    NNHIP_LAUNCH_CHECK("logical");
    return 0;
}

static bool cond_dt_ok(int dt) { return dt == NNHIP_DT_F32 || dt == NNHIP_DT_I32 || dt == NNHIP_DT_U8; }

extern "C" int nnhipWhereForward(float* out, const void* cond, int cond_dtype, const float* a, const float* b, float scalar_a, float scalar_b, int rank,
                                 const int64_t* shape, const int64_t* stride_c, const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t s) {
    NNHIP_CHECK_ARG(cond_dt_ok(cond_dtype), NNHIP_EINVAL, "nnhipWhereForward: the condition is bool/uint8, int32 or float32");
    TO_CHECK_DIMS("nnhipWhereForward", rank, shape);
    NNHIP_CHECK_ARG(rank == 0 || (stride_c && (stride_a || !a) && (stride_b || !b)), NNHIP_EINVAL, "nnhipWhereForward: null strides");
    int64_t zeros[TO_MAXRANK] = {0};
    const int64_t* strides[3] = {rank ? stride_c : zeros, a ? stride_a : zeros, b ? stride_b : zeros};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 3, nullptr, d, n) == 0, NNHIP_EINVAL, "nnhipWhereForward: more than %d axis groups", TO_MAXG);
    if (n == 0) return 0;
    TO_PTR("nnhipWhereForward", out);
    TI_PTR("nnhipWhereForward", cond, cond_dtype);
    if (a) TO_PTR("nnhipWhereForward", a);
    if (b) TO_PTR("nnhipWhereForward", b);
    hipStream_t st = (hipStream_t)s;
    const bool one = n == 1;
    const bool vec = n % 4 == 0 && aligned16(out) && (is_full(d, 0) || one) && aligned16(cond) && (!a || ((is_full(d, 1) || one) && aligned16(a))) &&
                     (!b || ((is_full(d, 2) || one) && aligned16(b)));
    if (vec) {
        note_tier(NNHIP_TIER_IDX_VEC4);
        hipLaunchKernelGGL(where_vec4_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, reinterpret_cast<float4*>(out), cond, cond_dtype, a, b, scalar_a,
                           scalar_b, n / 4);
    } else {
        note_tier(NNHIP_TIER_IDX_GENERAL);
        hipLaunchKernelGGL(where_general_kernel, dim3(grid_for(n)), dim3(256), 0, st, out, cond, cond_dtype, a, b, scalar_a, scalar_b, d, n);
    }
    NNHIP_LAUNCH_CHECK("where_forward");
    return 0;
}

extern "C" int nnhipWhereBackward(float* dA, float* dB, const float* grad, const void* cond, int cond_dtype, int rank, const int64_t* shape,
                                  const int64_t* stride_c, const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t s) {
    NNHIP_CHECK_ARG(cond_dt_ok(cond_dtype), NNHIP_EINVAL, "nnhipWhereBackward: the condition is bool/uint8, int32 or float32");
    TO_CHECK_DIMS("nnhipWhereBackward", rank, shape);
    NNHIP_CHECK_ARG(rank == 0 || (stride_c && (stride_a || !dA) && (stride_b || !dB)), NNHIP_EINVAL, "nnhipWhereBackward: null strides");
    int64_t total = 1;
    for (int i = 0; i < rank; ++i) total *= shape[i];
    if (total == 0 || (!dA && !dB)) return 0;
    TO_PTR("nnhipWhereBackward", grad);
    TI_PTR("nnhipWhereBackward", cond, cond_dtype);
    if (dA) TO_PTR("nnhipWhereBackward", dA);
    if (dB) TO_PTR("nnhipWhereBackward", dB);
    int64_t zeros[TO_MAXRANK] = {0}, full[TO_MAXRANK];
    int64_t acc = 1;
    for (int i = rank - 1; i >= 0; --i) { full[i] = acc; acc *= shape[i]; }
    const int64_t* strides[2] = {full, rank ? stride_c : zeros};
    TIn in{{grad, static_cast<const float*>(cond), nullptr}, 0.0f};
    hipStream_t st = (hipStream_t)s;
    int rc = 0;
#define TI_WGRAD(CT)                                                                                              \
    do {                                                                                                          \
        if (dA) rc = where_grad<WSel<CT, true>>(dA, in, shape, strides, stride_a, rank, st);                       \
        if (rc == 0 && dB) rc = where_grad<WSel<CT, false>>(dB, in, shape, strides, stride_b, rank, st);           \
    } while (0)
    if (cond_dtype == NNHIP_DT_U8) TI_WGRAD(NNHIP_DT_U8);
    else if (cond_dtype == NNHIP_DT_I32) TI_WGRAD(NNHIP_DT_I32);
    else TI_WGRAD(NNHIP_DT_F32);
#undef TI_WGRAD
    return rc;
}

extern "C" int nnhipSliceForward(void* out, const void* in, int64_t offset, int dtype, int rank, const int64_t* shape, const int64_t* stride_in,
                                 nnhipStream_t s) {
    NNHIP_CHECK_ARG(dt_ok(dtype), NNHIP_EINVAL, "nnhipSliceForward: unknown dtype %d", dtype);
    TO_CHECK_DIMS("nnhipSliceForward", rank, shape);
    NNHIP_CHECK_ARG(rank == 0 || stride_in, NNHIP_EINVAL, "nnhipSliceForward: null strides");
    const int64_t* strides[1] = {stride_in};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 1, nullptr, d, n) == 0, NNHIP_EINVAL, "nnhipSliceForward: more than %d axis groups", TO_MAXG);
    if (n == 0) return 0;
    TI_PTR("nnhipSliceForward", out, dtype);
    TI_PTR("nnhipSliceForward", in, dtype);
    hipStream_t st = (hipStream_t)s;
    if (dt_size(dtype) == 4) {          // float32 and int32: launch_ew's copy, by bits
        TIn ti{{static_cast<const float*>(in) + offset, nullptr, nullptr}, 0.0f};
        return launch_ew(static_cast<float*>(out), ti, d, n, CopyF{}, st, "slice_copy");
    }
    if (dt_size(dtype) == 8) return copy_typed<uint64_t>(out, static_cast<const uint64_t*>(in) + offset, d, n, st);
    return copy_typed<uint8_t>(out, static_cast<const uint8_t*>(in) + offset, d, n, st);
}

extern "C" int nnhipSliceBackward(float* dX, const float* grad, int rank, const int64_t* x_shape, const int64_t* start, const int64_t* step,
                                  const int64_t* count, nnhipStream_t s) {
    TO_CHECK_DIMS("nnhipSliceBackward", rank, x_shape);
    NNHIP_CHECK_ARG(rank == 0 || (start && step && count), NNHIP_EINVAL, "nnhipSliceBackward: null lattice description");
    int64_t total = 1, gtotal = 1;
    for (int i = 0; i < rank; ++i) {
        total *= x_shape[i];
        gtotal *= count[i];
        NNHIP_CHECK_ARG(count[i] >= 0 && step[i] != 0, NNHIP_EINVAL, "nnhipSliceBackward: a negative count or a zero step");
        if (count[i] > 0) {
            const int64_t lastc = start[i] + (count[i] - 1) * step[i];
            NNHIP_CHECK_ARG(start[i] >= 0 && start[i] < x_shape[i] && lastc >= 0 && lastc < x_shape[i], NNHIP_EINVAL,
                            "nnhipSliceBackward: the lattice of axis %d leaves the tensor", i);
        }
    }
    if (total == 0) return 0;
    TO_PTR("nnhipSliceBackward", dX);
    if (gtotal > 0) TO_PTR("nnhipSliceBackward", grad);
    // groups: axes of extent 1 drop out, adjacent axes taken whole merge
    SliceDims d{};
    int n = 0;
    bool prev_full = false;
    int64_t gs = 1, gstride[TO_MAXRANK];
    for (int i = rank - 1; i >= 0; --i) { gstride[i] = gs; gs *= count[i]; }
    for (int i = 0; i < rank; ++i) {
        if (x_shape[i] == 1) continue;
        const bool full = start[i] == 0 && step[i] == 1 && count[i] == x_shape[i];
        if (n > 0 && full && prev_full) {
            d.ext[n - 1] *= x_shape[i]; d.count[n - 1] = d.ext[n - 1]; d.gs[n - 1] = gstride[i];
        } else {
            NNHIP_CHECK_ARG(n < TO_MAXG, NNHIP_EINVAL, "nnhipSliceBackward: more than %d axis groups", TO_MAXG);
            d.ext[n] = x_shape[i]; d.start[n] = start[i]; d.step[n] = step[i]; d.count[n] = count[i]; d.gs[n] = gstride[i];
            ++n;
        }
        prev_full = full;
    }
    if (n == 0) { d.ext[0] = 1; d.start[0] = 0; d.step[0] = 1; d.count[0] = 1; d.gs[0] = 1; n = 1; prev_full = true; }
    d.nd = n;
    if (gtotal == 0) d.count[0] = 0;            // an empty selection: every element of dX is 0
    hipStream_t st = (hipStream_t)s;
    const bool vec = prev_full && gtotal > 0 && d.ext[n - 1] % 4 == 0 && aligned16(dX) && aligned16(grad);
    if (vec) {
        note_tier(NNHIP_TIER_SLICE_BWD_VEC);
        hipLaunchKernelGGL(slice_bwd_kernel<true>, dim3(grid_for(total / 4)), dim3(256), 0, st, dX, grad, d, total / 4);
    } else {
        note_tier(NNHIP_TIER_SLICE_BWD_SCALAR);
        hipLaunchKernelGGL(slice_bwd_kernel<false>, dim3(grid_for(total)), dim3(256), 0, st, dX, grad, d, total);
    }
    NNHIP_LAUNCH_CHECK("slice_backward");
    return 0;
}

extern "C" int nnhipStridedAssign(void* out, int64_t offset, const int64_t* stride_out, const void* in, const int64_t* stride_in, double scalar,
                                  int64_t scalar_i64, int scalar_is_int, int dtype, int rank, const int64_t* shape, nnhipStream_t s) {
    NNHIP_CHECK_ARG(dt_ok(dtype), NNHIP_EINVAL, "nnhipStridedAssign: unknown dtype %d", dtype);
    TO_CHECK_DIMS("nnhipStridedAssign", rank, shape);
    NNHIP_CHECK_ARG(rank == 0 || (stride_out && (stride_in || !in)), NNHIP_EINVAL, "nnhipStridedAssign: null strides");
    for (int i = 0; i < rank; ++i)
        NNHIP_CHECK_ARG(shape[i] <= 1 || stride_out[i] != 0, NNHIP_EINVAL, "nnhipStridedAssign: a zero destination stride (axis %d)", i);
    int64_t zeros[TO_MAXRANK] = {0};
    const int64_t* strides[2] = {rank ? stride_out : zeros, in ? stride_in : zeros};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 2, nullptr, d, n) == 0, NNHIP_EINVAL, "nnhipStridedAssign: more than %d axis groups", TO_MAXG);
    if (n == 0) return 0;
    TI_PTR("nnhipStridedAssign", out, dtype);
    if (in) TI_PTR("nnhipStridedAssign", in, dtype);
    hipStream_t st = (hipStream_t)s;
    switch (dtype) {
        case NNHIP_DT_F32: return assign_typed<float>(static_cast<float*>(out) + offset, in, scalar_as<float>(scalar, scalar_i64, scalar_is_int), d, n, st);
        case NNHIP_DT_I32: return assign_typed<int32_t>(static_cast<int32_t*>(out) + offset, in, scalar_as<int32_t>(scalar, scalar_i64, scalar_is_int), d, n, st);
        case NNHIP_DT_I64: return assign_typed<int64_t>(static_cast<int64_t*>(out) + offset, in, scalar_as<int64_t>(scalar, scalar_i64, scalar_is_int), d, n, st);
        default: return assign_typed<uint8_t>(static_cast<uint8_t*>(out) + offset, in, scalar_as<uint8_t>(scalar, scalar_i64, scalar_is_int), d, n, st);
    }
}

extern "C" int nnhipIndexGather(void* out, const void* x, int dtype, const void* const* idx, int idx_dtype, int k, const int64_t* dims, int64_t outer,
                                int64_t M, int64_t inner, nnhipStream_t s) {
    NNHIP_CHECK_ARG(dt_ok(dtype), NNHIP_EINVAL, "nnhipIndexGather: unknown dtype %d", dtype);
    GIdx gi;
    int64_t P;
    const int rc = check_index("nnhipIndexGather", idx, idx_dtype, k, dims, outer, M, inner, gi, P);
    if (rc) return rc;
    if (outer * M * inner == 0) return 0;
    TI_PTR("nnhipIndexGather", out, dtype);
    // P == 0 with M > 0: every index is out of range and reads as 0; x is then never dereferenced
    if (P > 0) TI_PTR("nnhipIndexGather", x, dtype);
    hipStream_t st = (hipStream_t)s;
    TI_BY_SIZE(dtype, gather_typed<T>(out, x, gi, outer, M, P, inner, st));
}

extern "C" int nnhipIndexAssign(void* dst, const void* src, double scalar, int64_t scalar_i64, int scalar_is_int, int dtype, int zero_fill,
                                const void* const* idx, int idx_dtype, int k, const int64_t* dims, int64_t outer, int64_t M, int64_t inner,
                                nnhipStream_t s) {
    NNHIP_CHECK_ARG(dt_ok(dtype), NNHIP_EINVAL, "nnhipIndexAssign: unknown dtype %d", dtype);
    GIdx gi;
    int64_t P;
    const int rc = check_index("nnhipIndexAssign", idx, idx_dtype, k, dims, outer, M, inner, gi, P);
    if (rc) return rc;
    if (outer * P * inner == 0) return 0;
    if (M == 0 && !zero_fill) return 0;
    TI_PTR("nnhipIndexAssign", dst, dtype);
    if (src) TI_PTR("nnhipIndexAssign", src, dtype);
    NNHIP_CHECK_ARG(ceil_div(P, 256) < ((int64_t)1 << 31), NNHIP_EINVAL, "nnhipIndexAssign: indexed extent too large");
    hipStream_t st = (hipStream_t)s;
    int32_t* last = static_cast<int32_t*>(workspace((size_t)P * sizeof(int32_t)));
    NNHIP_CHECK_ARG(last != nullptr, NNHIP_ENOMEM, "nnhipIndexAssign: workspace allocation failed");
    hipLaunchKernelGGL(index_fill_kernel, dim3((unsigned)ceil_div(P, 256)), dim3(256), 0, st, last, P, -1);
    NNHIP_LAUNCH_CHECK("index_fill_kernel");
    if (M > 0) {
        hipLaunchKernelGGL(index_last_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, st, gi, M, last);
        NNHIP_LAUNCH_CHECK("index_last_kernel");
    }
    switch (dtype) {
        case NNHIP_DT_I64: return index_assign_typed<uint64_t>(dst, src, (uint64_t)scalar_as<int64_t>(scalar, scalar_i64, scalar_is_int), zero_fill, last, outer, M, P, inner, st);
        case NNHIP_DT_U8: return index_assign_typed<uint8_t>(dst, src, scalar_as<uint8_t>(scalar, scalar_i64, scalar_is_int), zero_fill, last, outer, M, P, inner, st);
        case NNHIP_DT_I32: return index_assign_typed<uint32_t>(dst, src, (uint32_t)scalar_as<int32_t>(scalar, scalar_i64, scalar_is_int), zero_fill, last, outer, M, P, inner, st);
        default: {
            const float f = scalar_as<float>(scalar, scalar_i64, scalar_is_int);
            uint32_t bits;
            memcpy(&bits, &f, 4);
            return index_assign_typed<uint32_t>(dst, src, bits, zero_fill, last, outer, M, P, inner, st);
        }
    }
}

extern "C" int nnhipMaskedAssign(void* dst, const uint8_t* mask, const void* value, double scalar, int64_t scalar_i64, int scalar_is_int, int dtype,
                                 int64_t rows, int64_t inner, nnhipStream_t s) {
    NNHIP_CHECK_ARG(dt_ok(dtype), NNHIP_EINVAL, "nnhipMaskedAssign: unknown dtype %d", dtype);
    NNHIP_CHECK_ARG(rows >= 0 && inner >= 0, NNHIP_EINVAL, "nnhipMaskedAssign: negative size");
    if (rows * inner == 0) return 0;
    TI_PTR("nnhipMaskedAssign", dst, dtype);
    NNHIP_CHECK_ARG(mask != nullptr, NNHIP_EINVAL, "nnhipMaskedAssign: null pointer");
    if (value) TI_PTR("nnhipMaskedAssign", value, dtype);
    hipStream_t st = (hipStream_t)s;
    note_tier(NNHIP_TIER_IDX_GENERAL);
#define TI_MASKED(T)                                                                                                                         \
    hipLaunchKernelGGL(masked_assign_kernel<T>, dim3(grid_for(rows * inner)), dim3(256), 0, st, static_cast<T*>(dst), mask, static_cast<const T*>(value), \
                       scalar_as<T>(scalar, scalar_i64, scalar_is_int), rows, inner)
    switch (dtype) {
        case NNHIP_DT_F32: TI_MASKED(float); break;
        case NNHIP_DT_I32: TI_MASKED(int32_t); break;
        case NNHIP_DT_I64: TI_MASKED(int64_t); break;
        default: TI_MASKED(uint8_t); break;
    }
#undef TI_MASKED
    NNHIP_LAUNCH_CHECK("masked_assign_kernel");
    return 0;
}
