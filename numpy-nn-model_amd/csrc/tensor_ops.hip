// tensor_ops.hip -- the arithmetic core of the Tensor tape (ABI 223): broadcasting binary ops, axis reductions, strided copy.
//
// Shapes and strides reach every kernel BY VALUE in a small struct (at most 6 collapsed axis groups): no device upload, so every
// entry is legal inside a stream capture.  The entries take up to 8 raw axes; collapse() drops axes of extent 1 and merges adjacent
// axes that every operand walks contiguously (and that share a reduce flag) before a tier is picked.
//
// Elementwise tiers (forward of a binary op, the gradient of an operand that was not broadcast, the backward of a reduction, the copy):
//   same     same shape, both contiguous: the float4 map2 skeleton of ew_map.h (nnhipAdd's kernel for `add`, same bits)
//   scalar   one operand a Python scalar by value or a one-element device tensor read ON the device: the map1 skeleton
//   vec2d    at most two groups, every operand's innermost stride 0 or 1 (bias rows [N,F] o [F], keepdims columns [N,F] o [N,1]),
//            all 16-byte aligned: float4 along the innermost group, a stride-0 operand is one scalar load per float4
//   general  up to 6 groups, stride 0 on broadcast axes, 64-bit offsets, one element per lane and up to five 64-bit divisions per
//            element: for correctness, not speed
// Reduction tiers, one kernel family templated on (load functor, combine); the load functor is the identity for sum / mean / var /
// max / min and the LOCAL GRADIENT (dOut, dOut*b, -dOut*a/b^2, dOut*(a>=b), ...) for the gradient of a broadcast operand, whose
// full-shape gradient is therefore never written to memory:
//   row-wave   [K,R] or [R], R <= 1024: a wave per row, the row in the wave's registers (16 per lane)
//   row-block  [K,R] or [R]: a 256-thread block per (row, segment); R is split into S segments when K alone cannot fill the chip
//   col        [R,K] or [K,R,K]: lanes along the innermost kept group (coalesced), the block's four waves stride over R and merge
//              through LDS; R is split into S segments when the kept extent is small
//   general    anything else ([R,K,R] and deeper): a block per (output, segment), the reduced elements strided over its threads with a
//              full index decomposition each -- correctness only
// S > 1 leaves partials in the library's grow-only workspace and a finishing kernel merges them in segment order: two launches at
// most, no float atomics, the order of every combine is fixed by (shape, tier), so reruns are bit-identical.
// var is two sweeps over a block's segment (sum -> mean, then sum of (x - mean)^2: from registers in row-wave, a re-read otherwise);
// split segments leave (mean, M2) and the finishing kernel merges them with Chan's update.  Never E[x^2] - E[x]^2.
#include "tensor_ops.h"

namespace nnhip {

// ---- functors ----------------------------------------------------------------------------------------------------------------
// forward: out = op(a, b), one rounding per operation; maximum / minimum propagate a NaN from either side as NumPy does
struct BAdd { __device__ static float f(float a, float b) { return a + b; } };
struct BSub { __device__ static float f(float a, float b) { return a - b; } };
struct BMul { __device__ static float f(float a, float b) { return a * b; } };
struct BDiv { __device__ static float f(float a, float b) { return a / b; } };
struct BPow { __device__ static float f(float a, float b) { return powf(a, b); } };
struct BMax { __device__ static float f(float a, float b) { return (a >= b || a != a) ? a : b; } };
struct BMin { __device__ static float f(float a, float b) { return (a <= b || a != a) ? a : b; } };
template <class Op> struct Fwd2 {            // inputs (a, b, -)
    static constexpr bool U0 = true, U1 = true, U2 = false;
    __device__ float operator()(float a, float b, float) const { return Op::f(a, b); }
};
template <class Op> struct Map2F { __device__ float operator()(float a, float b) const { return Op::f(a, b); } };
// scalar tiers: the scalar is operand b (SIDE 1) or operand a (SIDE 0)
template <class Op, int SIDE> struct Map1S {
    float s;
    __device__ float operator()(float x) const { return SIDE ? Op::f(x, s) : Op::f(s, x); }
};
// local gradients on (g, a, b): the reference's expressions (neunet/autograd.py:110-186, 328-332, 456-484), NaN / inf included
struct GId  { static constexpr bool U0 = true, U1 = false, U2 = false; __device__ float operator()(float g, float, float) const { return g; } };
struct GNeg { static constexpr bool U0 = true, U1 = false, U2 = false; __device__ float operator()(float g, float, float) const { return -g; } };
struct GMulB { static constexpr bool U0 = true, U1 = false, U2 = true; __device__ float operator()(float g, float, float b) const { return g * b; } };
struct GMulA { static constexpr bool U0 = true, U1 = true, U2 = false; __device__ float operator()(float g, float a, float) const { return a * g; } };
struct GDivA { static constexpr bool U0 = true, U1 = false, U2 = true; __device__ float operator()(float g, float, float b) const { return g / b; } };
struct GDivB { static constexpr bool U0 = true, U1 = true, U2 = true; __device__ float operator()(float g, float a, float b) const { return (-g * a) / (b * b); } };
struct GPowA { static constexpr bool U0 = true, U1 = true, U2 = true; __device__ float operator()(float g, float a, float b) const { return (g * b) * powf(a, b - 1.0f); } };
struct GPowB { static constexpr bool U0 = true, U1 = true, U2 = true; __device__ float operator()(float g, float a, float b) const { return (g * powf(a, b)) * logf(a); } };
struct GGe { static constexpr bool U0 = true, U1 = true, U2 = true; __device__ float operator()(float g, float a, float b) const { return g * (a >= b ? 1.0f : 0.0f); } };
struct GLe { static constexpr bool U0 = true, U1 = true, U2 = true; __device__ float operator()(float g, float a, float b) const { return g * (a <= b ? 1.0f : 0.0f); } };
// backward of a reduction on (x, saved, grad): saved and grad are broadcast over the reduced axes
struct RScale { float c; static constexpr bool U0 = false, U1 = false, U2 = true; __device__ float operator()(float, float, float g) const { return g * c; } };
struct RVar { float c; static constexpr bool U0 = true, U1 = true, U2 = true; __device__ float operator()(float x, float m, float g) const { return g * 2.0f * (x - m) * c; } };
struct REq { static constexpr bool U0 = true, U1 = true, U2 = true; __device__ float operator()(float x, float m, float g) const { return g * (x == m ? 1.0f : 0.0f); } };

int g_last_tier = NNHIP_TIER_NONE;      // tensor_ops.h: note_tier
int64_t g_last_segments = 0;

// ---- 2-D transpose through LDS: out [B, R, C] contiguous, in element (b, r, c) at b * sb + r + c * sc ---------------------------------
__global__ __launch_bounds__(256) void transpose_tile_kernel(float* __restrict__ out, const float* __restrict__ in, int64_t R, int64_t C,
                                                             int64_t sb, int64_t sc, int64_t tiles_r, int64_t tiles_c, float scale) {
    __shared__ float tile[32][33];
    const int64_t t = blockIdx.x;
    const int64_t b = t / (tiles_r * tiles_c), tr = (t / tiles_c) % tiles_r, tc = t % tiles_c;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = tr * 32, c0 = tc * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + ty + 8 * j, r = r0 + tx;
        if (c < C && r < R) tile[ty + 8 * j][tx] = in[b * sb + r + c * sc];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + ty + 8 * j, c = c0 + tx;
        if (r < R && c < C) out[(b * R + r) * C + c] = tile[tx][ty + 8 * j] * scale;
    }
}

template <class Op>
static int binary_forward(float* out, const float* a, const float* b, float scalar, const TDims& d, int64_t n, hipStream_t st) {
    const bool fa = a && (is_full(d, 0) || n == 1), fb = b && (is_full(d, 1) || n == 1);
    if (fa && fb) { note_tier(NNHIP_TIER_EW_SAME); return launch_map2(out, a, b, n, Map2F<Op>{}, st, "binary_same"); }
    if (fa && (!b || is_scalar(d, 1))) { note_tier(NNHIP_TIER_EW_SCALAR); return launch_map1s(out, a, n, Map1S<Op, 1>{scalar}, b, st, "binary_scalar"); }
    if (fb && (!a || is_scalar(d, 0))) { note_tier(NNHIP_TIER_EW_SCALAR); return launch_map1s(out, b, n, Map1S<Op, 0>{scalar}, a, st, "binary_scalar"); }
    TIn in{{a, b, nullptr}, scalar};
    return launch_ew(out, in, d, n, Fwd2<Op>{}, st, "binary_broadcast");
}
// `add` on the same-shape tier is nnhipAdd's own instantiation (map2_kernel<AddF>)
template <>
int binary_forward<BAdd>(float* out, const float* a, const float* b, float scalar, const TDims& d, int64_t n, hipStream_t st) {
    const bool fa = a && (is_full(d, 0) || n == 1), fb = b && (is_full(d, 1) || n == 1);
    if (fa && fb) { note_tier(NNHIP_TIER_EW_SAME); return launch_map2(out, a, b, n, AddF{}, st, "binary_same"); }
    if (fa && (!b || is_scalar(d, 1))) { note_tier(NNHIP_TIER_EW_SCALAR); return launch_map1s(out, a, n, Map1S<BAdd, 1>{scalar}, b, st, "binary_scalar"); }
    if (fb && (!a || is_scalar(d, 0))) { note_tier(NNHIP_TIER_EW_SCALAR); return launch_map1s(out, b, n, Map1S<BAdd, 0>{scalar}, a, st, "binary_scalar"); }
    TIn in{{a, b, nullptr}, scalar};
    return launch_ew(out, in, d, n, Fwd2<BAdd>{}, st, "binary_broadcast");
}

// gradient of operand `which` (0: a, 1: b): one elementwise pass when it was not broadcast, one reduction otherwise
template <class G>
static int binary_grad(float* dst, int which, const TIn& in, const int64_t* shape, const int64_t* const* strides, int rank, hipStream_t st) {
    int32_t red[TO_MAXRANK];
    bool any = false;
    for (int i = 0; i < rank; ++i) { red[i] = shape[i] > 1 && strides[which + 1][i] == 0; any = any || red[i]; }
    TDims d;
    int64_t n;
    if (collapse(rank, shape, strides, 3, any ? red : nullptr, d, n) != 0) { set_last_error("nnhipBroadcastBinaryBackward: more than %d axis groups", TO_MAXG); return NNHIP_EINVAL; }
    if (!any) return launch_ew(dst, in, d, n, G{}, st, "binary_backward");
    return launch_reduce<G, SumC, false>(in, d, dst, nullptr, 1.0f, G{}, st, "binary_backward_reduce");
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipTensorOpsLastTier(int64_t* segments) {
    if (segments) *segments = g_last_segments;
    return g_last_tier;
}

extern "C" int nnhipBroadcastBinaryForward(int kind, float* out, const float* a, const float* b, float scalar, int rank, const int64_t* shape,
                                           const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t s) {
    NNHIP_CHECK_ARG(kind >= NNHIP_BIN_ADD && kind <= NNHIP_BIN_MIN, NNHIP_EINVAL, "nnhipBroadcastBinaryForward: unknown kind %d", kind);
    TO_CHECK_DIMS("nnhipBroadcastBinaryForward", rank, shape);
    NNHIP_CHECK_ARG(a != nullptr || b != nullptr, NNHIP_EINVAL, "nnhipBroadcastBinaryForward: null pointer (both operands)");
    NNHIP_CHECK_ARG(rank == 0 || ((stride_a || !a) && (stride_b || !b)), NNHIP_EINVAL, "nnhipBroadcastBinaryForward: null strides");
    int64_t zeros[TO_MAXRANK] = {0};
    const int64_t* strides[2] = {a ? stride_a : zeros, b ? stride_b : zeros};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 2, nullptr, d, n) == 0, NNHIP_EINVAL, "nnhipBroadcastBinaryForward: more than %d axis groups", TO_MAXG);
    if (n == 0) return 0;
    TO_PTR("nnhipBroadcastBinaryForward", out);
    if (a) TO_PTR("nnhipBroadcastBinaryForward", a);
    if (b) TO_PTR("nnhipBroadcastBinaryForward", b);
    hipStream_t st = (hipStream_t)s;
    switch (kind) {
        case NNHIP_BIN_ADD: return binary_forward<BAdd>(out, a, b, scalar, d, n, st);
        case NNHIP_BIN_SUB: return binary_forward<BSub>(out, a, b, scalar, d, n, st);
        case NNHIP_BIN_MUL: return binary_forward<BMul>(out, a, b, scalar, d, n, st);
        case NNHIP_BIN_DIV: return binary_forward<BDiv>(out, a, b, scalar, d, n, st);
        case NNHIP_BIN_POW: return binary_forward<BPow>(out, a, b, scalar, d, n, st);
        case NNHIP_BIN_MAX: return binary_forward<BMax>(out, a, b, scalar, d, n, st);
        default: return binary_forward<BMin>(out, a, b, scalar, d, n, st);
    }
}

extern "C" int nnhipBroadcastBinaryBackward(int kind, float* dA, float* dB, const float* dOut, const float* a, const float* b, float scalar,
                                            int rank, const int64_t* shape, const int64_t* stride_a, const int64_t* stride_b, nnhipStream_t s) {
    NNHIP_CHECK_ARG(kind >= NNHIP_BIN_ADD && kind <= NNHIP_BIN_MIN, NNHIP_EINVAL, "nnhipBroadcastBinaryBackward: unknown kind %d", kind);
    TO_CHECK_DIMS("nnhipBroadcastBinaryBackward", rank, shape);
    NNHIP_CHECK_ARG(a != nullptr || b != nullptr, NNHIP_EINVAL, "nnhipBroadcastBinaryBackward: null pointer (both operands)");
    NNHIP_CHECK_ARG((a || !dA) && (b || !dB), NNHIP_EINVAL, "nnhipBroadcastBinaryBackward: a by-value scalar has no gradient");
    NNHIP_CHECK_ARG(rank == 0 || ((stride_a || !a) && (stride_b || !b)), NNHIP_EINVAL, "nnhipBroadcastBinaryBackward: null strides");
    int64_t total = 1;
    for (int i = 0; i < rank; ++i) total *= shape[i];
    if (total == 0 || (!dA && !dB)) return 0;
    TO_PTR("nnhipBroadcastBinaryBackward", dOut);
    if (a) TO_PTR("nnhipBroadcastBinaryBackward", a);
    if (b) TO_PTR("nnhipBroadcastBinaryBackward", b);
    if (dA) TO_PTR("nnhipBroadcastBinaryBackward", dA);
    if (dB) TO_PTR("nnhipBroadcastBinaryBackward", dB);
    int64_t zeros[TO_MAXRANK] = {0}, full[TO_MAXRANK];
    int64_t acc = 1;
    for (int i = rank - 1; i >= 0; --i) { full[i] = acc; acc *= shape[i]; }
    const int64_t* strides[3] = {full, a ? stride_a : zeros, b ? stride_b : zeros};
    TIn in{{dOut, a, b}, scalar};
    hipStream_t st = (hipStream_t)s;
    int rc = 0;
#define TO_GRAD(GA, GB)                                                                        \
    do {                                                                                       \
        if (dA) rc = binary_grad<GA>(dA, 0, in, shape, strides, rank, st);                     \
        if (rc == 0 && dB) rc = binary_grad<GB>(dB, 1, in, shape, strides, rank, st);          \
    } while (0)
    switch (kind) {
        case NNHIP_BIN_ADD: TO_GRAD(GId, GId); break;
        case NNHIP_BIN_SUB: TO_GRAD(GId, GNeg); break;
        case NNHIP_BIN_MUL: TO_GRAD(GMulB, GMulA); break;
        case NNHIP_BIN_DIV: TO_GRAD(GDivA, GDivB); break;
        case NNHIP_BIN_POW: TO_GRAD(GPowA, GPowB); break;
        case NNHIP_BIN_MAX: TO_GRAD(GGe, GLe); break;
        default: TO_GRAD(GLe, GGe); break;
    }
#undef TO_GRAD
    return rc;
}

extern "C" int nnhipReduceAxesForward(int kind, float* out, float* mean_out, const float* in, int rank, const int64_t* shape,
                                      const int64_t* stride, const int32_t* reduce, nnhipStream_t s) {
    NNHIP_CHECK_ARG(kind >= NNHIP_RED_SUM && kind <= NNHIP_RED_MIN, NNHIP_EINVAL, "nnhipReduceAxesForward: unknown kind %d", kind);
    TO_CHECK_DIMS("nnhipReduceAxesForward", rank, shape);
    NNHIP_CHECK_ARG(rank == 0 || (stride && reduce), NNHIP_EINVAL, "nnhipReduceAxesForward: null strides or reduce flags");
    int64_t nred = 1, nout = 1;
    for (int i = 0; i < rank; ++i) (reduce[i] ? nred : nout) *= shape[i];
    if (nout == 0) return 0;
    NNHIP_CHECK_ARG(nred > 0, NNHIP_EINVAL, "nnhipReduceAxesForward: a reduction over zero elements");
    TO_PTR("nnhipReduceAxesForward", out);
    TO_PTR("nnhipReduceAxesForward", in);
    const int64_t* strides[1] = {stride};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 1, reduce, d, n) == 0, NNHIP_EINVAL, "nnhipReduceAxesForward: more than %d axis groups", TO_MAXG);
    TIn ti{{in, nullptr, nullptr}, 0.0f};
    hipStream_t st = (hipStream_t)s;
    switch (kind) {
        case NNHIP_RED_SUM: return launch_reduce<GId, SumC, false>(ti, d, out, nullptr, 1.0f, GId{}, st, "reduce_sum");
        case NNHIP_RED_MEAN: return launch_reduce<GId, SumC, false>(ti, d, out, nullptr, 1.0f / (float)nred, GId{}, st, "reduce_mean");
        case NNHIP_RED_VAR: return launch_reduce<GId, SumC, true>(ti, d, out, mean_out, 1.0f, GId{}, st, "reduce_var");
        case NNHIP_RED_MAX: return launch_reduce<GId, MaxC, false>(ti, d, out, nullptr, 1.0f, GId{}, st, "reduce_max");
        default: return launch_reduce<GId, MinC, false>(ti, d, out, nullptr, 1.0f, GId{}, st, "reduce_min");
    }
}

extern "C" int nnhipReduceAxesBackward(int kind, float* dX, const float* grad, const float* x, const float* saved, int rank,
                                       const int64_t* shape, const int32_t* reduce, nnhipStream_t s) {
    NNHIP_CHECK_ARG(kind >= NNHIP_RED_SUM && kind <= NNHIP_RED_MIN, NNHIP_EINVAL, "nnhipReduceAxesBackward: unknown kind %d", kind);
    TO_CHECK_DIMS("nnhipReduceAxesBackward", rank, shape);
    NNHIP_CHECK_ARG(rank == 0 || reduce, NNHIP_EINVAL, "nnhipReduceAxesBackward: null reduce flags");
    int64_t nred = 1, total = 1;
    for (int i = 0; i < rank; ++i) { total *= shape[i]; if (reduce[i]) nred *= shape[i]; }
    if (total == 0) return 0;
    TO_PTR("nnhipReduceAxesBackward", dX);
    TO_PTR("nnhipReduceAxesBackward", grad);
    const bool needs_x = kind >= NNHIP_RED_VAR;
    if (needs_x) { TO_PTR("nnhipReduceAxesBackward", x); TO_PTR("nnhipReduceAxesBackward", saved); }
    int64_t full[TO_MAXRANK], kept[TO_MAXRANK];
    int64_t acc = 1, kacc = 1;
    for (int i = rank - 1; i >= 0; --i) {
        full[i] = acc; acc *= shape[i];
        kept[i] = reduce[i] ? 0 : kacc;
        if (!reduce[i]) kacc *= shape[i];
    }
    const int64_t* strides[3] = {full, kept, kept};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 3, nullptr, d, n) == 0, NNHIP_EINVAL, "nnhipReduceAxesBackward: more than %d axis groups", TO_MAXG);
    TIn in{{needs_x ? x : grad, needs_x ? saved : grad, grad}, 0.0f};
    hipStream_t st = (hipStream_t)s;
    switch (kind) {
        case NNHIP_RED_SUM: return launch_ew(dX, in, d, n, RScale{1.0f}, st, "reduce_sum_backward");
        case NNHIP_RED_MEAN: return launch_ew(dX, in, d, n, RScale{1.0f / (float)nred}, st, "reduce_mean_backward");
        case NNHIP_RED_VAR: return launch_ew(dX, in, d, n, RVar{1.0f / (float)nred}, st, "reduce_var_backward");
        default: return launch_ew(dX, in, d, n, REq{}, st, "reduce_maxmin_backward");
    }
}

extern "C" int nnhipStridedCopy(float* out, const float* in, float scale, int rank, const int64_t* shape, const int64_t* stride_in,
                                nnhipStream_t s) {
    TO_CHECK_DIMS("nnhipStridedCopy", rank, shape);
    NNHIP_CHECK_ARG(rank == 0 || stride_in, NNHIP_EINVAL, "nnhipStridedCopy: null strides");
    const int64_t* strides[1] = {stride_in};
    TDims d;
    int64_t n;
    NNHIP_CHECK_ARG(collapse(rank, shape, strides, 1, nullptr, d, n) == 0, NNHIP_EINVAL, "nnhipStridedCopy: more than %d axis groups", TO_MAXG);
    if (n == 0) return 0;
    TO_PTR("nnhipStridedCopy", out);
    TO_PTR("nnhipStridedCopy", in);
    hipStream_t st = (hipStream_t)s;
    // the 2-D-transpose pattern: `in` is contiguous along the second-to-last group of `out`
    if ((d.nd == 2 || d.nd == 3) && d.s[0][d.nd - 2] == 1 && d.s[0][d.nd - 1] != 1) {
        const int64_t B = d.nd == 3 ? d.ext[0] : 1, R = d.ext[d.nd - 2], C = d.ext[d.nd - 1];
        const int64_t tr = ceil_div(R, 32), tc = ceil_div(C, 32);
        NNHIP_CHECK_ARG(B * tr * tc < ((int64_t)1 << 31), NNHIP_EINVAL, "nnhipStridedCopy: too many tiles");
        note_tier(NNHIP_TIER_COPY_TILE);
        hipLaunchKernelGGL(transpose_tile_kernel, dim3((unsigned)(B * tr * tc)), dim3(256), 0, st, out, in, R, C, d.nd == 3 ? d.s[0][0] : 0,
                           d.s[0][d.nd - 1], tr, tc, scale);
        NNHIP_LAUNCH_CHECK("transpose_tile_kernel");
        return 0;
    }
    TIn ti{{in, nullptr, nullptr}, 0.0f};
    if (scale == 1.0f) return launch_ew(out, ti, d, n, CopyF{}, st, "strided_copy");
    return launch_ew(out, ti, d, n, CopyScaleF{scale}, st, "strided_copy");
}
