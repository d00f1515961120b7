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
#include <math.h>

#include "ew_map.h"

namespace nnhip {

constexpr int TO_MAXG = 6;      // axis groups after collapsing
constexpr int TO_MAXRANK = NNHIP_TENSOR_MAX_RANK;
constexpr int TO_NIN = 3;

struct TDims {
    int nd;
    int64_t ext[TO_MAXG];
    int64_t s[TO_NIN][TO_MAXG];
    int red[TO_MAXG];            // reduce flag per group (reductions only)
};

// -> 0, or -1 when more than TO_MAXG groups remain.  total = product of extents (0: nothing to do).
static int collapse(int rank, const int64_t* shape, const int64_t* const* strides, int nin, const int32_t* red, TDims& d, int64_t& total) {
    d = TDims{};
    total = 1;
    for (int i = 0; i < rank; ++i) total *= shape[i];
    if (total == 0) return 0;
    int64_t ext[TO_MAXRANK], s[TO_NIN][TO_MAXRANK];
    int rf[TO_MAXRANK], n = 0;
    for (int i = 0; i < rank; ++i) {
        if (shape[i] == 1) continue;
        const int f = red ? (red[i] != 0) : 0;
        bool merge = n > 0 && rf[n - 1] == f;
        for (int k = 0; k < nin && merge; ++k) merge = s[k][n - 1] == strides[k][i] * shape[i];
        if (merge) {
            ext[n - 1] *= shape[i];
            for (int k = 0; k < nin; ++k) s[k][n - 1] = strides[k][i];
        } else {
            ext[n] = shape[i];
            rf[n] = f;
            for (int k = 0; k < nin; ++k) s[k][n] = strides[k][i];
            ++n;
        }
    }
    if (n > TO_MAXG) return -1;
    if (n == 0) { ext[0] = 1; rf[0] = 0; for (int k = 0; k < nin; ++k) s[k][0] = 0; n = 1; }
    d.nd = n;
    for (int i = 0; i < n; ++i) {
        d.ext[i] = ext[i];
        d.red[i] = rf[i];
        for (int k = 0; k < nin; ++k) d.s[k][i] = s[k][i];
    }
    return 0;
}

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
// strided copy on (in, -, -)
struct CopyF { static constexpr bool U0 = true, U1 = false, U2 = false; __device__ float operator()(float x, float, float) const { return x; } };
struct CopyScaleF { float c; static constexpr bool U0 = true, U1 = false, U2 = false; __device__ float operator()(float x, float, float) const { return x * c; } };

struct SumC { __device__ static float id() { return 0.0f; } __device__ static float op(float a, float b) { return a + b; } };
struct MaxC { __device__ static float id() { return -INFINITY; } __device__ static float op(float a, float b) { return (a >= b || a != a) ? a : b; } };
struct MinC { __device__ static float id() { return INFINITY; } __device__ static float op(float a, float b) { return (a <= b || a != a) ? a : b; } };

// The tier the last launch of this file took and the segments it split a reduction into (nnhipTensorOpsLastTier): a test hook, so
// that a case aimed at a tier is known to have reached it.  Plain process-wide words, written by the launching host thread.
static int g_last_tier = NNHIP_TIER_NONE;
static int64_t g_last_segments = 0;
static void note_tier(int tier, int64_t segments = 1) { g_last_tier = tier; g_last_segments = segments; }

struct TIn { const float* p[TO_NIN]; float sv; };       // a NULL operand is the by-value scalar `sv`

template <class F>
__device__ __forceinline__ float to_apply(const F& f, const TIn& in, int64_t o0, int64_t o1, int64_t o2) {
    const float x0 = F::U0 ? (in.p[0] ? in.p[0][o0] : in.sv) : 0.0f;
    const float x1 = F::U1 ? (in.p[1] ? in.p[1][o1] : in.sv) : 0.0f;
    const float x2 = F::U2 ? (in.p[2] ? in.p[2][o2] : in.sv) : 0.0f;
    return f(x0, x1, x2);
}

// ---- elementwise kernels -------------------------------------------------------------------------------------------------------
// general: out contiguous over d.ext, one element per lane per iteration
template <class F>
__global__ __launch_bounds__(256) void ew_general_kernel(float* __restrict__ out, TIn in, TDims d, int64_t n, F f) {
    const int64_t gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += gsz) {
        int64_t rem = i, o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
        for (int g = TO_MAXG - 1; g >= 1; --g) {
            if (g < d.nd) {
                const int64_t q = rem / d.ext[g], c = rem - q * d.ext[g];
                o0 += c * d.s[0][g]; o1 += c * d.s[1][g]; o2 += c * d.s[2][g];
                rem = q;
            }
        }
        o0 += rem * d.s[0][0]; o1 += rem * d.s[1][0]; o2 += rem * d.s[2][0];
        out[i] = to_apply(f, in, o0, o1, o2);
    }
}
// vec2d: out [rows, cols] contiguous, cols % 4 == 0; operand k at p[k][row * rs[k] + col * cs[k]], cs[k] in {0, 1}; every address
// that is loaded as a float4 is 16-byte aligned (the host checks base pointers and row strides)
__device__ __forceinline__ float4 vec2d_load(const float* p, float sv, int64_t base, int64_t c4, int64_t cs) {
    if (!p) return make_float4(sv, sv, sv, sv);
    if (cs) return *reinterpret_cast<const float4*>(p + base + 4 * c4);
    const float v = p[base];
    return make_float4(v, v, v, v);
}
template <class F>
__global__ __launch_bounds__(256) void ew_vec2d_kernel(float* __restrict__ out, TIn in, int64_t rows, int64_t cols4, int64_t rs0, int64_t rs1,
                                                       int64_t rs2, int cs0, int cs1, int cs2, F f) {
    const int64_t n4 = rows * cols4, gsz = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += gsz) {
        const int64_t row = i / cols4, c4 = i - row * cols4;
        float4 x0 = make_float4(0, 0, 0, 0), x1 = x0, x2 = x0, y;
        if (F::U0) x0 = vec2d_load(in.p[0], in.sv, row * rs0, c4, cs0);
        if (F::U1) x1 = vec2d_load(in.p[1], in.sv, row * rs1, c4, cs1);
        if (F::U2) x2 = vec2d_load(in.p[2], in.sv, row * rs2, c4, cs2);
        y.x = f(x0.x, x1.x, x2.x); y.y = f(x0.y, x1.y, x2.y); y.z = f(x0.z, x1.z, x2.z); y.w = f(x0.w, x1.w, x2.w);
        reinterpret_cast<float4*>(out)[i] = y;
    }
}

static int grid_for(int64_t items) {
    int64_t b = ceil_div(items > 0 ? items : 1, 256);
    return (int)(b < 16384 ? b : 16384);
}

// out contiguous over d; picks vec2d when it applies, the general tier otherwise.  use[k]: whether F reads operand k.
template <class F>
static int launch_ew(float* out, const TIn& in, const TDims& d, int64_t n, F f, hipStream_t st, const char* nm) {
    const bool use[TO_NIN] = {F::U0, F::U1, F::U2};
    bool vec = d.nd <= 2 && aligned16(out) && d.ext[d.nd - 1] % 4 == 0;
    for (int k = 0; k < TO_NIN && vec; ++k) {
        if (!use[k] || !in.p[k]) continue;
        const int64_t cs = d.s[k][d.nd - 1], rs = d.nd == 2 ? d.s[k][0] : 0;
        vec = (cs == 0 || cs == 1) && aligned16(in.p[k]) && (cs == 0 || rs % 4 == 0);
    }
    if (vec) {
        const int64_t rows = d.nd == 2 ? d.ext[0] : 1, cols4 = d.ext[d.nd - 1] / 4;
        int64_t rs[TO_NIN];
        int cs[TO_NIN];
        for (int k = 0; k < TO_NIN; ++k) { rs[k] = d.nd == 2 ? d.s[k][0] : 0; cs[k] = (int)d.s[k][d.nd - 1]; }
        note_tier(NNHIP_TIER_EW_VEC2D);
        hipLaunchKernelGGL(ew_vec2d_kernel<F>, dim3(grid_for(rows * cols4)), dim3(256), 0, st, out, in, rows, cols4, rs[0], rs[1], rs[2],
                           cs[0], cs[1], cs[2], f);
    } else {
        note_tier(NNHIP_TIER_EW_GENERAL);
        hipLaunchKernelGGL(ew_general_kernel<F>, dim3(grid_for(n)), dim3(256), 0, st, out, in, d, n, f);
    }
    NNHIP_LAUNCH_CHECK(nm);
    return 0;
}

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

// ---- reductions ------------------------------------------------------------------------------------------------------------------
template <class C>
__device__ __forceinline__ float wave_red(float v) {
    v = C::op(v, dpp_f32<kDppXor1>(v));
    v = C::op(v, dpp_f32<kDppXor2>(v));
    v = C::op(v, dpp_f32<kDppHalfMirror>(v));
    v = C::op(v, dpp_f32<kDppMirror>(v));
    return C::op(C::op(readlane_f32(v, 0), readlane_f32(v, 16)), C::op(readlane_f32(v, 32), readlane_f32(v, 48)));
}
// 256 threads; `red` is 4 floats of LDS; every thread gets the result; waves merge in wave order
template <class C>
__device__ __forceinline__ float block_red(float v, float* red) {
    v = wave_red<C>(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return C::op(C::op(red[0], red[1]), C::op(red[2], red[3]));
}

// The structured view (Ko, R, Ki): element (ko, r, ki) of operand k at ko * so[k] + r * sr[k] + ki * si[k]; output / partial
// index = ko * Ki + ki.  S segments of `seg` reduced elements each.
struct RView {
    int64_t Ko, R, Ki, so[TO_NIN], sr[TO_NIN], si[TO_NIN];
    int64_t S, seg;
    float scale;                // applied to a finished sum (mean); var divides M2 by R
};
struct ROut { float* out; float* mean; float* part; };      // part: [2][Ko*Ki][S] when S > 1 (plane 1: the segment means of var)

template <class F>
__device__ __forceinline__ float rv_load(const F& f, const TIn& in, const RView& v, int64_t ko, int64_t r, int64_t ki) {
    return to_apply(f, in, ko * v.so[0] + r * v.sr[0] + ki * v.si[0], ko * v.so[1] + r * v.sr[1] + ki * v.si[1],
                    ko * v.so[2] + r * v.sr[2] + ki * v.si[2]);
}
template <bool VAR>
__device__ __forceinline__ void rv_store(const RView& v, const ROut& o, int64_t oi, int64_t seg, float acc, float mean) {
    if (v.S > 1) {
        o.part[oi * v.S + seg] = acc;
        if (VAR) o.part[v.Ko * v.Ki * v.S + oi * v.S + seg] = mean;
    } else if (VAR) {
        o.out[oi] = acc / (float)v.R;
        if (o.mean) o.mean[oi] = mean;
    } else {
        o.out[oi] = acc * v.scale;
    }
}

// row-wave: Ki == 1, R <= 1024, S == 1: wave w of block b owns row 4 b + w; lane l holds elements l, l + 64, ...
template <class F, class C, bool VAR>
__global__ __launch_bounds__(256) void red_row_wave_kernel(TIn in, RView v, ROut o, F f) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= v.Ko) return;                          // wave-uniform
    const int lane = threadIdx.x & 63;
    float x[16];
    float acc = C::id();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t r = lane + 64 * j;
        x[j] = r < v.R ? rv_load(f, in, v, row, r, 0) : C::id();
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc = C::op(acc, x[j]);
    acc = wave_red<C>(acc);
    float mean = 0.0f;
    if (VAR) {
        mean = acc / (float)v.R;
        float m2 = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float dlt = x[j] - mean;
            m2 += (lane + 64 * j) < v.R ? dlt * dlt : 0.0f;
        }
        acc = wave_red<SumC>(m2);
    }
    if (lane == 0) rv_store<VAR>(v, o, row, 0, acc, mean);
}
// row-block: Ki == 1: block = (row, segment)
template <class F, class C, bool VAR>
__global__ __launch_bounds__(256) void red_row_block_kernel(TIn in, RView v, ROut o, F f) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x / v.S, sg = blockIdx.x - row * v.S;
    const int64_t r0 = sg * v.seg, r1 = (r0 + v.seg < v.R) ? r0 + v.seg : v.R;
    float acc = C::id();
#pragma unroll 8
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) acc = C::op(acc, rv_load(f, in, v, row, r, 0));
    acc = block_red<C>(acc, red);
    float mean = 0.0f;
    if (VAR) {
        mean = acc / (float)(r1 - r0);
        float m2 = 0.0f;
        for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
            const float dlt = rv_load(f, in, v, row, r, 0) - mean;
            m2 += dlt * dlt;
        }
        acc = block_red<SumC>(m2, red);
    }
    if (threadIdx.x == 0) rv_store<VAR>(v, o, row, sg, acc, mean);
}
// col: lane -> ki = bx * 64 + lane; wave w takes r = r0 + w, r0 + w + 4, ...; block = ((ko * S + segment) * nbx + bx)
template <class F, class C, bool VAR>
__global__ __launch_bounds__(256) void red_col_kernel(TIn in, RView v, ROut o, int64_t nbx, F f) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t bx = blockIdx.x % nbx, t = blockIdx.x / nbx;
    const int64_t ko = t / v.S, sg = t - ko * v.S;
    const int64_t ki = bx * 64 + lane;
    const bool live = ki < v.Ki;
    const int64_t r0 = sg * v.seg, r1 = (r0 + v.seg < v.R) ? r0 + v.seg : v.R;
    float acc = C::id();
    if (live) {
#pragma unroll 8
        for (int64_t r = r0 + w; r < r1; r += 4) acc = C::op(acc, rv_load(f, in, v, ko, r, ki));
    }
    red[w][lane] = acc;
    __syncthreads();
    acc = C::op(C::op(red[0][lane], red[1][lane]), C::op(red[2][lane], red[3][lane]));
    float mean = 0.0f;
    if (VAR) {
        mean = acc / (float)(r1 - r0);
        float m2 = 0.0f;
        if (live)
            for (int64_t r = r0 + w; r < r1; r += 4) {
                const float dlt = rv_load(f, in, v, ko, r, ki) - mean;
                m2 += dlt * dlt;
            }
        __syncthreads();
        red[w][lane] = m2;
        __syncthreads();
        acc = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    }
    if (live && w == 0) rv_store<VAR>(v, o, ko * v.Ki + ki, sg, acc, mean);
}
// finishing pass: a lane per output merges its S partials in segment order (var: Chan's update of (count, mean, M2))
template <class C, bool VAR>
__global__ __launch_bounds__(256) void red_finish_kernel(RView v, ROut o) {
    const int64_t nout = v.Ko * v.Ki, oi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (oi >= nout) return;
    const float* p = o.part + oi * v.S;
    if (VAR) {
        const float* pm = o.part + nout * v.S + oi * v.S;
        float n = (float)(v.seg < v.R ? v.seg : v.R), mean = pm[0], m2 = p[0];
        for (int64_t s = 1; s < v.S; ++s) {
            const int64_t r0 = s * v.seg;
            const float nb = (float)((r0 + v.seg < v.R ? r0 + v.seg : v.R) - r0), tot = n + nb, dlt = pm[s] - mean;
            mean += dlt * (nb / tot);
            m2 += p[s] + dlt * dlt * (n * nb / tot);
            n = tot;
        }
        o.out[oi] = m2 / (float)v.R;
        if (o.mean) o.mean[oi] = mean;
    } else {
        float acc = p[0];
        for (int64_t s = 1; s < v.S; ++s) acc = C::op(acc, p[s]);
        o.out[oi] = acc * v.scale;
    }
}
// general: a 256-thread block per output; d holds all groups with their reduce flags; out contiguous over the kept groups.  Thread t
// takes the reduced elements t, t + 256, ... in the row-major order of the reduced groups (coalesced where the innermost reduced group
// is contiguous), each with up to five 64-bit divisions: for correctness, not speed
template <class F, class C, bool VAR>
__global__ __launch_bounds__(256) void red_general_kernel(TIn in, TDims d, RView v, ROut o, F f) {
    __shared__ float red[4];
    const int64_t oi = blockIdx.x / v.S, sg = blockIdx.x - oi * v.S;       // v: Ko = outputs, Ki = 1, R = reduced elements
    const int64_t r0 = sg * v.seg, r1 = (r0 + v.seg < v.R) ? r0 + v.seg : v.R;
    int64_t b0 = 0, b1 = 0, b2 = 0, rem = oi;
    for (int g = d.nd - 1; g >= 0; --g) {
        if (d.red[g]) continue;
        const int64_t q = rem / d.ext[g], c = rem - q * d.ext[g];
        b0 += c * d.s[0][g]; b1 += c * d.s[1][g]; b2 += c * d.s[2][g];
        rem = q;
    }
    float acc = C::id(), mean = 0.0f;
    for (int pass = 0; pass < (VAR ? 2 : 1); ++pass) {
        float a2 = pass ? 0.0f : C::id();
        for (int64_t ri = r0 + threadIdx.x; ri < r1; ri += 256) {
            int64_t o0 = b0, o1 = b1, o2 = b2, rr = ri;
            for (int g = d.nd - 1; g >= 0; --g) {
                if (!d.red[g]) continue;
                const int64_t q = rr / d.ext[g], c = rr - q * d.ext[g];
                o0 += c * d.s[0][g]; o1 += c * d.s[1][g]; o2 += c * d.s[2][g];
                rr = q;
            }
            const float x = to_apply(f, in, o0, o1, o2);
            if (pass) { const float dlt = x - mean; a2 += dlt * dlt; }
            else a2 = C::op(a2, x);
        }
        if (pass) acc = block_red<SumC>(a2, red);
        else acc = block_red<C>(a2, red);
        if (VAR && pass == 0) mean = acc / (float)(r1 - r0);
    }
    if (threadIdx.x == 0) rv_store<VAR>(v, o, oi, sg, acc, mean);
}

// Tier boundaries (tests/tape_ref.py restates them as route())
constexpr int64_t RED_WAVE_MAX_R = 1024;        // a row of 16 registers per lane
constexpr int64_t RED_FILL_BLOCKS = 512;        // below this many blocks the reduced extent is split (256 CUs, two blocks each)
constexpr int64_t RED_ROW_SPLIT_MIN_R = 8192, RED_ROW_SEG = 4096;
constexpr int64_t RED_COL_SPLIT_MIN_R = 256, RED_COL_SEG = 64;
constexpr int64_t RED_GEN_SPLIT_MIN_R = 4096, RED_GEN_SEG = 2048;
constexpr int64_t RED_MAX_S = 256;

// d: collapsed groups with reduce flags and the operands' strides.  out: contiguous over the kept groups.
template <class F, class C, bool VAR>
static int launch_reduce(const TIn& in, const TDims& d, float* out, float* mean_out, float scale, F f, hipStream_t st, const char* nm) {
    int64_t nout = 1, nred = 1;
    for (int g = 0; g < d.nd; ++g) (d.red[g] ? nred : nout) *= d.ext[g];
    // the structured view: [R] [K,R] [R,K] [K,R,K]
    int gk0 = -1, gr = -1, gk1 = -1;
    bool structured = true;
    if (d.nd == 1) { if (d.red[0]) gr = 0; else gk1 = 0; }
    else if (d.nd == 2 && !d.red[0] && d.red[1]) { gk0 = 0; gr = 1; }
    else if (d.nd == 2 && d.red[0] && !d.red[1]) { gr = 0; gk1 = 1; }
    else if (d.nd == 3 && !d.red[0] && d.red[1] && !d.red[2]) { gk0 = 0; gr = 1; gk1 = 2; }
    else structured = false;
    if (!structured) {
        RView v{};
        v.Ko = nout; v.R = nred; v.Ki = 1; v.scale = scale; v.S = 1; v.seg = nred;
        if (nout < RED_FILL_BLOCKS && nred >= RED_GEN_SPLIT_MIN_R) {
            int64_t S = ceil_div(nred, RED_GEN_SEG), cap = ceil_div(2 * RED_FILL_BLOCKS, nout);
            S = S < cap ? S : cap; S = S < RED_MAX_S ? S : RED_MAX_S;
            v.seg = ceil_div(nred, S); v.S = ceil_div(nred, v.seg);
        }
        NNHIP_CHECK_ARG(nout * v.S < ((int64_t)1 << 31), NNHIP_EINVAL, "%s: too many blocks", nm);
        ROut o{out, mean_out, nullptr};
        if (v.S > 1) {
            o.part = static_cast<float*>(workspace((size_t)2 * nout * v.S * sizeof(float)));
            NNHIP_CHECK_ARG(o.part != nullptr, NNHIP_ENOMEM, "%s: workspace allocation failed", nm);
        }
        note_tier(NNHIP_TIER_RED_GENERAL, v.S);
        hipLaunchKernelGGL((red_general_kernel<F, C, VAR>), dim3((unsigned)(nout * v.S)), dim3(256), 0, st, in, d, v, o, f);
        NNHIP_LAUNCH_CHECK(nm);
        if (v.S > 1) {
            hipLaunchKernelGGL((red_finish_kernel<C, VAR>), dim3((unsigned)ceil_div(nout, 256)), dim3(256), 0, st, v, o);
            NNHIP_LAUNCH_CHECK(nm);
        }
        return 0;
    }
    RView v{};
    v.Ko = gk0 >= 0 ? d.ext[gk0] : 1; v.R = gr >= 0 ? d.ext[gr] : 1; v.Ki = gk1 >= 0 ? d.ext[gk1] : 1;
    for (int k = 0; k < TO_NIN; ++k) {
        v.so[k] = gk0 >= 0 ? d.s[k][gk0] : 0; v.sr[k] = gr >= 0 ? d.s[k][gr] : 0; v.si[k] = gk1 >= 0 ? d.s[k][gk1] : 0;
    }
    v.scale = scale;
    v.S = 1; v.seg = v.R;
    ROut o{out, mean_out, nullptr};
    const bool row = v.Ki == 1;
    int64_t nbx = 1;
    if (row) {
        if (v.R > RED_WAVE_MAX_R && v.Ko < RED_FILL_BLOCKS && v.R >= RED_ROW_SPLIT_MIN_R) {
            int64_t S = ceil_div(v.R, RED_ROW_SEG), cap = ceil_div(2 * RED_FILL_BLOCKS, v.Ko);
            S = S < cap ? S : cap; S = S < RED_MAX_S ? S : RED_MAX_S;
            v.seg = ceil_div(v.R, S); v.S = ceil_div(v.R, v.seg);
        }
    } else {
        nbx = ceil_div(v.Ki, 64);
        if (v.Ko * nbx < RED_FILL_BLOCKS && v.R >= RED_COL_SPLIT_MIN_R) {
            int64_t S = ceil_div(v.R, RED_COL_SEG), cap = ceil_div(2 * RED_FILL_BLOCKS, v.Ko * nbx);
            S = S < cap ? S : cap; S = S < RED_MAX_S ? S : RED_MAX_S;
            v.seg = ceil_div(v.R, S); v.S = ceil_div(v.R, v.seg);
        }
    }
    NNHIP_CHECK_ARG(v.Ko * v.S * nbx < ((int64_t)1 << 31) && nout < ((int64_t)1 << 38), NNHIP_EINVAL, "%s: too many blocks", nm);
    if (v.S > 1) {
        o.part = static_cast<float*>(workspace((size_t)2 * nout * v.S * sizeof(float)));
        NNHIP_CHECK_ARG(o.part != nullptr, NNHIP_ENOMEM, "%s: workspace allocation failed", nm);
    }
    note_tier(row ? (v.R <= RED_WAVE_MAX_R ? NNHIP_TIER_RED_ROW_WAVE : NNHIP_TIER_RED_ROW_BLOCK) : NNHIP_TIER_RED_COL, v.S);
    if (row && v.R <= RED_WAVE_MAX_R)
        hipLaunchKernelGGL((red_row_wave_kernel<F, C, VAR>), dim3((unsigned)ceil_div(v.Ko, 4)), dim3(256), 0, st, in, v, o, f);
    else if (row)
        hipLaunchKernelGGL((red_row_block_kernel<F, C, VAR>), dim3((unsigned)(v.Ko * v.S)), dim3(256), 0, st, in, v, o, f);
    else
        hipLaunchKernelGGL((red_col_kernel<F, C, VAR>), dim3((unsigned)(v.Ko * v.S * nbx)), dim3(256), 0, st, in, v, o, nbx, f);
    NNHIP_LAUNCH_CHECK(nm);
    if (v.S > 1) {
        hipLaunchKernelGGL((red_finish_kernel<C, VAR>), dim3((unsigned)ceil_div(nout, 256)), dim3(256), 0, st, v, o);
        NNHIP_LAUNCH_CHECK(nm);
    }
    return 0;
}

static int check_dims(const char* fn, int rank, const int64_t* shape) {
    NNHIP_CHECK_ARG(rank >= 0 && rank <= TO_MAXRANK, NNHIP_EINVAL, "%s: rank %d is outside 0..%d", fn, rank, TO_MAXRANK);
    NNHIP_CHECK_ARG(rank == 0 || shape != nullptr, NNHIP_EINVAL, "%s: null shape", fn);
    for (int i = 0; i < rank; ++i) NNHIP_CHECK_ARG(shape[i] >= 0, NNHIP_EINVAL, "%s: negative extent", fn);
    return 0;
}
#define TO_CHECK_DIMS(fn, rank, shape) do { const int _rc = check_dims(fn, rank, shape); if (_rc) return _rc; } while (0)
#define TO_PTR(fn, p)                                                          \
    do {                                                                       \
        NNHIP_CHECK_ARG((p) != nullptr, NNHIP_EINVAL, fn ": null pointer");     \
        NNHIP_CHECK_ARG(aligned4(p), NNHIP_EALIGN, fn ": misaligned pointer");  \
    } while (0)

static bool is_full(const TDims& d, int k) {         // operand k walks the collapsed shape contiguously
    int64_t want = 1;
    for (int g = d.nd - 1; g >= 0; --g) {
        if (d.s[k][g] != want) return false;
        want *= d.ext[g];
    }
    return true;
}
static bool is_scalar(const TDims& d, int k) {
    for (int g = 0; g < d.nd; ++g) if (d.s[k][g] != 0) return false;
    return true;
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
