// tensor_ops.h -- what the Tensor-tape sources share: the by-value shape description (TDims, collapse), the operand pack (TIn), the
// elementwise launcher (launch_ew: vec2d / general), the reduction kernels with their launcher (launch_reduce: the load functor is
// a template argument) and the tier hook (note_tier).  tensor_ops.hip (arithmetic, reductions, copy) and tensor_index.hip
// (comparisons, where, indexing) instantiate these templates with their own functors; one definition, so a tier is the same code
// in both.  tensor_ops.hip describes the tiers.
#pragma once
#include <math.h>

#include <type_traits>

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

// strided copy on (in, -, -)
struct CopyF { static constexpr bool U0 = true, U1 = false, U2 = false; __device__ float operator()(float x, float, float) const { return x; } };
struct CopyScaleF { float c; static constexpr bool U0 = true, U1 = false, U2 = false; __device__ float operator()(float x, float, float) const { return x * c; } };

struct SumC { __device__ static float id() { return 0.0f; } __device__ static float op(float a, float b) { return a + b; } };
struct MaxC { __device__ static float id() { return -INFINITY; } __device__ static float op(float a, float b) { return (a >= b || a != a) ? a : b; } };
struct MinC { __device__ static float id() { return INFINITY; } __device__ static float op(float a, float b) { return (a <= b || a != a) ? a : b; } };

// The tier the last launch of the tape sources took and the segments it split a reduction into (nnhipTensorOpsLastTier): a test
// hook, so that a case aimed at a tier is known to have reached it.  Plain process-wide words (defined in tensor_ops.hip),
// written by the launching host thread.
extern int g_last_tier;
extern int64_t g_last_segments;
inline void note_tier(int tier, int64_t segments = 1) { g_last_tier = tier; g_last_segments = segments; }

struct TIn { const float* p[TO_NIN]; float sv; };       // a NULL operand is the by-value scalar `sv`

// Operand 1 of a functor that declares `static constexpr bool BYTE1 = true` is a BYTE array behind the float pointer (a bool mask:
// tensor_index.hip's where-gradients); it is read as 0.0f / 1.0f and keeps such a functor off the float4 tier.
template <class F, class = void> struct byte_op1 { static constexpr bool value = false; };
template <class F> struct byte_op1<F, std::enable_if_t<F::BYTE1>> { static constexpr bool value = true; };
template <class F>
__device__ __forceinline__ float ld_op1(const float* p, int64_t o) {
    if constexpr (byte_op1<F>::value) return reinterpret_cast<const uint8_t*>(p)[o] ? 1.0f : 0.0f;
    else return p[o];
}

template <class F>
__device__ __forceinline__ float to_apply(const F& f, const TIn& in, int64_t o0, int64_t o1, int64_t o2) {
    const float x0 = F::U0 ? (in.p[0] ? in.p[0][o0] : in.sv) : 0.0f;
    const float x1 = F::U1 ? (in.p[1] ? ld_op1<F>(in.p[1], o1) : in.sv) : 0.0f;
    const float x2 = F::U2 ? (in.p[2] ? in.p[2][o2] : in.sv) : 0.0f;
    return f(x0, x1, x2);
}

// linear index over the collapsed groups -> the three operands' element offsets (up to five 64-bit divisions): the typed general
// kernels of tensor_index.hip.  ew_general_kernel below keeps the same walk written out: routed through this helper the compiler
// schedules it differently (another instruction stream for every instance of tensor_ops.hip), and that code is to stay as it is.
__device__ __forceinline__ void to_offsets(const TDims& d, int64_t i, int64_t& o0, int64_t& o1, int64_t& o2) {
    int64_t rem = i;
    o0 = 0; o1 = 0; o2 = 0;
#pragma unroll
    for (int g = TO_MAXG - 1; g >= 1; --g) {
        if (g < d.nd) {
            const int64_t q = rem / d.ext[g], c = rem - q * d.ext[g];
            o0 += c * d.s[0][g]; o1 += c * d.s[1][g]; o2 += c * d.s[2][g];
            rem = q;
        }
    }
    o0 += rem * d.s[0][0]; o1 += rem * d.s[1][0]; o2 += rem * d.s[2][0];
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
    bool vec = !byte_op1<F>::value && d.nd <= 2 && aligned16(out) && d.ext[d.nd - 1] % 4 == 0;
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

}  // namespace nnhip
