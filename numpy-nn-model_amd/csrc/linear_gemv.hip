// linear_gemv.hip -- weight-streaming Linear forward for 1..8 rows (the single-token steps of KV-cached decoding).  ABI 214
//   O[r, n] = sum_k X[r, k] W[n, k]  (+ b[n])  (+ addend[r, n]),   W [out, in] row-major: one contiguous row of W per output.
// Exact fp32 on the vector ALU, ONE launch, no workspace, no atomics: every W element is read once, straight from global memory
// into VGPRs with 16-byte loads (no LDS round trip for W), and used for all ROWS rows.  DESIGN.md section 5.12.
//
// The arithmetic of one output is fixed by (in_features) alone -- not by ROWS, not by the tile shape, not by the other rows:
//   1. k is cut into groups of four consecutive elements (one float4); thread t of the 256-thread block owns groups t, t + 256,
//      t + 512, ... and folds them, in that order and .x .y .z .w inside a group, into ONE fmaf chain that starts at 0;
//   2. the 256 chain ends go through LDS: thread q of eight adds the 32 ends  q, q + 8, q + 16, ...  in that order;
//   3. the eight sums meet in a three-level tree over the lanes (q ^ 1, q ^ 2, q ^ 4);
//   4. (acc + b[n]) + addend[r, n], each step rounded.
// So row r of an 8-row call carries the bits of a 1-row call on that row, and a rerun repeats itself.  K is split among the four
// waves of a block only -- never across blocks -- so nothing is merged through memory.
//
// NR output columns per block share every X load (X is tiny: it is read through the caches, rows * in * 4 bytes per block) and give
// each lane NR * U independent 16-byte W loads in flight before the first wait.  NR and U change how much is in flight, not what is
// added to what.
#include "common.h"

namespace nnhip {

constexpr int kGemvThreads = 256;
constexpr int kGemvStride = kGemvThreads + 8;      // LDS row stride of the chain ends: the eight-lane groups of a wave land on 64 distinct banks

static long long g_linear_gemv_launches = 0;
long long linear_gemv_launches() { return g_linear_gemv_launches; }

// one group of four k: VEC = one 16-byte load; otherwise four guarded 4-byte loads (any alignment >= 4, any in_features)
template <bool VEC>
__device__ __forceinline__ float4 gemv_ld4(const float* p, int g, int K) {
    if constexpr (VEC) {
        return reinterpret_cast<const float4*>(p)[g];
    } else {
        const int k = 4 * g;
        float4 v;
        v.x = p[k];
        v.y = k + 1 < K ? p[k + 1] : 0.f;
        v.z = k + 2 < K ? p[k + 2] : 0.f;
        v.w = k + 3 < K ? p[k + 3] : 0.f;
        return v;
    }
}
// the chain step of one group; elements past the end of a row are SKIPPED, not added as zeros (no 0 * x term ever exists)
template <bool VEC>
__device__ __forceinline__ float gemv_fma4(float acc, const float4& x, const float4& w, int g, int K) {
    acc = fmaf(x.x, w.x, acc);
    if constexpr (VEC) {
        acc = fmaf(x.y, w.y, acc);
        acc = fmaf(x.z, w.z, acc);
        acc = fmaf(x.w, w.w, acc);
    } else {
        const int k = 4 * g;
        if (k + 1 < K) acc = fmaf(x.y, w.y, acc);
        if (k + 2 < K) acc = fmaf(x.z, w.z, acc);
        if (k + 3 < K) acc = fmaf(x.w, w.w, acc);
    }
    return acc;
}

// UU groups per lane and column: all NR * UU W loads are issued before the first fmaf needs one
template <int ROWS, int NR, int UU, bool VEC>
__device__ __forceinline__ void gemv_step(float (&acc)[NR][ROWS], const float* X, const float* const (&wp)[NR], int g, int K) {
    float4 w[UU][NR];
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
        for (int i = 0; i < NR; ++i) w[u][i] = gemv_ld4<VEC>(wp[i], g + u * kGemvThreads, K);
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const float4 x = gemv_ld4<VEC>(X + (int64_t)r * K, g + u * kGemvThreads, K);
#pragma unroll
            for (int i = 0; i < NR; ++i) acc[i][r] = gemv_fma4<VEC>(acc[i][r], x, w[u][i], g + u * kGemvThreads, K);
        }
}

template <int ROWS, int NR, int U, bool VEC>
__global__ __launch_bounds__(kGemvThreads) void linear_gemv_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                                  const float* __restrict__ bias, const float* addend, float* O,
                                                                  int K, int N) {
    constexpr int V = NR * ROWS;                       // outputs of this block
    static_assert(V * 8 <= kGemvThreads, "eight threads finish one output");
    __shared__ float part[V * kGemvStride];
    const int t = threadIdx.x;
    const int n0 = blockIdx.x * NR;
    const float* wp[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {                     // a column past the end re-reads the last row; its result is dropped
        const int n = n0 + i < N ? n0 + i : N - 1;
        wp[i] = W + (int64_t)n * K;
    }
    float acc[NR][ROWS];
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[i][r] = 0.f;

    const int G = (K + 3) >> 2;                        // groups of four k
    int g = t;
    for (; g + kGemvThreads * (U - 1) < G; g += kGemvThreads * U) gemv_step<ROWS, NR, U, VEC>(acc, X, wp, g, K);
    for (; g < G; g += kGemvThreads) gemv_step<ROWS, NR, 1, VEC>(acc, X, wp, g, K);

#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) part[(i * ROWS + r) * kGemvStride + t] = acc[i][r];
    __syncthreads();
    const int v = t >> 3, q = t & 7;
    const float* pv = part + (v < V ? v : V - 1) * kGemvStride + q;
    float s = pv[0];
#pragma unroll
    for (int j = 1; j < kGemvThreads / 8; ++j) s += pv[8 * j];
    s += dpp_f32<kDppXor1>(s);
    s += dpp_f32<kDppXor2>(s);
    s += dpp_f32<kDppHalfMirror>(s);                   // the quads hold equal sums by now: lane q meets the other quad of its eight
    const int i = v / ROWS, r = v - i * ROWS, n = n0 + i;
    if (q == 0 && v < V && n < N) {
        if (bias) s += bias[n];
        if (addend) s += addend[(int64_t)r * N + n];
        O[(int64_t)r * N + n] = s;
    }
}

template <int ROWS, int NR, int U, bool VEC>
static void gemv_launch(const float* X, const float* W, const float* b, const float* addend, float* O, int K, int N, hipStream_t st) {
    hipLaunchKernelGGL((linear_gemv_kernel<ROWS, NR, U, VEC>), dim3((unsigned)ceil_div(N, NR)), dim3(kGemvThreads), 0, st, X, W, b,
                       addend, O, K, N);
}

template <int ROWS>
static void gemv_launch_rows(const float* X, const float* W, const float* b, const float* addend, float* O, int K, int N, bool vec,
                             hipStream_t st) {
    // wide layers: four columns per block (four blocks or more per CU still); narrow ones (GPT-2's 3072 -> 768) keep two, so that
    // 768 outputs are 384 blocks.  The unaligned path is there for correctness, not speed: one shape.
    if (!vec) gemv_launch<ROWS, 2, 2, false>(X, W, b, addend, O, K, N, st);
    else if (N >= 2048) gemv_launch<ROWS, 4, 2, true>(X, W, b, addend, O, K, N, st);
    else gemv_launch<ROWS, 2, 2, true>(X, W, b, addend, O, K, N, st);
}

// rows 1..8, in >= 1, out >= 1, pointers checked by the caller (linear.hip)
int linear_gemv(const float* X, const float* W, const float* b, const float* addend, float* O, int64_t rows, int64_t in, int64_t out,
                hipStream_t st) {
    if (in > (int64_t)0x7FFFFFF0 || out > (int64_t)0x7FFFFFF0) {
        set_last_error("nnhipLinearGemvForward: in_features / out_features beyond 2^31 - 16");
        return NNHIP_EINVAL;
    }
    const int K = (int)in, N = (int)out;
    const bool vec = (K & 3) == 0 && aligned16(X) && aligned16(W);
    switch (rows) {
        case 1: gemv_launch_rows<1>(X, W, b, addend, O, K, N, vec, st); break;
        case 2: gemv_launch_rows<2>(X, W, b, addend, O, K, N, vec, st); break;
        case 3: gemv_launch_rows<3>(X, W, b, addend, O, K, N, vec, st); break;
        case 4: gemv_launch_rows<4>(X, W, b, addend, O, K, N, vec, st); break;
        case 5: gemv_launch_rows<5>(X, W, b, addend, O, K, N, vec, st); break;
        case 6: gemv_launch_rows<6>(X, W, b, addend, O, K, N, vec, st); break;
        case 7: gemv_launch_rows<7>(X, W, b, addend, O, K, N, vec, st); break;
        case 8: gemv_launch_rows<8>(X, W, b, addend, O, K, N, vec, st); break;
        default: set_last_error("nnhipLinearGemvForward: rows must be 1..%d", NNHIP_LINEAR_GEMV_MAX_ROWS); return NNHIP_EINVAL;
    }
    NNHIP_LAUNCH_CHECK("linear_gemv_kernel");
    ++g_linear_gemv_launches;
    return 0;
}

}  // namespace nnhip
