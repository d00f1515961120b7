// recurrent_common.h -- what the one-launch recurrences share (recurrent.hip: nn.LSTM; recurrent_gru.hip: nn.GRU / nn.RNN / both
// directions of nn.Bidirectional).  Device side: the workgroup shape, the nonlinearities and their derivatives taken from the
// ACTIVATED value, the impossible-shape guard and the staging of h0 into LDS.  Host side: the packed-weight workspace, the argument
// checks, the tier dispatch, the launch helper and the backward's whole-sequence epilogue (defined in recurrent_gru.hip).
// The kernels' MFMA loops, lane coordinates and state registers are NOT shared between the LSTM and the GRU / RNN kernels: each
// attempt cost the LSTM's two- and four-tile instances 0.5-4 % (EXPERIMENTS.md 5.9), so recurrent.hip keeps its own.
#pragma once
#include <stdio.h>

#include <type_traits>

#include "common.h"

namespace nnhip {
int gemm_f32(const float* A, const float* B, float* C, const float* bias, float* preact, int64_t M, int64_t N, int64_t K, int64_t lda,
             int64_t ldb, int64_t ldc, bool a_kmajor, bool b_kmajor, int64_t batch, int64_t sA, int64_t sB, int64_t sC, int act,
             float beta, hipStream_t st);
int colsum(const float* X, int64_t rows, int64_t cols, int64_t ld, float* out, hipStream_t st);

typedef float f32x4_ __attribute__((ext_vector_type(4)));

constexpr int kRecRows = 16;             // batch rows per workgroup: the M of one 16x16x4 MFMA
constexpr int kRecWaves = 8;             // 2 waves per SIMD
constexpr int kRecThreads = kRecWaves * kWave;
constexpr int kRecMaxH = 512;            // 4 hidden tiles per wave; the LSTM backward's dG_t image is 16 x (4Hp + 4) floats of LDS

__device__ __forceinline__ float rec_act(int kind, float x) {
    if (kind == NNHIP_LSTM_TANH) return tanhf(x);
    if (kind == NNHIP_LSTM_SIGMOID) return 1.0f / (1.0f + expf(-x));
    return fmaxf(x, 0.0f);
}
// derivative from the ACTIVATED value y = act(x): tanh 1 - y^2, sigmoid y (1 - y), relu [x > 0] == [y > 0] (lstm.py:457: 0 at x <= 0)
__device__ __forceinline__ float rec_dact_y(int kind, float y) {
    if (kind == NNHIP_LSTM_TANH) return 1.0f - y * y;
    if (kind == NNHIP_LSTM_SIGMOID) return y * (1.0f - y);
    return y > 0.0f ? 1.0f : 0.0f;
}

// True where this instance cannot run the shape (impossible by the host's dispatch; `also` is the instance's own condition): the
// kernel leaves the outputs alone and returns, and `code` is raised in the library's device error word.
template <int MAXT>
__device__ __forceinline__ bool rec_bad_shape(int Hp, unsigned* err, unsigned code, bool also = false) {
    if (Hp > MAXT * 16 * kRecWaves || also || blockDim.x != kRecThreads) {
        if (threadIdx.x == 0 && err) __hip_atomic_store(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return true;
    }
    return false;
}

// a state s [B, H] (NULL = zeros) as the 16 x ldh LDS image that is the first step's A operand; padding rows and columns zero
__device__ __forceinline__ void rec_stage_state(const float* s, int B, int H, int Hp, int ldh, int b0, float* img) {
    for (int idx = threadIdx.x; idx < kRecRows * Hp; idx += kRecThreads) {
        const int r = idx / Hp, j = idx - r * Hp, b = b0 + r;
        img[r * ldh + j] = (s && b < B && j < H) ? s[(int64_t)b * H + j] : 0.0f;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct RecWeights {          // one direction; gate order f, i, o, c (LSTM), z, r, h (GRU) or the single gate (RNN)
    const float* wx[4];
    const float* wh[4];
    const float* b[4];
};
struct RecGrads {
    float* dwx[4];
    float* dwh[4];
    float* db[4];
};

// what every entry checks of its sizes, codes, X and the weights of its ng gates and ndir directions
int rec_common_checks(const char* fn, const float* X, const RecWeights* w, int ng, int64_t B, int64_t T, int64_t in, int64_t H, int nl,
                      int rnl, int ndir);
// packs the parameters of every direction into arena 2; *out = its base: ndir x (wxp [in, G] | whp [Hp, G] | bp [G]) | extra floats,
// G = ng Hp: column g Hp + j = gate g's column j, rows and columns >= H zero
int rec_pack(const RecWeights* w, int ng, int ndir, int64_t in, int H, int Hp, size_t extra, hipStream_t st, float** out);
// The backward's time-parallel part, whole-sequence GEMMs straight into the caller's buffers.  ws: rec_pack's base; dG [ndir, B, T, G]
// in input order.  dX = sum over directions of dG W_x^T (the second product through dX1 and one elementwise add); per direction and
// gate dW_x = X^T dG_g, dW_h = left^T dG_g, db = colsum(dG_g), where left is hprev [ndir, B, T, H] or, for the LAST gate where
// last_left is given, last_left + d * last_stride (the GRU's r * h_{t-1}).
int rec_bwd_epilogue(const float* X, const float* ws, const float* dG, const float* hprev, const float* last_left, int64_t last_stride,
                     float* dX, float* dX1, const RecGrads* grads, int ng, int ndir, int64_t B, int64_t T, int64_t in, int64_t H, int Hp,
                     hipStream_t st);

template <typename Args>
static int recurrence_run(void (*kern)(const Args), const Args& a, dim3 blocks, size_t lds, hipStream_t st, const char* name) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            char what[96];
            snprintf(what, sizeof what, "hipFuncSetAttribute(%s)", name);
            return hip_status(e, what);
        }
    }
    hipLaunchKernelGGL(kern, blocks, dim3(kRecThreads), lds, st, a);
    NNHIP_LAUNCH_CHECK(name);
    return 0;
}

// The tiers of every kernel family: 1 / 2 / 4 hidden tiles per wave for Hp <= 128 / 256 / 512.  run(std::integral_constant<int, MAXT>)
// launches the family's instance.
template <typename Run>
static int rec_tiers(int Hp, Run run) {
    if (Hp <= 128) return run(std::integral_constant<int, 1>{});
    if (Hp <= 256) return run(std::integral_constant<int, 2>{});
    return run(std::integral_constant<int, 4>{});
}

}  // namespace nnhip
