// recurrent_common.h -- what the one-launch recurrences share (recurrent.hip: nn.LSTM; recurrent_gru.hip: nn.GRU / nn.RNN): the
// workgroup shape, the nonlinearities and their derivatives taken from the ACTIVATED value, and the launch helper.
#pragma once
#include <stdio.h>

#include "common.h"

namespace nnhip {
int gemm_f32(const float* A, const float* B, float* C, const float* bias, float* preact, int64_t M, int64_t N, int64_t K, int64_t lda,
             int64_t ldb, int64_t ldc, bool a_kmajor, bool b_kmajor, int64_t batch, int64_t sA, int64_t sB, int64_t sC, int act,
             float beta, hipStream_t st);
int colsum(const float* X, int64_t rows, int64_t cols, int64_t ld, float* out, hipStream_t st);

typedef float f32x4_ __attribute__((ext_vector_type(4)));

constexpr int kLstmRows = 16;            // batch rows per workgroup: the M of one 16x16x4 MFMA
constexpr int kLstmWaves = 8;            // 2 waves per SIMD
constexpr int kLstmThreads = kLstmWaves * kWave;
constexpr int kLstmMaxH = 512;           // 4 hidden tiles per wave; the backward's dG_t image is 16 x (4Hp + 4) floats of LDS

__device__ __forceinline__ float lstm_act(int kind, float x) {
    if (kind == NNHIP_LSTM_TANH) return tanhf(x);
    if (kind == NNHIP_LSTM_SIGMOID) return 1.0f / (1.0f + expf(-x));
    return fmaxf(x, 0.0f);
}
// derivative from the ACTIVATED value y = act(x): tanh 1 - y^2, sigmoid y (1 - y), relu [x > 0] == [y > 0] (lstm.py:457: 0 at x <= 0)
__device__ __forceinline__ float lstm_dact_y(int kind, float y) {
    if (kind == NNHIP_LSTM_TANH) return 1.0f - y * y;
    if (kind == NNHIP_LSTM_SIGMOID) return y * (1.0f - y);
    return y > 0.0f ? 1.0f : 0.0f;
}

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
    hipLaunchKernelGGL(kern, blocks, dim3(kLstmThreads), lds, st, a);
    NNHIP_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace nnhip
