// recurrent.hip -- nn.LSTM: the whole timestep loop of a layer in ONE launch, forward and backward (ABI 211, net-new; the reference
// has no CUDA LSTM).  CPU semantics: neunet/nn/layers/lstm.py:312-362 (forward), :16-143 (backward), :412-460 (nonlinearities).
//
// Split of the work:
//   * time-parallel: the input projection P = X W_x + b for all B*T rows and the four gates at once, and after the backward recurrence
//     dX = dG W_x^T, dW_x = X^T dG, dW_h = H_prev^T dG, db = colsum(dG) -- the library's GEMM / column-sum kernels;
//   * the recurrence: one workgroup per slice of 16 batch rows runs all T steps.  A step is gates = P_t + h_{t-1} W_h on
//     v_mfma_f32_16x16x4_f32, then the cell update in registers; h_t goes to the next step through LDS.  Batch rows are independent:
//     no inter-workgroup communication, no grid barrier, no residency requirement.
// The four gate weights are packed per call into [in, 4Hp] / [Hp, 4Hp] (Hp = H rounded up to 16, zero padding) in the library's
// recurrent workspace block (arena 2): every kernel below is branch-free over the padding, and the padded columns of the saved gates
// and of dG are finite (zero in dG), so the K = 4Hp dX GEMM is exact.
// This file is the LSTM's step arithmetic and its two entries.  The pack, the argument checks, the tier dispatch and the backward's
// whole-sequence GEMMs are the GRU / RNN entries' (recurrent_common.h, with ng = 4 and ndir = 1).  The non-resident MFMA loops below
// are recurrent_gru.hip's rec_mfma_cols<4> / rec_mfma_rows written out: called as helpers they cost the two- and four-tile
// instances 0.6-3.9 % (EXPERIMENTS.md 5.9).
#include <stdlib.h>

#include "common.h"
#include "recurrent_common.h"

namespace nnhip {

struct LstmFwdArgs {
    float* gates;           // [B, T, 4Hp]: P (pre-activations incl. bias) on entry, activated f, i, o, g on exit
    const float* whp;       // [Hp, 4Hp]
    const float* h0;        // [B, H] or NULL (zeros)
    const float* c0;
    float* Y;               // [B, T, H]    h_t
    float* cell;            // [B, T+1, H]  c_{t-1} at index t (index 0 = c0)
    float* hprev;           // [B, T, H]    h_{t-1}
    float* hT;              // [B, H] or NULL; may alias h0 (cycled state)
    float* cT;              // may alias c0
    unsigned* err;
    int B, T, H, Hp, nl, rnl;
};

// One workgroup = 16 batch rows, all T steps.  Wave w owns hidden tiles jt = w, w + 8, ... (16 columns each) of ALL FOUR gates, so
// the MFMA accumulators of f, i, o, g for one (row, column) sit in the same lane and the cell update needs no data movement:
// C/D map of 16x16x4: row = 4 (lane >> 4) + r, column = lane & 15.  The reduction index is permuted -- lane group q = lane >> 4 covers
// k = q KS + s at k-step s (KS = Hp / 4) -- so that a lane's A operands h_{t-1}[row][q KS + s] are consecutive in LDS.
// RES: W_h stays in registers for the whole sequence (Hp == 128: one tile per wave, 32 k-steps x 4 gates = 128 VGPRs); otherwise
// every step re-reads its W_h columns from L2.
template <bool RES, int MAXT>
__global__ __launch_bounds__(kRecThreads, 1) void lstm_fwd_kernel(const LstmFwdArgs a) {
    extern __shared__ float lds[];
    const int Hp = a.Hp, ldh = Hp + 4, G = 4 * Hp, KS = Hp / 4, ntile = Hp / 16;
    if (rec_bad_shape<MAXT>(Hp, a.err, NNHIP_DEVERR_LSTM_SHAPE, RES && (MAXT != 1 || Hp != 128))) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
    const int b0 = blockIdx.x * kRecRows;
    float* hbuf[2] = {lds, lds + kRecRows * ldh};

    rec_stage_state(a.h0, a.B, a.H, Hp, ldh, b0, hbuf[0]);
    float creg[MAXT][4], hreg[MAXT][4];
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt) {
        const int j = (wave + tt * kRecWaves) * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + q * 4 + r;
            const bool v = b < a.B && j < a.H;
            creg[tt][r] = (v && a.c0) ? a.c0[(int64_t)b * a.H + j] : 0.0f;
            hreg[tt][r] = (v && a.h0) ? a.h0[(int64_t)b * a.H + j] : 0.0f;
            if (v) a.cell[(int64_t)b * (a.T + 1) * a.H + j] = creg[tt][r];
        }
    }
    float wreg[RES ? 32 : 1][4];
    if constexpr (RES) {
        const int j = wave * 16 + col;
#pragma unroll
        for (int s = 0; s < 32; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                wreg[s][g] = a.whp[(int64_t)(q * 32 + s) * G + g * Hp + j];
    }
    __syncthreads();

    for (int t = 0; t < a.T; ++t) {
        const float* hcur = hbuf[t & 1];
        float* hnext = hbuf[(t & 1) ^ 1];
#pragma unroll
        for (int tt = 0; tt < MAXT; ++tt) {
            const int jt = wave + tt * kRecWaves;
            if (jt < ntile) {                                         // wave-uniform
                const int j = jt * 16 + col;
                float pre[4][4];                                          // P_t of this tile, in flight under the MFMAs
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int b = b0 + q * 4 + r;
#pragma unroll
                    for (int g = 0; g < 4; ++g) pre[g][r] = b < a.B ? a.gates[((int64_t)b * a.T + t) * G + g * Hp + j] : 0.0f;
                }
                f32x4_ acc[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = f32x4_{0.f, 0.f, 0.f, 0.f};
                const float* arow = hcur + col * ldh + q * KS;
                if constexpr (RES) {
#pragma unroll
                    for (int s = 0; s < 32; ++s) {
                        const float av = arow[s];
#pragma unroll
                        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wreg[s][g], acc[g], 0, 0, 0);
                    }
                } else {
                    // W_h from L2, one chunk of 4 k-steps (16 values) in flight ahead of the MFMAs that use the previous one (KS % 4 == 0)
                    const float* wcol = a.whp + (int64_t)q * KS * G + j;
                    float wn[4][4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int g = 0; g < 4; ++g) wn[u][g] = wcol[(int64_t)u * G + g * Hp];
#pragma unroll 1
                    for (int s = 0; s < KS; s += 4) {
                        float wv[4][4];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int g = 0; g < 4; ++g) wv[u][g] = wn[u][g];
                        if (s + 4 < KS) {
#pragma unroll
                            for (int u = 0; u < 4; ++u)
#pragma unroll
                                for (int g = 0; g < 4; ++g) wn[u][g] = wcol[(int64_t)(s + 4 + u) * G + g * Hp];
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const float av = arow[s + u];
#pragma unroll
                            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wv[u][g], acc[g], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = q * 4 + r, b = b0 + row;
                    const float f = rec_act(a.rnl, acc[0][r] + pre[0][r]);
                    const float i = rec_act(a.rnl, acc[1][r] + pre[1][r]);
                    const float o = rec_act(a.rnl, acc[2][r] + pre[2][r]);
                    const float gg = rec_act(a.nl, acc[3][r] + pre[3][r]);
                    const float c = f * creg[tt][r] + i * gg;
                    const float h = o * rec_act(a.nl, c);
                    const bool v = b < a.B && j < a.H;
                    if (b < a.B) {
                        float* gp = a.gates + ((int64_t)b * a.T + t) * G + j;
                        gp[0] = f;
                        gp[Hp] = i;
                        gp[2 * Hp] = o;
                        gp[3 * Hp] = gg;
                    }
                    if (v) {
                        const int64_t bt = (int64_t)b * a.T + t;
                        a.cell[((int64_t)b * (a.T + 1) + t + 1) * a.H + j] = c;
                        a.Y[bt * a.H + j] = h;
                        a.hprev[bt * a.H + j] = hreg[tt][r];
                    }
                    creg[tt][r] = v ? c : 0.0f;
                    hreg[tt][r] = v ? h : 0.0f;
                    hnext[row * ldh + j] = hreg[tt][r];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt) {
        const int j = (wave + tt * kRecWaves) * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + q * 4 + r;
            if (b < a.B && j < a.H) {
                if (a.hT) a.hT[(int64_t)b * a.H + j] = hreg[tt][r];
                if (a.cT) a.cT[(int64_t)b * a.H + j] = creg[tt][r];
            }
        }
    }
}

struct LstmBwdArgs {
    const float* gates;     // [B, T, 4Hp] activated (forward output)
    const float* cell;      // [B, T+1, H]
    const float* whp;       // [Hp, 4Hp]
    const float* dY;        // [B, T, H] or NULL
    const float* dYlast;    // [B, H] or NULL: gradient of h_{T-1} alone (return_sequences "last")
    float* dG;              // [B, T, 4Hp] pre-activation gate gradients (padded columns 0)
    unsigned* err;
    int B, T, H, Hp, nl, rnl;
};

// one lane's saved values of step t for rows rb .. rb+3 of column j
__device__ __forceinline__ void lstm_bwd_load(const LstmBwdArgs& a, int t, int rb, int j, float (&gv)[4][4], float (&cn)[4], float (&cp)[4],
                                              float (&dy)[4]) {
    const int G = 4 * a.Hp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = rb + r;
        const bool v = b < a.B && j < a.H;
        const int64_t bt = (int64_t)b * a.T + t;
#pragma unroll
        for (int g = 0; g < 4; ++g) gv[g][r] = v ? a.gates[bt * G + g * a.Hp + j] : 0.0f;
        cn[r] = v ? a.cell[((int64_t)b * (a.T + 1) + t + 1) * a.H + j] : 0.0f;
        cp[r] = v ? a.cell[((int64_t)b * (a.T + 1) + t) * a.H + j] : 0.0f;
        float d = (v && a.dY) ? a.dY[bt * a.H + j] : 0.0f;
        if (v && a.dYlast && t == a.T - 1) d += a.dYlast[(int64_t)b * a.H + j];
        dy[r] = d;
    }
}

// BPTT, t = T-1 ... 0, dh and dc carried in registers.  dh_{t} = grad_t + dG_{t+1} W_h^T: an MFMA over K = 4Hp whose A operand is the
// previous step's dG image in LDS and whose output tile has the forward's (row, column) ownership, so the gate values a lane loads
// are those of its own accumulator elements.  Lane group q = lane >> 4 covers the reduction indices q Hp + s: gate q's columns.
// RES: the wave's W_h^T slice in registers (Hp == 128: 128 VGPRs).
template <bool RES, int MAXT>
__global__ __launch_bounds__(kRecThreads, 1) void lstm_bwd_kernel(const LstmBwdArgs a) {
    extern __shared__ float lds[];
    const int Hp = a.Hp, G = 4 * Hp, ldg = G + 4, ntile = Hp / 16;
    // rec_bad_shape() written out: through the helper lstm_bwd_kernel<true, 1> takes 232 VGPRs instead of 230
    if (Hp > MAXT * 16 * kRecWaves || (RES && (MAXT != 1 || Hp != 128)) || blockDim.x != kRecThreads) {
        if (threadIdx.x == 0 && a.err) __hip_atomic_store(a.err, (unsigned)NNHIP_DEVERR_LSTM_SHAPE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
    const int b0 = blockIdx.x * kRecRows;
    float wreg[RES ? 128 : 1];
    if constexpr (RES) {
        const int j = wave * 16 + col;
#pragma unroll
        for (int s = 0; s < 128; ++s) wreg[s] = a.whp[(int64_t)j * G + q * Hp + s];
    }
    float dcreg[MAXT][4];
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dcreg[tt][r] = 0.0f;

    for (int t = a.T - 1; t >= 0; --t) {
        // the step's saved values, loaded ahead of the MFMAs where the registers allow it (MAXT <= 2), else after the barrier
        constexpr int PF = MAXT <= 2 ? MAXT : 1;
        float gv[PF][4][4], cn[PF][4], cp[PF][4], dy[PF][4];
        if constexpr (MAXT <= 2) {
#pragma unroll
            for (int tt = 0; tt < MAXT; ++tt)
                lstm_bwd_load(a, t, b0 + q * 4, (wave + tt * kRecWaves) * 16 + col, gv[tt], cn[tt], cp[tt], dy[tt]);
        }
        f32x4_ acc[MAXT];
#pragma unroll
        for (int tt = 0; tt < MAXT; ++tt) {
            acc[tt] = f32x4_{0.f, 0.f, 0.f, 0.f};
            const int jt = wave + tt * kRecWaves;
            if (jt < ntile && t != a.T - 1) {                         // wave-uniform; no dG_{T} term at the last step
                const float* arow = lds + col * ldg + q * Hp;
                if constexpr (RES) {
#pragma unroll
                    for (int s = 0; s < 128; ++s) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[s], wreg[s], acc[tt], 0, 0, 0);
                } else {
                    // W_h^T from L2: a lane's 16 values of a chunk are contiguous (four 16-B loads), one chunk ahead (Hp % 16 == 0)
                    const f32x4_* w = reinterpret_cast<const f32x4_*>(a.whp + (int64_t)(jt * 16 + col) * G + q * Hp);
                    f32x4_ wn[4] = {w[0], w[1], w[2], w[3]};
#pragma unroll 1
                    for (int s = 0; s < Hp; s += 16) {
                        const f32x4_ wv[4] = {wn[0], wn[1], wn[2], wn[3]};
                        if (s + 16 < Hp) {
#pragma unroll
                            for (int u = 0; u < 4; ++u) wn[u] = w[(s + 16) / 4 + u];
                        }
#pragma unroll
                        for (int u = 0; u < 16; ++u)
                            acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[s + u], wv[u >> 2][u & 3], acc[tt], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                                              // every wave is done reading dG_{t+1}
#pragma unroll
        for (int tt = 0; tt < MAXT; ++tt) {
            const int jt = wave + tt * kRecWaves;
            if (jt < ntile) {
                    const int j = jt * 16 + col;
                    const int pt = MAXT <= 2 ? tt : 0;
                    if constexpr (MAXT > 2) lstm_bwd_load(a, t, b0 + q * 4, j, gv[0], cn[0], cp[0], dy[0]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = q * 4 + r, b = b0 + row;
                        const bool v = b < a.B && j < a.H;
                        const float f = gv[pt][0][r], i = gv[pt][1][r], o = gv[pt][2][r], gg = gv[pt][3][r];
                        const float dh = dy[pt][r] + acc[tt][r];
                        const float tc = rec_act(a.nl, cn[pt][r]);
                        const float dc = dh * o * rec_dact_y(a.nl, tc) + dcreg[tt][r];
                        float d[4];
                        d[2] = dh * tc * rec_dact_y(a.rnl, o);
                        d[0] = dc * cp[pt][r] * rec_dact_y(a.rnl, f);
                        d[1] = dc * gg * rec_dact_y(a.rnl, i);
                        d[3] = dc * i * rec_dact_y(a.nl, gg);
                        dcreg[tt][r] = v ? dc * f : 0.0f;
                        float* out = a.dG + ((int64_t)b * a.T + t) * G + j;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float x = v ? d[g] : 0.0f;
                            lds[row * ldg + g * Hp + j] = x;
                            if (b < a.B) out[g * Hp] = x;
                        }
                    }
            }
        }
        __syncthreads();
    }
}

static bool lstm_resident_on() {
    static const int on = env_int("NNHIP_LSTM_RESIDENT", 1);   // A/B knob
    return on != 0;
}

static RecWeights rec_from_lstm(const nnhipLSTMWeights* w) {
    RecWeights out;
    for (int g = 0; g < 4; ++g) { out.wx[g] = w->wx[g]; out.wh[g] = w->wh[g]; out.b[g] = w->b[g]; }
    return out;
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipLSTMForward(const float* X, const nnhipLSTMWeights* w, const float* h0, const float* c0, float* Y, float* gates,
                                float* cell, float* hprev, float* hT, float* cT, int64_t B, int64_t T, int64_t in, int64_t H, int nl,
                                int rnl, nnhipStream_t stream) {
    const char* fn = "nnhipLSTMForward";
    NNHIP_CHECK_ARG(w, NNHIP_EINVAL, "%s: null X / weights", fn);
    const RecWeights rw = rec_from_lstm(w);
    if (int rc = rec_common_checks(fn, X, &rw, 4, B, T, in, H, nl, rnl, 1)) return rc;
    NNHIP_CHECK_ARG(Y && gates && cell && hprev, NNHIP_EINVAL, "%s: null output / saved-state buffer", fn);
    NNHIP_CHECK_ARG(aligned4(h0) && aligned4(c0) && aligned4(Y) && aligned4(gates) && aligned4(cell) && aligned4(hprev) && aligned4(hT) &&
                        aligned4(cT), NNHIP_EALIGN, "%s: misaligned state / output buffer", fn);
    hipStream_t st = (hipStream_t)stream;
    const int Hp = (int)ceil_div(H, 16) * 16;
    const int64_t G = 4 * (int64_t)Hp;
    float* ws = nullptr;                                        // wxp [in, 4Hp] | whp [Hp, 4Hp] | bp [4Hp]
    int rc = rec_pack(&rw, 4, 1, in, (int)H, Hp, 0, st, &ws);
    if (rc) return rc;
    // P = X W_x + b for all B*T rows and the four gates: one GEMM into the saved-gates buffer
    rc = gemm_f32(X, ws, gates, ws + (in + Hp) * G, nullptr, B * T, G, in, in, G, G, true, false, 1, 0, 0, 0, 0, 1.0f, st);
    if (rc) return rc;
    LstmFwdArgs a;
    a.gates = gates; a.whp = ws + in * G; a.h0 = h0; a.c0 = c0; a.Y = Y; a.cell = cell; a.hprev = hprev; a.hT = hT; a.cT = cT;
    a.err = device_error_word();
    a.B = (int)B; a.T = (int)T; a.H = (int)H; a.Hp = Hp; a.nl = nl; a.rnl = rnl;
    const dim3 blocks((unsigned)ceil_div(B, kRecRows));
    const size_t lds = (size_t)2 * kRecRows * (Hp + 4) * sizeof(float);
    if (Hp == 128 && lstm_resident_on()) return recurrence_run(lstm_fwd_kernel<true, 1>, a, blocks, lds, st, "lstm_fwd_kernel");
    return rec_tiers(Hp, [&](auto mt) { return recurrence_run(lstm_fwd_kernel<false, decltype(mt)::value>, a, blocks, lds, st, "lstm_fwd_kernel"); });
}

extern "C" int nnhipLSTMBackward(const float* X, const nnhipLSTMWeights* w, const float* gates, const float* cell, const float* hprev,
                                 const float* dY, const float* dYlast, float* dX, const nnhipLSTMGrads* grads, int64_t B, int64_t T,
                                 int64_t in, int64_t H, int nl, int rnl, nnhipStream_t stream) {
    const char* fn = "nnhipLSTMBackward";
    NNHIP_CHECK_ARG(w, NNHIP_EINVAL, "%s: null X / weights", fn);
    const RecWeights rw = rec_from_lstm(w);
    if (int rc = rec_common_checks(fn, X, &rw, 4, B, T, in, H, nl, rnl, 1)) return rc;
    NNHIP_CHECK_ARG(gates && cell && hprev, NNHIP_EINVAL, "%s: null saved-state buffer", fn);
    NNHIP_CHECK_ARG(dY || dYlast, NNHIP_EINVAL, "%s: null dY and dYlast", fn);
    NNHIP_CHECK_ARG(aligned4(gates) && aligned4(cell) && aligned4(hprev) && aligned4(dY) && aligned4(dYlast) && aligned4(dX), NNHIP_EALIGN,
                    "%s: misaligned saved-state / gradient buffer", fn);
    RecGrads rg;
    for (int g = 0; grads && g < 4; ++g) {
        rg.dwx[g] = grads->dwx[g]; rg.dwh[g] = grads->dwh[g]; rg.db[g] = grads->db[g];
        NNHIP_CHECK_ARG(aligned4(rg.dwx[g]) && aligned4(rg.dwh[g]) && aligned4(rg.db[g]), NNHIP_EALIGN,
                        "%s: misaligned parameter gradient buffer", fn);
    }
    hipStream_t st = (hipStream_t)stream;
    const int Hp = (int)ceil_div(H, 16) * 16;
    const int64_t G = 4 * (int64_t)Hp, BT = B * T;
    float* ws = nullptr;                                        // wxp | whp | bp | dG [B, T, 4Hp]
    int rc = rec_pack(&rw, 4, 1, in, (int)H, Hp, (size_t)(BT * G), st, &ws);
    if (rc) return rc;
    float* dG = ws + (in + Hp) * G + G;
    LstmBwdArgs a;
    a.gates = gates; a.cell = cell; a.whp = ws + in * G; a.dY = dY; a.dYlast = dYlast; a.dG = dG;
    a.err = device_error_word();
    a.B = (int)B; a.T = (int)T; a.H = (int)H; a.Hp = Hp; a.nl = nl; a.rnl = rnl;
    const dim3 blocks((unsigned)ceil_div(B, kRecRows));
    const size_t lds = (size_t)kRecRows * (G + 4) * sizeof(float);
    if (Hp == 128 && lstm_resident_on()) rc = recurrence_run(lstm_bwd_kernel<true, 1>, a, blocks, lds, st, "lstm_bwd_kernel");
    else rc = rec_tiers(Hp, [&](auto mt) { return recurrence_run(lstm_bwd_kernel<false, decltype(mt)::value>, a, blocks, lds, st, "lstm_bwd_kernel"); });
    if (rc) return rc;
    return rec_bwd_epilogue(X, ws, dG, hprev, nullptr, 0, dX, nullptr, grads ? &rg : nullptr, 4, 1, B, T, in, H, Hp, st);
}
