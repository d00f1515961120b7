// recurrent_gru.hip -- nn.GRU, nn.RNN and the two directions of nn.Bidirectional: the whole timestep loop of a layer, for one or both
// directions, in ONE launch, forward and backward (ABI 220, net-new; the reference has no CUDA recurrences).  CPU semantics:
// neunet/nn/layers/gru.py:273-311 (forward), :66-110 (backward); rnn.py:151-159, :46-56; bidirectional.py:16-23, :89-103 (merge).
//
// The split of the work is the LSTM's (recurrent.hip): the input projection P = X W_x + b of all B*T rows
// and the parameter gradients are whole-sequence GEMMs; the recurrence is one workgroup per 16 batch rows and direction
// (blockIdx.y) that runs all T steps on v_mfma_f32_16x16x4_f32 with h going from step to step through LDS.
// What differs is the GRU's step: the candidate needs (r_t * h_{t-1}) W_hh, so r must be complete -- across all waves -- before the
// second product starts.  A step is two MFMA phases with a barrier between them, forward and backward.  The RNN is the same
// skeleton with one gate and one phase (NG = 1).
// Direction 1 consumes the input backwards: its step s reads x[:, T-1-s] and writes its output at index s (what the reference's
// reverse_layer(X.flip(1)) yields; the reverse output is not flipped back).  Everything that is a function of an input row -- P,
// the saved gates, h_{t-1}, dG, r * h_{t-1} -- is indexed by INPUT time for both directions, so no flipped copy of X or dX exists.
// Weights are packed per call and direction into [in, NG Hp] / [Hp, NG Hp] / [NG Hp] (Hp = H rounded up to 16, zero padding) in arena
// 2; the kernels are branch-free over the padding, and the padded columns of dG are zero.
#include <algorithm>

#include "common.h"
#include "recurrent_common.h"

namespace nnhip {

struct RecPack {
    RecWeights w[2];
    float* base;            // direction d at base + d * stride: wxp [in, G] | whp [Hp, G] | bp [G]
    int64_t stride, in;
    int H, Hp, ng;
};

__global__ __launch_bounds__(256) void rec_pack_kernel(const RecPack p) {
    const RecWeights& w = p.w[blockIdx.y];
    float* out = p.base + blockIdx.y * p.stride;
    const int64_t G = (int64_t)p.ng * p.Hp;
    const int64_t nx = p.in * G, nh = (int64_t)p.Hp * G, n = nx + nh + G;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        if (idx < nx) {
            const int64_t r = idx / G;
            const int c = (int)(idx - r * G), g = c / p.Hp, j = c - g * p.Hp;
            out[idx] = j < p.H ? w.wx[g][r * p.H + j] : 0.0f;
        } else if (idx < nx + nh) {
            const int64_t e = idx - nx, r = e / G;
            const int c = (int)(e - r * G), g = c / p.Hp, j = c - g * p.Hp;
            out[idx] = (r < p.H && j < p.H) ? w.wh[g][r * p.H + j] : 0.0f;
        } else {
            const int c = (int)(idx - nx - nh), g = c / p.Hp, j = c - g * p.Hp;
            out[idx] = (j < p.H && w.b[g]) ? w.b[g][j] : 0.0f;
        }
    }
}

// acc[g] += A W[:, g Hp + j], g < NA: A is a 16-row LDS image (this lane's row at arow, reduction index permuted as in the LSTM: lane
// group q covers k = q KS + s), W has row pitch G and wcol points at (row q KS, this lane's column of gate 0).  W comes from L2, one
// chunk of 4 k-steps in flight ahead of the MFMAs that use the previous one (KS % 4 == 0).
template <int NA>
__device__ __forceinline__ void rec_mfma_cols(const float* arow, const float* wcol, int G, int Hp, int KS, f32x4_ (&acc)[NA]) {
    float wn[4][NA];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int g = 0; g < NA; ++g) wn[u][g] = wcol[(int64_t)u * G + g * Hp];
#pragma unroll 1
    for (int s = 0; s < KS; s += 4) {
        float wv[4][NA];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int g = 0; g < NA; ++g) wv[u][g] = wn[u][g];
        if (s + 4 < KS) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int g = 0; g < NA; ++g) wn[u][g] = wcol[(int64_t)(s + 4 + u) * G + g * Hp];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float av = arow[s + u];
#pragma unroll
            for (int g = 0; g < NA; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wv[u][g], acc[g], 0, 0, 0);
        }
    }
}

// acc += A W^T over K = 4 KL: lane group q covers k = q KL + i, so the lane's KL weights are contiguous at w (16-byte aligned,
// KL % 4 == 0) and its A operands contiguous at a.  Chunks of 16 values (four 16-B loads) one chunk ahead, then a tail of 4s.
__device__ __forceinline__ f32x4_ rec_mfma_rows(const float* a, const float* w, int KL, f32x4_ acc) {
    const f32x4_* w4 = reinterpret_cast<const f32x4_*>(w);
    const int K16 = KL & ~15;
    int s = 0;
    if (K16) {
        f32x4_ wn[4] = {w4[0], w4[1], w4[2], w4[3]};
#pragma unroll 1
        for (; s < K16; s += 16) {
            const f32x4_ wv[4] = {wn[0], wn[1], wn[2], wn[3]};
            if (s + 16 < K16) {
#pragma unroll
                for (int u = 0; u < 4; ++u) wn[u] = w4[(s + 16) / 4 + u];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s + u], wv[u >> 2][u & 3], acc, 0, 0, 0);
        }
    }
#pragma unroll 1
    for (; s < KL; s += 4) {
        const f32x4_ wv = w4[s / 4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s + u], wv[u], acc, 0, 0, 0);
    }
    return acc;
}

struct RecFwdArgs {
    float* gates;           // [ndir, B, T, G]: P (pre-activations incl. bias) on entry; GRU: activated z | r | c on exit (input time)
    const float* wp;        // packed weights of direction d at wp + d * wstride
    int64_t wstride, in;
    const float* h0;        // [ndir, B, H] or NULL (zeros)
    float* Y;               // [ndir, B, T, H]  h of step s at index s
    float* hprev;           // [ndir, B, T, H]  the h that met x[:, tau], at index tau
    float* hT;              // [ndir, B, H] or NULL; may alias h0
    unsigned* err;
    int B, T, H, Hp, nl, rnl;
};

// One workgroup = 16 batch rows of one direction, all T steps.  Wave w owns hidden tiles jt = w, w + 8, ... of ALL gates, so z, r, c
// and h_{t-1} of one (row, column) sit in the same lane (C/D map of 16x16x4: row = 4 (lane >> 4) + r, column = lane & 15).
// NG == 3 (GRU): phase A  z, r = rnl(P_zr + h_{t-1} [W_hz | W_hr]);  r * h_{t-1} -> LDS;  barrier;
//                phase B  c = nl(P_h + (r * h_{t-1}) W_hh);  h_t = z h_{t-1} + (1 - z) c -> the other h buffer;  barrier.
// NG == 1 (RNN): phase B alone with h_{t-1} as its operand:  h_t = nl(P + h_{t-1} W_h).
template <int NG, int MAXT>
__global__ __launch_bounds__(kRecThreads, 1) void rec_fwd_kernel(const RecFwdArgs a) {
    extern __shared__ float lds[];
    const int Hp = a.Hp, ldh = Hp + 4, G = NG * Hp, KS = Hp / 4, ntile = Hp / 16;
    if (rec_bad_shape<MAXT>(Hp, a.err, NNHIP_DEVERR_RECURRENT_SHAPE)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
    const int b0 = blockIdx.x * kRecRows, dir = blockIdx.y;
    const int64_t BT = (int64_t)a.B * a.T, BH = (int64_t)a.B * a.H;
    float* gates = a.gates + dir * BT * G;
    const float* whp = a.wp + dir * a.wstride + a.in * G;
    const float* h0 = a.h0 ? a.h0 + dir * BH : nullptr;
    float* Y = a.Y + dir * BT * a.H;
    float* hprev = a.hprev + dir * BT * a.H;
    float* hbuf[2] = {lds, lds + kRecRows * ldh};
    float* rh = lds + 2 * kRecRows * ldh;                            // NG == 3 only

    rec_stage_state(h0, a.B, a.H, Hp, ldh, b0, hbuf[0]);
    float hreg[MAXT][4];
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt) {
        const int j = (wave + tt * kRecWaves) * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + q * 4 + r;
            hreg[tt][r] = (h0 && b < a.B && j < a.H) ? h0[(int64_t)b * a.H + j] : 0.0f;
        }
    }
    __syncthreads();

    for (int s = 0; s < a.T; ++s) {
        const int tau = dir ? a.T - 1 - s : s;
        const float* hcur = hbuf[s & 1];
        float* hnext = hbuf[(s & 1) ^ 1];
        float zreg[MAXT][4], ph[MAXT][4];
#pragma unroll
        for (int tt = 0; tt < MAXT; ++tt) {
            const int jt = wave + tt * kRecWaves;
            if (jt < ntile) {                                         // wave-uniform
                const int j = jt * 16 + col;
                float pre[NG == 3 ? 2 : 1][4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int b = b0 + q * 4 + r;
                    const float* gp = gates + ((int64_t)b * a.T + tau) * G + j;
                    ph[tt][r] = b < a.B ? gp[(NG - 1) * Hp] : 0.0f;
                    if constexpr (NG == 3) {
                        pre[0][r] = b < a.B ? gp[0] : 0.0f;
                        pre[1][r] = b < a.B ? gp[Hp] : 0.0f;
                    }
                }
                if constexpr (NG == 3) {
                    f32x4_ acc[2] = {f32x4_{0.f, 0.f, 0.f, 0.f}, f32x4_{0.f, 0.f, 0.f, 0.f}};
                    rec_mfma_cols<2>(hcur + col * ldh + q * KS, whp + (int64_t)q * KS * G + j, G, Hp, KS, acc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = q * 4 + r, b = b0 + row;
                        const float z = rec_act(a.rnl, acc[0][r] + pre[0][r]);
                        const float rr = rec_act(a.rnl, acc[1][r] + pre[1][r]);
                        zreg[tt][r] = z;
                        rh[row * ldh + j] = rr * hreg[tt][r];
                        if (b < a.B) {
                            float* gp = gates + ((int64_t)b * a.T + tau) * G + j;
                            gp[0] = z;
                            gp[Hp] = rr;
                        }
                    }
                }
            }
        }
        if constexpr (NG == 3) __syncthreads();                       // r * h_{t-1} is complete
#pragma unroll
        for (int tt = 0; tt < MAXT; ++tt) {
            const int jt = wave + tt * kRecWaves;
            if (jt < ntile) {
                const int j = jt * 16 + col;
                f32x4_ acc[1] = {f32x4_{0.f, 0.f, 0.f, 0.f}};
                rec_mfma_cols<1>((NG == 3 ? rh : hcur) + col * ldh + q * KS, whp + (int64_t)q * KS * G + (NG - 1) * Hp + j, G, Hp, KS, acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = q * 4 + r, b = b0 + row;
                    const float c = rec_act(a.nl, acc[0][r] + ph[tt][r]);
                    float h = c;
                    if constexpr (NG == 3) {
                        h = zreg[tt][r] * hreg[tt][r] + (1.0f - zreg[tt][r]) * c;
                        if (b < a.B) gates[((int64_t)b * a.T + tau) * G + 2 * Hp + j] = c;
                    }
                    const bool v = b < a.B && j < a.H;
                    if (v) {
                        Y[((int64_t)b * a.T + s) * a.H + j] = h;
                        hprev[((int64_t)b * a.T + tau) * a.H + j] = hreg[tt][r];
                    }
                    hreg[tt][r] = v ? h : 0.0f;
                    hnext[row * ldh + j] = hreg[tt][r];
                }
            }
        }
        __syncthreads();
    }
    if (a.hT) {
        float* hT = a.hT + dir * BH;
#pragma unroll
        for (int tt = 0; tt < MAXT; ++tt) {
            const int j = (wave + tt * kRecWaves) * 16 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = b0 + q * 4 + r;
                if (b < a.B && j < a.H) hT[(int64_t)b * a.H + j] = hreg[tt][r];
            }
        }
    }
}

struct RecBwdArgs {
    const float* gates;     // GRU: [ndir, B, T, 3Hp] activated (input time).  RNN: Y [ndir, B, T, H] (step index)
    const float* hprev;     // [ndir, B, T, H] (input time)
    const float* wp;
    int64_t wstride, in;
    const float* dY;        // [ndir, B, T, H] (step index) or NULL
    const float* dYlast;    // [ndir, B, H] or NULL: gradient of the last step's h alone
    float* dG;              // [ndir, B, T, G] pre-activation gate gradients (input time; padded columns 0)
    float* rh;              // GRU: [ndir] blocks of rhstride floats, [B, T, H] each: r * h_{t-1}, the A operand of dW_hh
    int64_t rhstride;
    unsigned* err;
    int B, T, H, Hp, nl, rnl;
};

// BPTT, steps T-1 ... 0, the carried dh in registers; hd = dY_s (+ dYlast at the last step) + carry.
// NG == 3 (gru.py:66-110):  phase A  dc = hd (1 - z) nl'(c) -> LDS;  barrier;  tmp = dc W_hh^T;
//                           phase B  dr = tmp h_{t-1} rnl'(r),  dz = hd (h_{t-1} - c) rnl'(z) -> LDS;  barrier;
//                                    carry = [dz | dr] [W_hz | W_hr]^T + tmp r + hd z.
// NG == 1 (rnn.py:46-56):   ds = hd nl'(h_t) -> LDS;  barrier;  carry = ds W_h^T;  barrier.
// The MFMA outputs have the forward's (row, column) ownership, so a lane's saved values are those of its own accumulator elements.
template <int NG, int MAXT>
__global__ __launch_bounds__(kRecThreads, 1) void rec_bwd_kernel(const RecBwdArgs a) {
    extern __shared__ float lds[];
    const int Hp = a.Hp, G = NG * Hp, ldc = Hp + 4, ldz = 2 * Hp + 4, ntile = Hp / 16;
    if (rec_bad_shape<MAXT>(Hp, a.err, NNHIP_DEVERR_RECURRENT_SHAPE)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, col = lane & 15;
    const int b0 = blockIdx.x * kRecRows, dir = blockIdx.y;
    const int64_t BT = (int64_t)a.B * a.T;
    const float* gates = a.gates + dir * BT * (NG == 3 ? G : a.H);
    const float* hprev = a.hprev + dir * BT * a.H;
    const float* whp = a.wp + dir * a.wstride + a.in * G;
    const float* dY = a.dY ? a.dY + dir * BT * a.H : nullptr;
    const float* dYlast = a.dYlast ? a.dYlast + dir * (int64_t)a.B * a.H : nullptr;
    float* dG = a.dG + dir * BT * G;
    float* rh = NG == 3 ? a.rh + dir * a.rhstride : nullptr;
    float* dcb = lds;                                                 // 16 x (Hp + 4): dc_t (RNN: ds_t)
    float* dzr = lds + kRecRows * ldc;                               // 16 x (2Hp + 4): dz_t | dr_t (NG == 3 only)

    float carry[MAXT][4];
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[tt][r] = 0.0f;

    for (int s = a.T - 1; s >= 0; --s) {
        const int tau = dir ? a.T - 1 - s : s;
        float hdz[MAXT][4], rv[MAXT][4], fr[MAXT][4], dz[MAXT][4];    // what phase B needs of this lane's elements (NG == 3)
#pragma unroll
        for (int tt = 0; tt < MAXT; ++tt) {
            const int jt = wave + tt * kRecWaves;
            if (jt < ntile) {                                         // wave-uniform
                const int j = jt * 16 + col;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = q * 4 + r, b = b0 + row;
                    const bool v = b < a.B && j < a.H;
                    const int64_t bs = (int64_t)b * a.T + s, bt = (int64_t)b * a.T + tau;
                    float hd = carry[tt][r];
                    if (v && dY) hd += dY[bs * a.H + j];
                    if (v && dYlast && s == a.T - 1) hd += dYlast[(int64_t)b * a.H + j];
                    float dc;
                    if constexpr (NG == 3) {
                        const float* gp = gates + bt * G + j;
                        const float z = v ? gp[0] : 0.0f, rr = v ? gp[Hp] : 0.0f, c = v ? gp[2 * Hp] : 0.0f;
                        const float hp = v ? hprev[bt * a.H + j] : 0.0f;
                        dc = v ? hd * (1.0f - z) * rec_dact_y(a.nl, c) : 0.0f;
                        dz[tt][r] = v ? hd * (hp - c) * rec_dact_y(a.rnl, z) : 0.0f;
                        fr[tt][r] = hp * rec_dact_y(a.rnl, rr);
                        hdz[tt][r] = hd * z;
                        rv[tt][r] = rr;
                        if (v) rh[bt * a.H + j] = rr * hp;
                    } else {
                        const float h = v ? gates[bs * a.H + j] : 0.0f;
                        dc = v ? hd * rec_dact_y(a.nl, h) : 0.0f;
                    }
                    dcb[row * ldc + j] = dc;
                    if (b < a.B) dG[bt * G + (NG - 1) * Hp + j] = dc;
                }
            }
        }
        __syncthreads();                                              // dc_t is complete
        f32x4_ tmp[MAXT];
#pragma unroll
        for (int tt = 0; tt < MAXT; ++tt) {
            tmp[tt] = f32x4_{0.f, 0.f, 0.f, 0.f};
            const int jt = wave + tt * kRecWaves;
            if (jt < ntile && (NG == 3 || s > 0))                     // the RNN's product only feeds the next step's carry
                tmp[tt] = rec_mfma_rows(dcb + col * ldc + q * (Hp / 4), whp + (int64_t)(jt * 16 + col) * G + (NG - 1) * Hp + q * (Hp / 4), Hp / 4,
                                        tmp[tt]);
        }
        if constexpr (NG == 3) {
#pragma unroll
            for (int tt = 0; tt < MAXT; ++tt) {
                const int jt = wave + tt * kRecWaves;
                if (jt < ntile) {
                    const int j = jt * 16 + col;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = q * 4 + r, b = b0 + row;
                        const bool v = b < a.B && j < a.H;
                        const float dr = v ? tmp[tt][r] * fr[tt][r] : 0.0f;
                        dzr[row * ldz + j] = dz[tt][r];
                        dzr[row * ldz + Hp + j] = dr;
                        if (b < a.B) {
                            float* out = dG + ((int64_t)b * a.T + tau) * G + j;
                            out[0] = dz[tt][r];
                            out[Hp] = dr;
                        }
                    }
                }
            }
            __syncthreads();                                          // dz_t | dr_t is complete
#pragma unroll
            for (int tt = 0; tt < MAXT; ++tt) {
                const int jt = wave + tt * kRecWaves;
                if (jt < ntile) {
                    const int j = jt * 16 + col;
                    f32x4_ acc = f32x4_{0.f, 0.f, 0.f, 0.f};
                    if (s > 0) acc = rec_mfma_rows(dzr + col * ldz + q * (Hp / 2), whp + (int64_t)j * G + q * (Hp / 2), Hp / 2, acc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool v = b0 + q * 4 + r < a.B && j < a.H;
                        carry[tt][r] = v ? acc[r] + tmp[tt][r] * rv[tt][r] + hdz[tt][r] : 0.0f;
                    }
                }
            }
            // no barrier here: the next step writes dcb (last read before the barrier above) and, after its own first barrier, dzr
        } else {
#pragma unroll
            for (int tt = 0; tt < MAXT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool v = b0 + q * 4 + r < a.B && (wave + tt * kRecWaves) * 16 + col < a.H;
                    carry[tt][r] = v ? tmp[tt][r] : 0.0f;
                }
            __syncthreads();                                          // every wave is done reading ds_t
        }
    }
}

__global__ __launch_bounds__(256) void rec_add_kernel(float* __restrict__ x, const float* __restrict__ y, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] += y[i];
}

struct MergeArgs {
    const float* D;         // [rows, H]
    const float* R;
    const float* g;         // backward: the merged output's gradient, [rows, 2H] (concat) or [rows, H]
    float* out;             // forward: the merged output
    float* dD;              // backward: [rows, H] each
    float* dR;
    int64_t rows;
    int H, mode;
};

// bidirectional.py:89-103
__global__ __launch_bounds__(256) void bidir_merge_fwd_kernel(const MergeArgs a) {
    const int64_t n = a.rows * a.H;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = a.D[i], r = a.R[i];
        if (a.mode == NNHIP_MERGE_CONCAT) {
            const int64_t row = i / a.H;
            const int j = (int)(i - row * a.H);
            a.out[row * 2 * a.H + j] = d;
            a.out[row * 2 * a.H + a.H + j] = r;
        } else {
            a.out[i] = a.mode == NNHIP_MERGE_SUM ? d + r : a.mode == NNHIP_MERGE_MUL ? d * r : (d + r) / 2.0f;
        }
    }
}

// bidirectional.py:16-23
__global__ __launch_bounds__(256) void bidir_merge_bwd_kernel(const MergeArgs a) {
    const int64_t n = a.rows * a.H;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (a.mode == NNHIP_MERGE_CONCAT) {
            const int64_t row = i / a.H;
            const int j = (int)(i - row * a.H);
            a.dD[i] = a.g[row * 2 * a.H + j];
            a.dR[i] = a.g[row * 2 * a.H + a.H + j];
        } else if (a.mode == NNHIP_MERGE_MUL) {
            const float g = a.g[i];
            a.dD[i] = g * a.R[i];
            a.dR[i] = g * a.D[i];
        } else {
            const float g = a.mode == NNHIP_MERGE_SUM ? a.g[i] : a.g[i] / 2.0f;
            a.dD[i] = g;
            a.dR[i] = g;
        }
    }
}

static int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }

int rec_common_checks(const char* fn, const float* X, const RecWeights* w, int ng, int64_t B, int64_t T, int64_t in, int64_t H, int nl,
                      int rnl, int ndir) {
    NNHIP_CHECK_ARG(B >= 1 && T >= 1 && in >= 1 && H >= 1, NNHIP_EINVAL, "%s: sizes must be positive (B %lld, T %lld, in %lld, H %lld)", fn,
                    (long long)B, (long long)T, (long long)in, (long long)H);
    NNHIP_CHECK_ARG(ndir == 1 || ndir == 2, NNHIP_EINVAL, "%s: ndir must be 1 or 2, got %d", fn, ndir);
    NNHIP_CHECK_ARG(H <= kRecMaxH, NNHIP_EINVAL, "%s: hidden_size %lld > %d is not supported", fn, (long long)H, kRecMaxH);
    NNHIP_CHECK_ARG(ndir * B * T < ((int64_t)1 << 31) && in < ((int64_t)1 << 31), NNHIP_EINVAL, "%s: B*T or in_features too large", fn);
    NNHIP_CHECK_ARG(nl >= 0 && nl <= 2 && rnl >= 0 && rnl <= 2, NNHIP_EINVAL, "%s: bad nonlinearity code (%d, %d)", fn, nl, rnl);
    NNHIP_CHECK_ARG(X, NNHIP_EINVAL, "%s: null X / weights", fn);
    for (int d = 0; d < ndir; ++d)
        for (int g = 0; g < ng; ++g) {
            NNHIP_CHECK_ARG(w[d].wx[g] && w[d].wh[g], NNHIP_EINVAL, "%s: null weight %d of direction %d", fn, g, d);
            NNHIP_CHECK_ARG(aligned4(w[d].wx[g]) && aligned4(w[d].wh[g]) && aligned4(w[d].b[g]), NNHIP_EALIGN, "%s: misaligned weight", fn);
        }
    NNHIP_CHECK_ARG(aligned4(X), NNHIP_EALIGN, "%s: misaligned X", fn);
    return 0;
}

int rec_pack(const RecWeights* w, int ng, int ndir, int64_t in, int H, int Hp, size_t extra, hipStream_t st, float** out) {
    const int64_t G = (int64_t)ng * Hp, n = (in + Hp) * G + G;
    float* ws = static_cast<float*>(workspace_arena(2, (size_t)(ndir * n + extra) * sizeof(float)));
    if (!ws) {
        set_last_error("recurrent workspace allocation failed (%lld bytes)%s", (long long)((ndir * n + extra) * sizeof(float)),
                       workspace_locked() ? " -- the workspace is locked by a captured hipGraph" : "");
        return NNHIP_ENOMEM;
    }
    RecPack p;
    for (int d = 0; d < 2; ++d) p.w[d] = w[d < ndir ? d : 0];
    p.base = ws; p.stride = n; p.in = in; p.H = H; p.Hp = Hp; p.ng = ng;
    const int64_t blocks = std::min<int64_t>(ceil_div(n, 256), 1024);
    hipLaunchKernelGGL(rec_pack_kernel, dim3((unsigned)blocks, (unsigned)ndir), dim3(256), 0, st, p);
    NNHIP_LAUNCH_CHECK("rec_pack_kernel");
    *out = ws;
    return 0;
}

int rec_bwd_epilogue(const float* X, const float* ws, const float* dG, const float* hprev, const float* last_left, int64_t last_stride,
                     float* dX, float* dX1, const RecGrads* grads, int ng, int ndir, int64_t B, int64_t T, int64_t in, int64_t H, int Hp,
                     hipStream_t st) {
    const int64_t G = (int64_t)ng * Hp, BT = B * T, stride = (in + Hp) * G + G;
    int rc = 0;
    for (int d = 0; dX && d < ndir; ++d) {
        if ((rc = gemm_f32(dG + d * BT * G, ws + d * stride, d ? dX1 : dX, nullptr, nullptr, BT, in, G, G, G, in, true, true, 1, 0, 0, 0, 0, 1.0f, st)))
            return rc;
        if (d) {
            const int64_t n = BT * in;
            hipLaunchKernelGGL(rec_add_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(n, 256), 2048)), dim3(256), 0, st, dX, dX1, n);
            NNHIP_LAUNCH_CHECK("rec_add_kernel");
        }
    }
    for (int d = 0; grads && d < ndir; ++d) {
        const float* hp = hprev + d * BT * H;
        for (int g = 0; g < ng; ++g) {
            const float* dGg = dG + d * BT * G + (int64_t)g * Hp;
            const float* left = (last_left && g == ng - 1) ? last_left + d * last_stride : hp;
            if (grads[d].dwx[g] && (rc = gemm_f32(X, dGg, grads[d].dwx[g], nullptr, nullptr, in, H, BT, in, G, H, false, false, 1, 0, 0, 0, 0, 1.0f, st)))
                return rc;
            if (grads[d].dwh[g] && (rc = gemm_f32(left, dGg, grads[d].dwh[g], nullptr, nullptr, H, H, BT, H, G, H, false, false, 1, 0, 0, 0, 0, 1.0f, st)))
                return rc;
            if (grads[d].db[g] && (rc = colsum(dGg, BT, H, G, grads[d].db[g], st))) return rc;
        }
    }
    return 0;
}

// gates: GRU the caller's saved-gates buffer [ndir, B, T, 3Hp]; RNN NULL (P lives in the workspace: the activated value is Y itself)
template <int NG>
static int rec_forward(const char* fn, const float* X, const RecWeights* w, const float* h0, float* Y, float* gates, float* hprev, float* hT,
                       int64_t B, int64_t T, int64_t in, int64_t H, int nl, int rnl, int ndir, hipStream_t st) {
    if (int rc = rec_common_checks(fn, X, w, NG, B, T, in, H, nl, rnl, ndir)) return rc;
    NNHIP_CHECK_ARG(Y && hprev && (NG == 1 || gates), NNHIP_EINVAL, "%s: null output / saved-state buffer", fn);
    NNHIP_CHECK_ARG(aligned4(h0) && aligned4(Y) && aligned4(gates) && aligned4(hprev) && aligned4(hT), NNHIP_EALIGN,
                    "%s: misaligned state / output buffer", fn);
    const int Hp = (int)ceil_div(H, 16) * 16;
    const int64_t G = (int64_t)NG * Hp, BT = B * T, stride = (in + Hp) * G + G;
    float* ws = nullptr;
    int rc = rec_pack(w, NG, ndir, in, (int)H, Hp, NG == 1 ? (size_t)(ndir * BT * G) : 0, st, &ws);
    if (rc) return rc;
    float* P = NG == 1 ? ws + ndir * stride : gates;
    // P = X W_x + b of all B*T rows and every gate, one GEMM per direction; both read X in input order
    for (int d = 0; d < ndir; ++d) {
        const float* wd = ws + d * stride;
        rc = gemm_f32(X, wd, P + d * BT * G, wd + (in + Hp) * G, nullptr, BT, G, in, in, G, G, true, false, 1, 0, 0, 0, 0, 1.0f, st);
        if (rc) return rc;
    }
    RecFwdArgs a;
    a.gates = P; a.wp = ws; a.wstride = stride; a.in = in; a.h0 = h0; a.Y = Y; a.hprev = hprev; a.hT = hT;
    a.err = device_error_word();
    a.B = (int)B; a.T = (int)T; a.H = (int)H; a.Hp = Hp; a.nl = nl; a.rnl = rnl;
    const dim3 blocks((unsigned)ceil_div(B, kRecRows), (unsigned)ndir);
    const size_t lds = (size_t)(NG == 3 ? 3 : 2) * kRecRows * (Hp + 4) * sizeof(float);
    // no register-resident W_h tier (not measured)
    return rec_tiers(Hp, [&](auto mt) { return recurrence_run(rec_fwd_kernel<NG, decltype(mt)::value>, a, blocks, lds, st, "rec_fwd_kernel"); });
}

template <int NG>
static int rec_backward(const char* fn, const float* X, const RecWeights* w, const float* gates, const float* hprev, const float* dY,
                        const float* dYlast, float* dX, const RecGrads* grads, int64_t B, int64_t T, int64_t in, int64_t H, int nl, int rnl,
                        int ndir, hipStream_t st) {
    if (int rc = rec_common_checks(fn, X, w, NG, B, T, in, H, nl, rnl, ndir)) return rc;
    NNHIP_CHECK_ARG(gates && hprev, NNHIP_EINVAL, "%s: null saved-state buffer", fn);
    NNHIP_CHECK_ARG(dY || dYlast, NNHIP_EINVAL, "%s: null dY and dYlast", fn);
    NNHIP_CHECK_ARG(aligned4(gates) && aligned4(hprev) && aligned4(dY) && aligned4(dYlast) && aligned4(dX), NNHIP_EALIGN,
                    "%s: misaligned saved-state / gradient buffer", fn);
    for (int d = 0; grads && d < ndir; ++d)
        for (int g = 0; g < NG; ++g)
            NNHIP_CHECK_ARG(aligned4(grads[d].dwx[g]) && aligned4(grads[d].dwh[g]) && aligned4(grads[d].db[g]), NNHIP_EALIGN,
                            "%s: misaligned parameter gradient buffer", fn);
    const int Hp = (int)ceil_div(H, 16) * 16;
    const int64_t G = (int64_t)NG * Hp, BT = B * T, stride = (in + Hp) * G + G;
    const int64_t rhstride = NG == 3 ? round4(BT * H) : 0, ndx = (dX && ndir == 2) ? round4(BT * in) : 0;
    float* ws = nullptr;
    int rc = rec_pack(w, NG, ndir, in, (int)H, Hp, (size_t)(ndir * (BT * G + rhstride) + ndx), st, &ws);
    if (rc) return rc;
    float* dG = ws + ndir * stride;
    float* rh = dG + ndir * BT * G;
    float* dX1 = rh + ndir * rhstride;
    RecBwdArgs a;
    a.gates = gates; a.hprev = hprev; a.wp = ws; a.wstride = stride; a.in = in; a.dY = dY; a.dYlast = dYlast; a.dG = dG; a.rh = rh;
    a.rhstride = rhstride;
    a.err = device_error_word();
    a.B = (int)B; a.T = (int)T; a.H = (int)H; a.Hp = Hp; a.nl = nl; a.rnl = rnl;
    const dim3 blocks((unsigned)ceil_div(B, kRecRows), (unsigned)ndir);
    const size_t lds = (size_t)kRecRows * (NG == 3 ? 3 * Hp + 8 : Hp + 4) * sizeof(float);
    rc = rec_tiers(Hp, [&](auto mt) { return recurrence_run(rec_bwd_kernel<NG, decltype(mt)::value>, a, blocks, lds, st, "rec_bwd_kernel"); });
    if (rc) return rc;
    return rec_bwd_epilogue(X, ws, dG, hprev, NG == 3 ? rh : nullptr, rhstride, dX, dX1, grads, NG, ndir, B, T, in, H, Hp, st);
}

static void rec_from_gru(const nnhipGRUWeights* w, int ndir, RecWeights (&out)[2]) {
    for (int d = 0; d < 2; ++d) {
        const nnhipGRUWeights& s = w[d < ndir ? d : 0];
        out[d] = RecWeights{{s.wx[0], s.wx[1], s.wx[2]}, {s.wh[0], s.wh[1], s.wh[2]}, {s.b[0], s.b[1], s.b[2]}};
    }
}
static void rec_from_rnn(const nnhipRNNWeights* w, int ndir, RecWeights (&out)[2]) {
    for (int d = 0; d < 2; ++d) {
        const nnhipRNNWeights& s = w[d < ndir ? d : 0];
        out[d] = RecWeights{{s.wx, nullptr, nullptr}, {s.wh, nullptr, nullptr}, {s.b, nullptr, nullptr}};
    }
}

static int merge_checks(const char* fn, int64_t rows, int64_t H, int mode) {
    NNHIP_CHECK_ARG(rows >= 1 && H >= 1 && H < ((int64_t)1 << 30), NNHIP_EINVAL, "%s: sizes must be positive (rows %lld, H %lld)", fn,
                    (long long)rows, (long long)H);
    NNHIP_CHECK_ARG(mode >= NNHIP_MERGE_CONCAT && mode <= NNHIP_MERGE_AVG, NNHIP_EINVAL, "%s: bad merge mode %d", fn, mode);
    return 0;
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipGRUForward(const float* X, const nnhipGRUWeights* w, const float* h0, float* Y, float* gates, float* hprev, float* hT,
                               int64_t B, int64_t T, int64_t in, int64_t H, int nl, int rnl, int ndir, nnhipStream_t stream) {
    const char* fn = "nnhipGRUForward";
    NNHIP_CHECK_ARG(w, NNHIP_EINVAL, "%s: null X / weights", fn);
    NNHIP_CHECK_ARG(ndir == 1 || ndir == 2, NNHIP_EINVAL, "%s: ndir must be 1 or 2, got %d", fn, ndir);
    RecWeights rw[2];
    rec_from_gru(w, ndir, rw);
    return rec_forward<3>(fn, X, rw, h0, Y, gates, hprev, hT, B, T, in, H, nl, rnl, ndir, (hipStream_t)stream);
}

extern "C" int nnhipGRUBackward(const float* X, const nnhipGRUWeights* w, const float* gates, const float* hprev, const float* dY,
                                const float* dYlast, float* dX, const nnhipGRUGrads* grads, int64_t B, int64_t T, int64_t in, int64_t H,
                                int nl, int rnl, int ndir, nnhipStream_t stream) {
    const char* fn = "nnhipGRUBackward";
    NNHIP_CHECK_ARG(w, NNHIP_EINVAL, "%s: null X / weights", fn);
    NNHIP_CHECK_ARG(ndir == 1 || ndir == 2, NNHIP_EINVAL, "%s: ndir must be 1 or 2, got %d", fn, ndir);
    RecWeights rw[2];
    rec_from_gru(w, ndir, rw);
    RecGrads rg[2];
    for (int d = 0; grads && d < ndir; ++d)
        for (int g = 0; g < 3; ++g) { rg[d].dwx[g] = grads[d].dwx[g]; rg[d].dwh[g] = grads[d].dwh[g]; rg[d].db[g] = grads[d].db[g]; }
    return rec_backward<3>(fn, X, rw, gates, hprev, dY, dYlast, dX, grads ? rg : nullptr, B, T, in, H, nl, rnl, ndir, (hipStream_t)stream);
}

extern "C" int nnhipRNNForward(const float* X, const nnhipRNNWeights* w, const float* h0, float* Y, float* hprev, float* hT, int64_t B,
                               int64_t T, int64_t in, int64_t H, int nl, int ndir, nnhipStream_t stream) {
    const char* fn = "nnhipRNNForward";
    NNHIP_CHECK_ARG(w, NNHIP_EINVAL, "%s: null X / weights", fn);
    NNHIP_CHECK_ARG(ndir == 1 || ndir == 2, NNHIP_EINVAL, "%s: ndir must be 1 or 2, got %d", fn, ndir);
    RecWeights rw[2];
    rec_from_rnn(w, ndir, rw);
    return rec_forward<1>(fn, X, rw, h0, Y, nullptr, hprev, hT, B, T, in, H, nl, nl, ndir, (hipStream_t)stream);
}

extern "C" int nnhipRNNBackward(const float* X, const nnhipRNNWeights* w, const float* Y, const float* hprev, const float* dY,
                                const float* dYlast, float* dX, const nnhipRNNGrads* grads, int64_t B, int64_t T, int64_t in, int64_t H,
                                int nl, int ndir, nnhipStream_t stream) {
    const char* fn = "nnhipRNNBackward";
    NNHIP_CHECK_ARG(w, NNHIP_EINVAL, "%s: null X / weights", fn);
    NNHIP_CHECK_ARG(ndir == 1 || ndir == 2, NNHIP_EINVAL, "%s: ndir must be 1 or 2, got %d", fn, ndir);
    RecWeights rw[2];
    rec_from_rnn(w, ndir, rw);
    RecGrads rg[2];
    for (int d = 0; grads && d < ndir; ++d)
        rg[d] = RecGrads{{grads[d].dwx, nullptr, nullptr}, {grads[d].dwh, nullptr, nullptr}, {grads[d].db, nullptr, nullptr}};
    return rec_backward<1>(fn, X, rw, Y, hprev, dY, dYlast, dX, grads ? rg : nullptr, B, T, in, H, nl, nl, ndir, (hipStream_t)stream);
}

extern "C" int nnhipBidirectionalMergeForward(const float* D, const float* R, float* out, int64_t rows, int64_t H, int mode,
                                              nnhipStream_t stream) {
    const char* fn = "nnhipBidirectionalMergeForward";
    if (int rc = merge_checks(fn, rows, H, mode)) return rc;
    NNHIP_CHECK_ARG(D && R && out, NNHIP_EINVAL, "%s: null buffer", fn);
    NNHIP_CHECK_ARG(aligned4(D) && aligned4(R) && aligned4(out), NNHIP_EALIGN, "%s: misaligned buffer", fn);
    MergeArgs a{D, R, nullptr, out, nullptr, nullptr, rows, (int)H, mode};
    const int64_t blocks = std::min<int64_t>(ceil_div(rows * H, 256), 2048);
    hipLaunchKernelGGL(bidir_merge_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    NNHIP_LAUNCH_CHECK("bidir_merge_fwd_kernel");
    return 0;
}

extern "C" int nnhipBidirectionalMergeBackward(const float* grad, const float* D, const float* R, float* dD, float* dR, int64_t rows,
                                               int64_t H, int mode, nnhipStream_t stream) {
    const char* fn = "nnhipBidirectionalMergeBackward";
    if (int rc = merge_checks(fn, rows, H, mode)) return rc;
    NNHIP_CHECK_ARG(grad && dD && dR && (mode != NNHIP_MERGE_MUL || (D && R)), NNHIP_EINVAL, "%s: null buffer", fn);
    NNHIP_CHECK_ARG(aligned4(grad) && aligned4(D) && aligned4(R) && aligned4(dD) && aligned4(dR), NNHIP_EALIGN, "%s: misaligned buffer", fn);
    MergeArgs a{D, R, grad, nullptr, dD, dR, rows, (int)H, mode};
    const int64_t blocks = std::min<int64_t>(ceil_div(rows * H, 256), 2048);
    hipLaunchKernelGGL(bidir_merge_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    NNHIP_LAUNCH_CHECK("bidir_merge_bwd_kernel");
    return 0;
}
