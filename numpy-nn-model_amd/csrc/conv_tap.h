// conv_tap.h -- the device-side pipeline that the implicit-GEMM conv kernels share: conv_mfma.hip (Conv2d forward / dgrad / wgrad)
// and conv_transpose.hip (the stride-phase ConvTranspose2d forward).  Buffer-descriptor loads, the pinned issue order of a k-step,
// the 64x64 wave-tile store, and the tap-outermost k-step of the forward / dgrad family.
#pragma once
#include "conv_common.h"
#include "gemm_common.h"

namespace nnhip {

constexpr unsigned CV_SENT = 0x80000000u;   // vector offset of an element that does not exist: past num_records (< 2 GiB) -> reads 0

__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_rsrc(const float* base, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float bload1(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0));
}
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
    const u32x4_ t = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    return make_float4(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w));
}

// One k-step's issue order (gemm.hip, gemm_k_step): the tile's NLD loads ride one per MFMA under the first MFMAs, its NDW LDS
// stores under the last; with fewer MFMAs than slots the last slot of each phase takes the rest.
template <int MASK, int CNT>
__device__ __forceinline__ void conv_sgb() { __builtin_amdgcn_sched_group_barrier(MASK, CNT, 0); }   // (the builtin wants literal constants)
template <int I, int N, int MASK, int LASTCNT>
__device__ __forceinline__ void conv_pin_pairs() {                       // N x { 1 MFMA, 1 MASK-instruction }, the last pair takes LASTCNT
    if constexpr (I < N) {
        conv_sgb<0x008, 1>();
        conv_sgb<MASK, (I == N - 1 ? LASTCNT : 1)>();
        conv_pin_pairs<I + 1, N, MASK, LASTCNT>();
    }
}
template <int NMF, int NLD, int NDW>
__device__ __forceinline__ void conv_pin_pipeline() {
    constexpr int N1 = NLD < NMF / 2 ? NLD : NMF / 2;
    constexpr int N2 = NDW < NMF - N1 ? NDW : NMF - N1;
    conv_pin_pairs<0, N1, 0x020, NLD - N1 + 1>();                          // VMEM reads
    if constexpr (NMF - N1 - N2 > 0) conv_sgb<0x008, NMF - N1 - N2>();
    conv_pin_pairs<0, N2, 0x200, NDW - N2 + 1>();                          // DS writes
}

// Each wave's 64x64 result tile -> rows of float4 through its own LDS region (gemm_common.h, gemm_epilogue: a lane owns a strided
// COLUMN of an MFMA accumulator; direct stores are 4x the instructions).  store(row_in_tile, col4_in_tile, float4)
template <class Store>
__device__ __forceinline__ void conv_store_tile(f32x16 (&acc)[2][2], float* __restrict__ smem, int wave, int lane, int l31, int lh,
                                                Store&& store) {
    constexpr int ELD = 68;
    float* E = smem + wave * (32 * ELD);
    const int er = lane >> 4, ec = (lane & 15) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) E[((e & 3) + 8 * (e >> 2) + 4 * lh) * ELD + n * 32 + l31] = acc[i][n][e];
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0); E is private to the wave
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int rl = it * 4 + er;
            store(i * 32 + rl, ec, *reinterpret_cast<const float4*>(&E[rl * ELD + ec]));
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
    }
}

template <int WM>
struct TapCfg {
    static constexpr int WN = 4 / WM, BM = 64 * WM, BN = 64 * WN, BK = WM == 2 ? 32 : 16;
    static constexpr int ALD = BK + 4, NVA = BM * BK / 1024, KPT = 16;      // KPT: source channels per thread per tile
    // both tiles k-major, rows of BK + 4 floats (conflict-free 16-byte LDS accesses with lane = row): a thread's 16 gathered
    // channels of one pixel are 16 consecutive k of one B row -- four ds_write_b128 -- and the MFMA fragments are ds_read_b128
    static constexpr int A_SIZE = BM * ALD, B_SIZE = BN * ALD, STAGE = A_SIZE + B_SIZE;
    static constexpr int NMF = 16 * (BK / 8), NLD = NVA + KPT, NDW = NVA + KPT / 4;
    static constexpr size_t LDS = (size_t)2 * STAGE * sizeof(float);
};

template <int WM>
__device__ __forceinline__ void tap_k_step(f32x16 (&acc)[2][2], float4 (&fa)[TapCfg<WM>::NVA], float (&fb)[16],
                                           const float4 (&ca)[TapCfg<WM>::NVA], const float (&cb)[16], float* __restrict__ smem, int cur,
                                           __amdgpu_buffer_rsrc_t rsA, __amdgpu_buffer_rsrc_t rsB, const unsigned (&voffA)[TapCfg<WM>::NVA],
                                           unsigned soffA, unsigned voffB, int cbase, int Cs, unsigned HWs4,
                                           const int (&sA)[TapCfg<WM>::NVA], int sB, int wm, int wn, int l31, int lh) {
    using C = TapCfg<WM>;
    // ---- fetch (tile t+2) --------------------------------------------------------------------------------------------------
#pragma unroll
    for (int p = 0; p < C::NVA; ++p) fa[p] = bload4(rsA, voffA[p], soffA);
#pragma unroll
    for (int j = 0; j < C::KPT; ++j) {
        const int c = cbase + j;                                         // uniform
        fb[j] = bload1(rsB, c < Cs ? voffB : CV_SENT, (unsigned)c * HWs4);
    }
    // ---- multiply (tile t, LDS stage cur) ----------------------------------------------------------------------------------
    const float* As = smem + cur * C::STAGE;
    const float* Bs = As + C::A_SIZE;
#pragma unroll
    for (int g = 0; g < C::BK / 8; ++g) {
        float a[2][4], b[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float4 v = *reinterpret_cast<const float4*>(&As[(wm * 64 + i * 32 + l31) * C::ALD + g * 8 + lh * 4]);
            a[i][0] = v.x; a[i][1] = v.y; a[i][2] = v.z; a[i][3] = v.w;
            const float4 w = *reinterpret_cast<const float4*>(&Bs[(wn * 64 + i * 32 + l31) * C::ALD + g * 8 + lh * 4]);
            b[i][0] = w.x; b[i][1] = w.y; b[i][2] = w.z; b[i][3] = w.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][j], b[n][j], acc[i][n], 0, 0, 0);
    }
    // ---- commit (tile t+1 -> the other stage) ------------------------------------------------------------------------------
    float* An = smem + (cur ^ 1) * C::STAGE;
    float* Bn = An + C::A_SIZE;
#pragma unroll
    for (int p = 0; p < C::NVA; ++p) *reinterpret_cast<float4*>(&An[sA[p]]) = ca[p];
#pragma unroll
    for (int j = 0; j < C::KPT; j += 4) *reinterpret_cast<float4*>(&Bn[sB + j]) = make_float4(cb[j], cb[j + 1], cb[j + 2], cb[j + 3]);
    conv_pin_pipeline<C::NMF, C::NLD, C::NDW>();
    __syncthreads();
}

}  // namespace nnhip
