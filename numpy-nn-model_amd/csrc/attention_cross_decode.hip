// attention_cross_decode.hip -- one query row per (batch row, head) against a READ-ONLY encoder memory (ABI 217, net-new: the
// reference's predict() re-runs the whole decoder over the prefix for every token, examples/seq2seq.ipynb cell 17; this is the
// cross-attention of cell 5 for the one new row of a cached step, with the attention map cell 21 plots).
//
// What differs from attention_decode.hip, whose lane layout it reuses (attention_decode.h: LPK lanes per key with float4 loads, a
// DPP row reduction for the score, per-slot online softmax, an LDS merge in slot order):
//   * nothing is appended: Kmem / Vmem [B, H, S, dh] are only read, and the query is a plain [B, D] row, not a q|k|v row;
//   * the length notion is a key_valid mask (source padding, holes allowed), with the masked-softmax entry points' rule: a
//     masked key scores -1e9, not -inf, so a fully masked row is the plain average of all S values;
//   * P (optional) receives the softmax probabilities [B, H, S]: the lane that owns a key writes its raw score where the
//     probability goes, and after the merge THE SAME lane normalises what it wrote -- no thread reads another's store;
//   * ONE launch, no workspace, no atomics: one block per (b, h) loops over the keys, KPI = 128 (dh 32) / 64 (dh 64, 128) per
//     iteration, and folds its slots in a fixed order, so reruns are bit-identical.
//
// No key split: source sentences have tens of keys and B*H blocks of one or two iterations each are what the chip gets.  A long
// memory with a small B*H is therefore slow BY CONSTRUCTION (one block streams all 2*S*dh*4 bytes of a head); a split plan as in
// attention_decode.hip is out of scope here (DESIGN.md has the numbers).
#include "attention_decode.h"

namespace nnhip {

constexpr float kMaskedScore = -1e9f;        // nnhipMaskedSoftmaxForward's fill value (the notebook's where(mask == 0, -1e9, scores))

// grid B*H, 256 threads
template <int DH>
__global__ __launch_bounds__(DEC_THREADS) void attn_cross_decode_kernel(
    const float* __restrict__ Q, const float* __restrict__ Km, const float* __restrict__ Vm, const int32_t* __restrict__ key_valid,
    float* __restrict__ O, float* P, int H, int S, int64_t ld_q, float scale_log2e) {
    using L = DecLanes<DH>;
    constexpr int LPK = L::LPK, NV = L::NV, KPW = L::KPW, NSLOT = L::NSLOT, KPI = L::KPI;
    __shared__ float s_m[NSLOT], s_l[NSLOT];
    __shared__ __attribute__((aligned(16))) float s_o[NSLOT][DH + 4];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int D = H * DH;
    const float* qrow = Q + (int64_t)b * ld_q + h * DH;
    const float* Kh = Km + (int64_t)bh * S * DH;
    const float* Vh = Vm + (int64_t)bh * S * DH;
    const int32_t* valid = key_valid ? key_valid + (int64_t)b * S : nullptr;
    float* Ph = P ? P + (int64_t)bh * S : nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPK, c = (lane % LPK) * 4;      // key slot in the wave, first column of this lane
    const bool leader = lane % LPK == 0;                 // the lane that writes (and later normalises) its key's entry of P
    const float masked = kMaskedScore * kLog2e;          // scores live in the log2 domain
    dec_f4 q[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) q[v] = *reinterpret_cast<const dec_f4*>(qrow + c + v * 4 * LPK) * scale_log2e;
    float m = -INFINITY, l = 0.f;
    dec_f4 o[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) o[v] = dec_f4{0.f, 0.f, 0.f, 0.f};
    // key of (iteration base kb, unroll u, slot g): kb + (wave * U + u) * KPW + g, as in attn_decode_kernel
    for (int kb = 0; kb < S; kb += KPI) {
        dec_f4 kk[DEC_U][NV], vv[DEC_U][NV];
        bool ok[DEC_U], live[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int key = kb + (wave * DEC_U + u) * KPW + g;
            ok[u] = key < S;
            live[u] = ok[u] && (!valid || valid[key] != 0);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                if (ok[u]) {
                    kk[u][v] = *reinterpret_cast<const dec_f4*>(Kh + (int64_t)key * DH + c + v * 4 * LPK);
                    vv[u][v] = *reinterpret_cast<const dec_f4*>(Vh + (int64_t)key * DH + c + v * 4 * LPK);
                } else {
                    kk[u][v] = vv[u][v] = dec_f4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const float d = group_sum<LPK>(dec_dot<NV>(q, kk[u]));     // wave-converged: every lane takes part, live key or not
            const float sc = ok[u] ? (live[u] ? d : masked) : -INFINITY;
            if (Ph && leader && ok[u]) Ph[kb + (wave * DEC_U + u) * KPW + g] = sc;
            dec_online_step<NV>(sc, ok[u], vv[u], m, l, o);
        }
    }
    // ---- the block's NSLOT states -> one (m, l, o[DH]), folded in slot order ----------------------------------------
    const int slot = wave * KPW + g;
    if (leader) { s_m[slot] = m; s_l[slot] = l; }
#pragma unroll
    for (int v = 0; v < NV; ++v) *reinterpret_cast<dec_f4*>(&s_o[slot][c + v * 4 * LPK]) = o[v];
    __syncthreads();
    // every thread folds (M, L) itself, in the same order: the same bits everywhere, no second barrier
    float M = s_m[0];
#pragma unroll
    for (int s = 1; s < NSLOT; ++s) M = fmaxf(M, s_m[s]);             // finite: slot 0 of wave 0 always holds key 0 (S >= 1)
    float Lsum = 0.f;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) Lsum += s_l[s] * __builtin_amdgcn_exp2f(s_m[s] - M);   // exp2(-inf) = 0 for a slot without a key
    if (threadIdx.x < DH) {
        const int t = threadIdx.x;
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) acc += s_o[s][t] * __builtin_amdgcn_exp2f(s_m[s] - M);
        O[(int64_t)b * D + h * DH + t] = acc / Lsum;
    }
    if (Ph && leader) {                                               // raw scores -> probabilities, each lane its own entries
        for (int kb = 0; kb < S; kb += KPI) {
#pragma unroll
            for (int u = 0; u < DEC_U; ++u) {
                const int key = kb + (wave * DEC_U + u) * KPW + g;
                if (key < S) Ph[key] = __builtin_amdgcn_exp2f(Ph[key] - M) / Lsum;
            }
        }
    }
}

// Token-major projections K, V [B, S, D] (row stride ld) -> the head-major memories [B, H, S, dh].  One float4 per thread and tensor.
__global__ __launch_bounds__(256) void kv_memory_fill_kernel(const float* __restrict__ K, const float* __restrict__ V,
                                                             float* __restrict__ Km, float* __restrict__ Vm, int64_t total, int H,
                                                             int S, int dh, int64_t ld) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int q4 = dh >> 2;
    const int c = (int)(i % q4) * 4;
    int64_t r = i / q4;
    const int h = (int)(r % H); r /= H;
    const int tok = (int)(r % S);
    const int b = (int)(r / S);
    const int64_t src = ((int64_t)b * S + tok) * ld + h * dh + c;
    const int64_t dst = (((int64_t)b * H + h) * S + tok) * dh + c;
    *reinterpret_cast<dec_f4*>(Km + dst) = *reinterpret_cast<const dec_f4*>(K + src);
    *reinterpret_cast<dec_f4*>(Vm + dst) = *reinterpret_cast<const dec_f4*>(V + src);
}

// The status rules both exports share; *launch = false for an empty batch.
static int cross_check(const char* fn, int64_t B, int64_t H, int64_t S, int64_t dh, int64_t ld, const char* ld_name, const void* a,
                       const void* b, const void* c, const void* d, bool* launch) {
    *launch = false;
    NNHIP_CHECK_ARG(B >= 0 && H >= 0 && S >= 0, NNHIP_EINVAL, "%s: negative size", fn);
    NNHIP_CHECK_ARG(dh == 32 || dh == 64 || dh == 128, NNHIP_EINVAL, "%s: unsupported head dim %lld (32, 64 or 128)", fn, (long long)dh);
    if (B == 0) return 0;
    NNHIP_CHECK_ARG(H >= 1 && S >= 1, NNHIP_EINVAL, "%s: H and S must be >= 1", fn);
    NNHIP_CHECK_ARG(B * H < ((int64_t)1 << 31) && S < ((int64_t)1 << 30) && H * dh < ((int64_t)1 << 30) && B * S < ((int64_t)1 << 31),
                    NNHIP_EINVAL, "%s: size out of range (B*H < 2^31, B*S < 2^31, S < 2^30)", fn);
    NNHIP_CHECK_ARG(a && b && c && d, NNHIP_EINVAL, "%s: null pointer", fn);
    NNHIP_CHECK_ARG(ld >= H * dh && ld % 4 == 0, NNHIP_EINVAL, "%s: %s must be >= H * head_dim and a multiple of 4", fn, ld_name);
    NNHIP_CHECK_ARG(aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d), NNHIP_EALIGN, "%s: operands must be 16-byte aligned", fn);
    *launch = true;
    return 0;
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipAttentionDecodeCross(const float* Q, const float* Kmem, const float* Vmem, const int32_t* key_valid, float* O,
                                         float* P, int64_t B, int64_t H, int64_t S, int64_t head_dim, int64_t ld_q, float scale,
                                         nnhipStream_t s) {
    bool launch;
    if (int rc = cross_check("nnhipAttentionDecodeCross", B, H, S, head_dim, ld_q, "ld_q", Q, Kmem, Vmem, O, &launch)) return rc;
    if (!launch) return 0;
    NNHIP_CHECK_ARG(aligned4(key_valid) && aligned4(P), NNHIP_EALIGN, "nnhipAttentionDecodeCross: key_valid / P must be 4-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const float sl2 = scale * kLog2e;
#define XDEC(DH_)                                                                                                                \
    do {                                                                                                                         \
        hipLaunchKernelGGL(attn_cross_decode_kernel<DH_>, dim3((unsigned)(B * H)), dim3(DEC_THREADS), 0, st, Q, Kmem, Vmem,      \
                           key_valid, O, P, (int)H, (int)S, ld_q, sl2);                                                          \
        NNHIP_LAUNCH_CHECK("attn_cross_decode_kernel");                                                                          \
    } while (0)
    if (head_dim == 32) XDEC(32);
    else if (head_dim == 64) XDEC(64);
    else XDEC(128);
#undef XDEC
    return 0;
}

extern "C" int nnhipKVMemoryFill(const float* K, const float* V, float* Kmem, float* Vmem, int64_t B, int64_t H, int64_t S,
                                 int64_t head_dim, int64_t ld, nnhipStream_t s) {
    bool launch;
    if (int rc = cross_check("nnhipKVMemoryFill", B, H, S, head_dim, ld, "ld", K, V, Kmem, Vmem, &launch)) return rc;
    if (!launch) return 0;
    const int64_t total = B * S * H * (head_dim / 4);
    NNHIP_CHECK_ARG(ceil_div(total, 256) < ((int64_t)1 << 31), NNHIP_EINVAL, "nnhipKVMemoryFill: size out of range");
    hipLaunchKernelGGL(kv_memory_fill_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)s, K, V, Kmem, Vmem,
                       total, (int)H, (int)S, (int)head_dim, ld);
    NNHIP_LAUNCH_CHECK("kv_memory_fill_kernel");
    return 0;
}
