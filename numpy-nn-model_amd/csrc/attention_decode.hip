// attention_decode.hip -- KV-cached single-token attention for incremental decoding (ABI 212, net-new: the reference's
// generate() re-runs the whole prefix for every token, examples/gpt2/gpt2_infer.py:318-350).
//
// One query row per (batch row, head) against that head's cached keys and values.  2 * t * dh * 4 bytes are read per
// (b, h) and nothing is reused: HBM-bound VALU work, no MFMA to feed.  What decides the speed is how many bytes are in
// flight, so:
//
//   * Cache layout: HEAD-MAJOR, K and V each [B, H, Tmax, dh] fp32.  A head's keys are then one contiguous stream and a
//     wave load of 64 lanes x 16 B covers 1 KiB = 8 whole 128-B lines (dh 64: 4 complete keys; dh 32: 8; dh 128: 2 x 2).
//     In the token-major layout of the fused projection ([B, T, 3D]) the same load would touch one 256-B piece in each of
//     four rows 3D floats apart -- the strided layout DESIGN.md 5 measured 8-9 % behind head-major for the training kernels.
//   * Lanes: LPK = min(16, dh/4) adjacent lanes own one key (a float4 each, two for dh 128), so a wave works on
//     KPW = 64/LPK keys at once and a score is a DPP reduction inside a 16-lane row: no LDS, no cross-row traffic.
//     Every key slot of every wave keeps its OWN online-softmax state (m, l, o[dh] spread over its LPK lanes): the inner
//     loop has no communication between slots at all.
//   * Unroll: U = 4 key groups per wave and iteration -- 8 (dh 128: 16) independent 1-KiB loads in flight per wave before
//     the first use, 4 waves per block, several blocks per CU.
//   * Split: the key range of a (b, h) is cut into `splits` chunks of `chunk` keys (a multiple of 64 = one block pass), one
//     block each, so that B*H*splits approaches the chip's 256 CUs when B*H is small (GPT-2 small, batch 1: 12 heads x 16 splits = 192 blocks).
//     The plan depends on (B, H, Tmax) only -- never on the device-side lengths -- so the launch can sit in a captured graph.
//   * Merge: the 4*KPW slot states of a block meet in LDS and are folded in slot order; the block writes its partial
//     (m, l, o[dh]) to the workspace; a second launch folds the partials of the live splits in split order.  Fixed orders
//     everywhere: the output is bit-identical from run to run.  (One split: the block writes O itself, no second launch.)
//
// The new token's k and v are appended by the split-0 block of each (b, h) at index cache_len[b]; every block reads that
// key from the qkv row, not from the cache, so no block reads what another one writes in the same launch.  cache_len is
// a device int32[B] that this kernel only reads (rows of a batch may differ; the host advances it with its own op).
// A row with cache_len[b] outside 0 .. Tmax-1 raises the device error word and is skipped: nothing of that row is written.
#include "attention_decode.h"      // the lane layout, shared with attention_cross_decode.hip

namespace nnhip {

struct DecodePlan { int splits; int chunk; };
// chunk: a multiple of DEC_PASS keys; splits * chunk >= Tmax.  Asks for 1024 blocks (4 per CU of a 256-CU part) and gets fewer
// when B*H is small, because a chunk is never shorter than one 64-key block pass: GPT-2 small at batch 1 with Tmax 1024 is
// 12 x 16 = 192 blocks of one loop iteration each, and since the plan is fixed by Tmax (not by the device-side length) only the
// splits below the live length do work -- 24 blocks at t = 128.  At batch 1 the call is launch- and latency-bound either way
// (EXPERIMENTS 5.10 has the times); shorter chunks would add merge work for the same DRAM round trip.
static DecodePlan decode_plan(int64_t B, int64_t H, int64_t Tmax) {
    const int64_t bh = B * H > 0 ? B * H : 1;
    int64_t want = ceil_div(1024, bh);
    const int64_t most = ceil_div(Tmax, DEC_PASS);
    if (want > most) want = most;
    if (want < 1) want = 1;
    if (want > 64) want = 64;
    int64_t chunk = ceil_div(ceil_div(Tmax, want), DEC_PASS) * DEC_PASS;
    if (chunk < DEC_PASS) chunk = DEC_PASS;
    return DecodePlan{(int)ceil_div(Tmax, chunk), (int)chunk};
}

// grid (splits, B*H), 256 threads.  part: [B*H][splits][DH + 2] = (m, l, o[DH]), m in the log2 domain.
template <int DH>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_kernel(
    const float* __restrict__ qkv, float* __restrict__ Kc, float* __restrict__ Vc, const int32_t* __restrict__ cache_len,
    float* __restrict__ O, float* __restrict__ part, int H, int Tmax, int64_t ld, float scale_log2e, int chunk, unsigned* err) {
    using L = DecLanes<DH>;
    constexpr int LPK = L::LPK, NV = L::NV, KPW = L::KPW, NSLOT = L::NSLOT;
    __shared__ float s_m[NSLOT], s_l[NSLOT];
    __shared__ __attribute__((aligned(16))) float s_o[NSLOT][DH + 4];
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int split = blockIdx.x, nsplit = gridDim.x;
    const int pos = ld_dev_i32(cache_len + b);           // tokens already cached = index of the new one
    if (pos < 0 || pos >= Tmax) {                        // no room: refuse the row (block-uniform)
        if (threadIdx.x == 0 && err) __hip_atomic_store(err, (unsigned)NNHIP_DEVERR_KVCACHE_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int n = pos + 1;                               // keys 0 .. pos
    const int D = H * DH;
    const float* qrow = qkv + (int64_t)b * ld + h * DH;
    const float* knew = qrow + D;
    const float* vnew = qrow + 2 * D;
    float* Kh = Kc + (int64_t)bh * Tmax * DH;
    float* Vh = Vc + (int64_t)bh * Tmax * DH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / LPK, c = (lane % LPK) * 4;      // key slot in the wave, first column of this lane
    if (split == 0 && threadIdx.x < DH / 4) {            // append the new token (read below from qkv, never from the cache)
        const int cc = threadIdx.x * 4;
        *reinterpret_cast<dec_f4*>(Kh + (int64_t)pos * DH + cc) = *reinterpret_cast<const dec_f4*>(knew + cc);
        *reinterpret_cast<dec_f4*>(Vh + (int64_t)pos * DH + cc) = *reinterpret_cast<const dec_f4*>(vnew + cc);
    }
    const int k0 = split * chunk;
    const int k1 = min(n, k0 + chunk);
    if (k0 >= n) return;                                 // a split past the live length (block-uniform): the merge skips it too
    dec_f4 q[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) q[v] = *reinterpret_cast<const dec_f4*>(qrow + c + v * 4 * LPK) * scale_log2e;
    float m = -INFINITY, l = 0.f;
    dec_f4 o[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) o[v] = dec_f4{0.f, 0.f, 0.f, 0.f};
    // key of (iteration base kb, unroll u, slot g): kb + (wave * U + u) * KPW + g -- a wave's U loads are 1 KiB each, back to back
    for (int kb = k0; kb < k1; kb += DEC_WAVES * DEC_U * KPW) {
        dec_f4 kk[DEC_U][NV], vv[DEC_U][NV];
        bool ok[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int key = kb + (wave * DEC_U + u) * KPW + g;
            ok[u] = key < k1;
            const float* kp = key == pos ? knew : Kh + (int64_t)key * DH;
            const float* vp = key == pos ? vnew : Vh + (int64_t)key * DH;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                if (ok[u]) {
                    kk[u][v] = *reinterpret_cast<const dec_f4*>(kp + c + v * 4 * LPK);
                    vv[u][v] = *reinterpret_cast<const dec_f4*>(vp + c + v * 4 * LPK);
                } else {
                    kk[u][v] = vv[u][v] = dec_f4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const float d = group_sum<LPK>(dec_dot<NV>(q, kk[u]));     // wave-converged: every lane takes part, live key or not
            dec_online_step<NV>(ok[u] ? d : -INFINITY, ok[u], vv[u], m, l, o);
        }
    }
    // ---- the block's NSLOT states -> one (m, l, o[DH]), folded in slot order ----------------------------------------
    const int slot = wave * KPW + g;
    if (lane % LPK == 0) { s_m[slot] = m; s_l[slot] = l; }
#pragma unroll
    for (int v = 0; v < NV; ++v) *reinterpret_cast<dec_f4*>(&s_o[slot][c + v * 4 * LPK]) = o[v];
    __syncthreads();
    if (threadIdx.x < DH) {
        const int t = threadIdx.x;
        float M = s_m[0];
#pragma unroll
        for (int s = 1; s < NSLOT; ++s) M = fmaxf(M, s_m[s]);         // finite: slot 0 of wave 0 always holds key k0 < n
        float L = 0.f, acc = 0.f;
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            const float w = __builtin_amdgcn_exp2f(s_m[s] - M);       // exp2(-inf) = 0 for a slot that saw no key
            L += s_l[s] * w;
            acc += s_o[s][t] * w;
        }
        if (nsplit == 1) {
            O[(int64_t)b * D + h * DH + t] = acc / L;
        } else {
            float* pp = part + ((int64_t)bh * nsplit + split) * (DH + 2);
            if (t == 0) { pp[0] = M; pp[1] = L; }
            pp[2 + t] = acc;
        }
    }
}

// grid B*H, max(DH, 64) threads: O = the partials of the live splits, folded in split order
template <int DH>
__global__ __launch_bounds__(DH < 64 ? 64 : DH) void attn_decode_merge_kernel(
    const float* __restrict__ part, const int32_t* __restrict__ cache_len, float* __restrict__ O, int H, int Tmax, int chunk, int nsplit) {
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int t = threadIdx.x;
    const int pos = ld_dev_i32(cache_len + b);
    if (pos < 0 || pos >= Tmax || t >= DH) return;       // (a refused row: attn_decode_kernel raised the error word)
    const int live = pos / chunk + 1;                    // splits with k0 < n = pos + 1
    const float* pp = part + (int64_t)bh * nsplit * (DH + 2);
    float M = pp[0];
    for (int s = 1; s < live; ++s) M = fmaxf(M, pp[s * (DH + 2)]);
    float L = 0.f, acc = 0.f;
    for (int s = 0; s < live; ++s) {
        const float w = __builtin_amdgcn_exp2f(pp[s * (DH + 2)] - M);
        L += pp[s * (DH + 2) + 1] * w;
        acc += pp[s * (DH + 2) + 2 + t] * w;
    }
    O[(int64_t)b * H * DH + h * DH + t] = acc / L;
}

// Prefill: k and v of T tokens out of the fused projection [B, T, 3D] (row stride ld) into the head-major cache at token
// index start(b) + i, start = cache_len[b] (or 0 without cache_len).  One float4 per thread and tensor.
__global__ __launch_bounds__(256) void kv_cache_fill_kernel(const float* __restrict__ qkv, float* __restrict__ Kc, float* __restrict__ Vc,
                                                            const int32_t* __restrict__ cache_len, int64_t total, int H, int T,
                                                            int Tmax, int dh, int64_t ld, unsigned* err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int q4 = dh >> 2;
    const int c = (int)(i % q4) * 4;
    int64_t r = i / q4;
    const int h = (int)(r % H); r /= H;
    const int tok = (int)(r % T);
    const int b = (int)(r / T);
    const int start = cache_len ? ld_dev_i32(cache_len + b) : 0;
    if (start < 0 || start > Tmax - T) {
        if (err) __hip_atomic_store(err, (unsigned)NNHIP_DEVERR_KVCACHE_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int D = H * dh;
    const float* src = qkv + ((int64_t)b * T + tok) * ld + D + h * dh + c;
    const int64_t dst = (((int64_t)b * H + h) * Tmax + start + tok) * dh + c;
    *reinterpret_cast<dec_f4*>(Kc + dst) = *reinterpret_cast<const dec_f4*>(src);
    *reinterpret_cast<dec_f4*>(Vc + dst) = *reinterpret_cast<const dec_f4*>(src + D);
}

static int decode_check_dims(const char* fn, int64_t B, int64_t H, int64_t Tmax, int64_t dh) {
    NNHIP_CHECK_ARG(B >= 0 && H >= 0 && Tmax >= 0 && dh >= 0, NNHIP_EINVAL, "%s: negative size", fn);
    NNHIP_CHECK_ARG(dh == 32 || dh == 64 || dh == 128, NNHIP_EINVAL, "%s: unsupported head dim %lld (32, 64 or 128)", fn, (long long)dh);
    NNHIP_CHECK_ARG(B * H <= 65535 && Tmax < ((int64_t)1 << 30) && H * dh < ((int64_t)1 << 30), NNHIP_EINVAL,
                    "%s: size out of range (B*H <= 65535, Tmax < 2^30)", fn);
    return 0;
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int64_t nnhipAttentionDecodeWorkspace(int64_t B, int64_t H, int64_t Tmax, int64_t head_dim) {
    if (int rc = decode_check_dims("nnhipAttentionDecodeWorkspace", B, H, Tmax, head_dim)) return rc;
    if (B == 0 || H == 0 || Tmax == 0) return 0;
    const DecodePlan p = decode_plan(B, H, Tmax);
    return p.splits > 1 ? B * H * p.splits * (head_dim + 2) * (int64_t)sizeof(float) : 0;
}

extern "C" int nnhipAttentionDecode(const float* qkv, float* Kcache, float* Vcache, const int32_t* cache_len, float* O,
                                    float* workspace, int64_t B, int64_t H, int64_t Tmax, int64_t head_dim, int64_t ld_qkv,
                                    float scale, nnhipStream_t s) {
    if (int rc = decode_check_dims("nnhipAttentionDecode", B, H, Tmax, head_dim)) return rc;
    if (B == 0 || H == 0) return 0;
    NNHIP_CHECK_ARG(Tmax >= 1, NNHIP_EINVAL, "nnhipAttentionDecode: Tmax must be >= 1");
    NNHIP_CHECK_ARG(qkv && Kcache && Vcache && cache_len && O, NNHIP_EINVAL, "nnhipAttentionDecode: null pointer");
    NNHIP_CHECK_ARG(ld_qkv >= 3 * H * head_dim, NNHIP_EINVAL, "nnhipAttentionDecode: ld_qkv smaller than 3 * H * head_dim");
    const DecodePlan p = decode_plan(B, H, Tmax);
    NNHIP_CHECK_ARG(p.splits == 1 || workspace, NNHIP_EINVAL, "nnhipAttentionDecode: null workspace (nnhipAttentionDecodeWorkspace bytes needed)");
    NNHIP_CHECK_ARG(aligned16(qkv) && aligned16(Kcache) && aligned16(Vcache) && ld_qkv % 4 == 0 && aligned4(cache_len) && aligned4(O) &&
                    aligned4(workspace), NNHIP_EALIGN, "nnhipAttentionDecode: qkv / caches must be 16-byte aligned with ld_qkv a multiple of 4");
    if (int rc = device_error_status("nnhipAttentionDecode")) return rc;
    hipStream_t st = (hipStream_t)s;
    unsigned* err = device_error_word();
    const float sl2 = scale * kLog2e;
    const dim3 grid((unsigned)p.splits, (unsigned)(B * H));
#define DEC(DH_)                                                                                                                   \
    do {                                                                                                                           \
        hipLaunchKernelGGL(attn_decode_kernel<DH_>, grid, dim3(DEC_THREADS), 0, st, qkv, Kcache, Vcache, cache_len, O, workspace, \
                           (int)H, (int)Tmax, ld_qkv, sl2, p.chunk, err);                                                          \
        NNHIP_LAUNCH_CHECK("attn_decode_kernel");                                                                                  \
        if (p.splits > 1) {                                                                                                        \
            hipLaunchKernelGGL(attn_decode_merge_kernel<DH_>, dim3((unsigned)(B * H)), dim3(DH_ < 64 ? 64 : DH_), 0, st, workspace, \
                               cache_len, O, (int)H, (int)Tmax, p.chunk, p.splits);                                                \
            NNHIP_LAUNCH_CHECK("attn_decode_merge_kernel");                                                                        \
        }                                                                                                                          \
    } while (0)
    if (head_dim == 32) DEC(32);
    else if (head_dim == 64) DEC(64);
    else DEC(128);
#undef DEC
    return 0;
}

extern "C" int nnhipKVCacheFill(const float* qkv, float* Kcache, float* Vcache, const int32_t* cache_len, int64_t B, int64_t H,
                                int64_t T, int64_t Tmax, int64_t head_dim, int64_t ld_qkv, nnhipStream_t s) {
    if (int rc = decode_check_dims("nnhipKVCacheFill", B, H, Tmax, head_dim)) return rc;
    NNHIP_CHECK_ARG(T >= 0, NNHIP_EINVAL, "nnhipKVCacheFill: negative size");
    if (B == 0 || H == 0 || T == 0) return 0;
    NNHIP_CHECK_ARG(T <= Tmax, NNHIP_EINVAL, "nnhipKVCacheFill: %lld tokens do not fit a cache of %lld", (long long)T, (long long)Tmax);
    NNHIP_CHECK_ARG(qkv && Kcache && Vcache, NNHIP_EINVAL, "nnhipKVCacheFill: null pointer");
    NNHIP_CHECK_ARG(ld_qkv >= 3 * H * head_dim, NNHIP_EINVAL, "nnhipKVCacheFill: ld_qkv smaller than 3 * H * head_dim");
    NNHIP_CHECK_ARG(aligned16(qkv) && aligned16(Kcache) && aligned16(Vcache) && ld_qkv % 4 == 0 && aligned4(cache_len), NNHIP_EALIGN,
                    "nnhipKVCacheFill: qkv / caches must be 16-byte aligned with ld_qkv a multiple of 4");
    if (int rc = device_error_status("nnhipKVCacheFill")) return rc;
    const int64_t total = B * T * H * (head_dim / 4);
    hipLaunchKernelGGL(kv_cache_fill_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)s, qkv, Kcache, Vcache,
                       cache_len, total, (int)H, (int)T, (int)Tmax, (int)head_dim, ld_qkv, device_error_word());
    NNHIP_LAUNCH_CHECK("kv_cache_fill_kernel");
    return 0;
}
