// attention_decode.h -- the lane layout the two single-query attention kernels share (attention_decode.hip: the KV-cached
// self-attention step; attention_cross_decode.hip: one query row against a read-only encoder memory).
//
// LPK = min(16, dh/4) adjacent lanes own one key (a float4 each, two for dh 128), so a wave works on KPW = 64/LPK keys at once
// and a score is a DPP reduction inside a 16-lane row.  Every key slot of every wave keeps its own online-softmax state
// (m, l, o[dh] spread over its LPK lanes); a block has NSLOT = DEC_WAVES * KPW of them and folds them through LDS in slot order.
#pragma once
#include "common.h"

namespace nnhip {

constexpr int DEC_THREADS = 256, DEC_WAVES = 4, DEC_U = 4, DEC_PASS = 64;
typedef float dec_f4 __attribute__((ext_vector_type(4)));

template <int DH>
struct DecLanes {
    static constexpr int LPK = DH / 4 < 16 ? DH / 4 : 16;       // lanes per key
    static constexpr int NV = DH / (4 * LPK);                   // float4 per lane and key (2 for dh 128)
    static constexpr int KPW = 64 / LPK;                        // keys per wave-load
    static constexpr int NSLOT = DEC_WAVES * KPW;
    static constexpr int KPI = DEC_WAVES * DEC_U * KPW;         // keys per block iteration
};

template <int LPK>
__device__ __forceinline__ float group_sum(float v) {      // sum over the LPK adjacent lanes that own one key
    v += dpp_f32<kDppXor1>(v);
    v += dpp_f32<kDppXor2>(v);
    v += dpp_f32<kDppHalfMirror>(v);
    if constexpr (LPK == 16) v += dpp_f32<kDppMirror>(v);
    return v;
}

// q . k over this lane's NV float4 pieces (the caller finishes it with group_sum)
template <int NV>
__device__ __forceinline__ float dec_dot(const dec_f4 (&q)[NV], const dec_f4 (&k)[NV]) {
    float d = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) d += (q[v].x * k[v].x + q[v].y * k[v].y) + (q[v].z * k[v].z + q[v].w * k[v].w);
    return d;
}

// One key into a slot's online-softmax state: sc is the score in the log2 domain, -inf for a slot that holds no key this time.
template <int NV>
__device__ __forceinline__ void dec_online_step(float sc, bool ok, const dec_f4 (&vv)[NV], float& m, float& l, dec_f4 (&o)[NV]) {
    const float mn = fmaxf(m, sc);
    const float alpha = mn == -INFINITY ? 1.f : __builtin_amdgcn_exp2f(m - mn);
    const float p = ok ? __builtin_amdgcn_exp2f(sc - mn) : 0.f;
    l = l * alpha + p;
#pragma unroll
    for (int v = 0; v < NV; ++v) o[v] = o[v] * alpha + vv[v] * p;
    m = mn;
}

}  // namespace nnhip
