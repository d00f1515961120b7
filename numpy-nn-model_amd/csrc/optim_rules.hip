// optim_rules.hip -- SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax and NAdam for gfx950 (ABI 221): a per-tensor launch and a
// one-launch multi-tensor step on the optimizer handle of optim.hip (plan blob with change-only upload, device-side stepping for
// hipGraph replay, grad_scale / gradient divisor).  CPU semantics: neunet/optim.py:76-244; the element updates: optim_rules_device.h.
// Pure bandwidth, and a rule only moves the streams it has: read p, g and write p (12 B/elem) plus 8 B/elem per state stream --
// SGD 12, Momentum / RMSprop / Adagrad 20, Adadelta / Adamax / NAdam 28 (= Adam).
#include "common.h"
#include "optim_rules_device.h"

namespace nnhip {

// float4 rounds of all of a rule's streams in flight per thread, by state-stream count (developer A/B: -DRULE_UNR0=..., 1, 2).
// Two rounds of Adam's four streams are eight 16-byte loads per thread; a rule with fewer streams takes more rounds to keep as many
// bytes in flight.  A thread whose share is shorter than that falls to two rounds, then one.
#ifndef RULE_UNR0
#define RULE_UNR0 4
#endif
#ifndef RULE_UNR1
#define RULE_UNR1 2
#endif
#ifndef RULE_UNR2
#define RULE_UNR2 2
#endif
template <int NS> struct RuleUnroll { static constexpr int kRounds = NS == 0 ? RULE_UNR0 : NS == 1 ? RULE_UNR1 : RULE_UNR2; };

typedef float rule_f4 __attribute__((ext_vector_type(4)));

template <int RULE>
__device__ __forceinline__ void rule4(rule_f4& P, const rule_f4& G, rule_f4& M, rule_f4& V, const AdamHyper& h) {
    float p0 = P.x, p1 = P.y, p2 = P.z, p3 = P.w, m0 = M.x, m1 = M.y, m2 = M.z, m3 = M.w, v0 = V.x, v1 = V.y, v2 = V.z, v3 = V.w;
    rule1<RULE>(p0, G.x, m0, v0, h); rule1<RULE>(p1, G.y, m1, v1, h); rule1<RULE>(p2, G.z, m2, v2, h); rule1<RULE>(p3, G.w, m3, v3, h);
    P.x = p0; P.y = p1; P.z = p2; P.w = p3; M.x = m0; M.y = m1; M.z = m2; M.w = m3; V.x = v0; V.y = v1; V.z = v2; V.w = v3;
}

// U float4 rounds at i, i + stride, ...: every load of every round leaves before the first update.  The gradient is dead after this
// pass: it is read past L2 allocation.  State streams the rule does not have are neither loaded nor stored (m4 / v4 may be null).
template <int RULE, int U>
__device__ __forceinline__ void rule_rounds(rule_f4* __restrict__ p4, const rule_f4* __restrict__ g4, rule_f4* __restrict__ m4,
                                            rule_f4* __restrict__ v4, int64_t i, int64_t stride_threads, const AdamHyper& h) {
    constexpr int NS = RuleTraits<RULE>::kState;
    rule_f4 P[U], G[U], M[U], V[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t k = i + u * stride_threads;
        P[u] = p4[k];
        G[u] = __builtin_nontemporal_load(&g4[k]);
        M[u] = V[u] = rule_f4{0.f, 0.f, 0.f, 0.f};
        if constexpr (NS >= 1) M[u] = m4[k];
        if constexpr (NS >= 2) V[u] = v4[k];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t k = i + u * stride_threads;
        rule4<RULE>(P[u], G[u], M[u], V[u], h);
        p4[k] = P[u];
        if constexpr (NS >= 1) m4[k] = M[u];
        if constexpr (NS >= 2) v4[k] = V[u];
    }
}

template <int RULE>
__device__ __forceinline__ void rule_scalar(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t j, const AdamHyper& h) {
    constexpr int NS = RuleTraits<RULE>::kState;
    float pj = p[j], mj = 0.f, vj = 0.f;
    if constexpr (NS >= 1) mj = m[j];
    if constexpr (NS >= 2) vj = v[j];
    rule1<RULE>(pj, g[j], mj, vj, h);
    p[j] = pj;
    if constexpr (NS >= 1) m[j] = mj;
    if constexpr (NS >= 2) v[j] = vj;
}

// Elements [0, n) of one tensor (or one chunk of it) by threads first, first + stride_threads, ...: the shape of adam_span.
// vec: every stream the rule has is 16-byte aligned -- float4 rounds, then the last n % 4 elements one by one; else one by one.
template <int RULE>
__device__ __forceinline__ void rule_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, int64_t n, int64_t first, int64_t stride_threads, bool vec,
                                          const AdamHyper& h) {
    constexpr int U = RuleUnroll<RuleTraits<RULE>::kState>::kRounds;
    if (vec) {
        const int64_t nv = n >> 2;
        rule_f4* __restrict__ p4 = reinterpret_cast<rule_f4*>(p);
        const rule_f4* __restrict__ g4 = reinterpret_cast<const rule_f4*>(g);
        rule_f4* __restrict__ m4 = reinterpret_cast<rule_f4*>(m);
        rule_f4* __restrict__ v4 = reinterpret_cast<rule_f4*>(v);
        int64_t i = first;
        for (; i + (U - 1) * stride_threads < nv; i += U * stride_threads) rule_rounds<RULE, U>(p4, g4, m4, v4, i, stride_threads, h);
        if constexpr (U > 2) {
            for (; i + stride_threads < nv; i += 2 * stride_threads) rule_rounds<RULE, 2>(p4, g4, m4, v4, i, stride_threads, h);
        }
        for (; i < nv; i += stride_threads) rule_rounds<RULE, 1>(p4, g4, m4, v4, i, stride_threads, h);
        for (int64_t j = (nv << 2) + first; j < n; j += stride_threads) rule_scalar<RULE>(p, g, m, v, j, h);
    } else {
        for (int64_t j = first; j < n; j += stride_threads) rule_scalar<RULE>(p, g, m, v, j, h);
    }
}

template <int RULE>
__global__ __launch_bounds__(256) void optim_rule_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, int64_t n, bool vec, const AdamHyper h) {
    rule_span<RULE>(p, g, m, v, n, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256, vec, h);
}

// One block per chunk of the handle's plan (optim.hip: fused_optimizer_plan).  Blob: [p*][g*] and one table per state stream of the
// rule (n pointers each) [sizes int64 n][blk_tensor int32 nblk][blk_chunk int32 nblk].  dev_state / grad_div: the device-side
// stepping protocol of adam_device.h, unchanged -- lr and grad_scale come from the state, and so do bc1 / bc2 for the rules with
// betas; the others pass b1 = b2 = 0, for which the corrections are 1 and never recomputed.  The last block advances the step.
template <int RULE>
__global__ __launch_bounds__(256) void optim_rule_multi_kernel(const unsigned char* __restrict__ blob, int n, int nblk, AdamHyper h,
                                                               float* __restrict__ dev_state, double b1, double b2, int chunk,
                                                               const float* __restrict__ grad_div) {
    constexpr int NS = RuleTraits<RULE>::kState;
    __shared__ float sh[5];
    AdamDevRaw raw;
    adam_dev_issue(raw, dev_state, grad_div);              // thread 0's state loads leave now; the plan lookups run behind them
    const size_t table = sizeof(void*) * (size_t)n;
    float* const* P = reinterpret_cast<float* const*>(blob);
    const float* const* G = reinterpret_cast<const float* const*>(blob + table);
    const int64_t* sizes = reinterpret_cast<const int64_t*>(blob + table * (2 + NS));
    const int32_t* blk_tensor = reinterpret_cast<const int32_t*>(blob + table * (2 + NS) + sizeof(int64_t) * n);
    const int32_t* blk_chunk = blk_tensor + nblk;
    const int ti = blk_tensor[blockIdx.x];
    const int64_t off = (int64_t)blk_chunk[blockIdx.x] * chunk;
    int64_t cnt = sizes[ti] - off;
    if (cnt > chunk) cnt = chunk;
    float* p = P[ti] + off;
    const float* g = G[ti] + off;
    float* m = nullptr;
    float* v = nullptr;
    uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g);
    if constexpr (NS >= 1) { m = reinterpret_cast<float* const*>(blob + table * 2)[ti] + off; bits |= reinterpret_cast<uintptr_t>(m); }
    if constexpr (NS >= 2) { v = reinterpret_cast<float* const*>(blob + table * 3)[ti] + off; bits |= reinterpret_cast<uintptr_t>(v); }
    // chunk offsets are multiples of 2048 elements, so 16-B alignment of the chunk == of the tensor
    const bool vec = (bits & 15u) == 0;
    adam_dev_resolve(h, raw, dev_state, b1, b2, grad_div, sh);
    rule_span<RULE>(p, g, m, v, cnt, threadIdx.x, 256, vec, h);
    adam_dev_finish(dev_state, nblk, b1, b2);
}

template <int RULE>
static void launch_rule(float* p, const float* g, float* m, float* v, int64_t n, const AdamHyper& h, hipStream_t st) {
    constexpr int NS = RuleTraits<RULE>::kState;
    const bool vec = aligned16(p) && aligned16(g) && (NS < 1 || aligned16(m)) && (NS < 2 || aligned16(v));
    int64_t blocks = ceil_div(vec ? (n >> 2) + 1 : n, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(optim_rule_kernel<RULE>, dim3((unsigned)blocks), dim3(256), 0, st, p, g, m, v, n, vec, h);
}

template <int RULE>
static void launch_rule_multi(const unsigned char* blob, int n, int nblk, const AdamHyper& h, float* dev_state, double b1, double b2,
                              int chunk, const float* grad_div, hipStream_t st) {
    hipLaunchKernelGGL(optim_rule_multi_kernel<RULE>, dim3((unsigned)nblk), dim3(256), 0, st, blob, n, nblk, h, dev_state, b1, b2,
                       chunk, grad_div);
}

#define NNHIP_RULE_DISPATCH(rule, fn, ...)                                   \
    switch (rule) {                                                          \
        case NNHIP_OPT_SGD: fn<NNHIP_OPT_SGD>(__VA_ARGS__); break;           \
        case NNHIP_OPT_MOMENTUM: fn<NNHIP_OPT_MOMENTUM>(__VA_ARGS__); break; \
        case NNHIP_OPT_RMSPROP: fn<NNHIP_OPT_RMSPROP>(__VA_ARGS__); break;   \
        case NNHIP_OPT_ADAGRAD: fn<NNHIP_OPT_ADAGRAD>(__VA_ARGS__); break;   \
        case NNHIP_OPT_ADADELTA: fn<NNHIP_OPT_ADADELTA>(__VA_ARGS__); break; \
        case NNHIP_OPT_ADAMAX: fn<NNHIP_OPT_ADAMAX>(__VA_ARGS__); break;     \
        default: fn<NNHIP_OPT_NADAM>(__VA_ARGS__); break;                    \
    }

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipOptimizerRuleStep(int32_t rule, float* p, const float* g, float* s1, float* s2, int64_t n, double lr,
                                      double coef1, double coef2, double eps, int32_t step, float grad_scale, nnhipStream_t s) {
    const int ns = rule_state_count(rule);
    NNHIP_CHECK_ARG(ns >= 0, NNHIP_EINVAL, "nnhipOptimizerRuleStep: unknown rule %d", (int)rule);
    NNHIP_CHECK_ARG(n >= 0, NNHIP_EINVAL, "nnhipOptimizerRuleStep: negative size");
    NNHIP_CHECK_ARG(step >= 1, NNHIP_EINVAL, "nnhipOptimizerRuleStep: step >= 1 required");
    if (n == 0) return 0;
    NNHIP_CHECK_ARG(p && g, NNHIP_EINVAL, "nnhipOptimizerRuleStep: null pointer");
    NNHIP_CHECK_ARG((ns < 1 || s1) && (ns < 2 || s2), NNHIP_EINVAL, "nnhipOptimizerRuleStep: null state pointer (the rule has %d state stream(s))", ns);
    const AdamHyper h = make_hyper(lr, coef1, coef2, eps, 0.0, step, 0, grad_scale);
    NNHIP_RULE_DISPATCH(rule, launch_rule, p, g, s1, s2, n, h, (hipStream_t)s);
    NNHIP_LAUNCH_CHECK("optim_rule_kernel");
    return 0;
}

extern "C" int nnhipOptimizerRuleMultiTensorStep(void* opt, int32_t rule, int32_t n_tensors, float* const* p, const float* const* g,
                                                 float* const* s1, float* const* s2, const int64_t* sizes, double lr, double coef1,
                                                 double coef2, double eps, int32_t step, float grad_scale, nnhipStream_t s) {
    NNHIP_CHECK_ARG(opt != nullptr, NNHIP_EINVAL, "nnhipOptimizerRuleMultiTensorStep: null optimizer handle");
    if (int rc = device_error_status("nnhipOptimizerRuleMultiTensorStep")) return rc;   // an earlier kernel raised the device error word
    const int ns = rule_state_count(rule);
    NNHIP_CHECK_ARG(ns >= 0, NNHIP_EINVAL, "nnhipOptimizerRuleMultiTensorStep: unknown rule %d", (int)rule);
    NNHIP_CHECK_ARG(n_tensors >= 0 && step >= 0, NNHIP_EINVAL, "nnhipOptimizerRuleMultiTensorStep: bad n_tensors/step");
    if (n_tensors == 0) return 0;
    NNHIP_CHECK_ARG(p && g && sizes, NNHIP_EINVAL, "nnhipOptimizerRuleMultiTensorStep: null table");
    NNHIP_CHECK_ARG((ns < 1 || s1) && (ns < 2 || s2), NNHIP_EINVAL, "nnhipOptimizerRuleMultiTensorStep: null state table (the rule has %d state stream(s))", ns);
    float* dstate = nullptr;
    const float* grad_div = nullptr;
    if (int rc = fused_optimizer_state(opt, step, &dstate, &grad_div)) {               // step == 0 without SetStep + SetHyper: EINVAL,
        set_last_error("nnhipOptimizerRuleMultiTensorStep: step == 0 needs nnhipFusedOptimizerSetStep and SetHyper first");   // before the plan
        return rc;
    }
    hipStream_t st = (hipStream_t)s;
    const void* const* const tables[4] = {reinterpret_cast<const void* const*>(p), reinterpret_cast<const void* const*>(g),
                                          reinterpret_cast<const void* const*>(s1), reinterpret_cast<const void* const*>(s2)};
    const unsigned char* blob = nullptr;
    int nblk = 0, chunk = 0;
    if (int rc = fused_optimizer_plan(opt, "nnhipOptimizerRuleMultiTensorStep", n_tensors, 2 + ns, tables, sizes, st, &blob, &nblk, &chunk)) return rc;
    if (nblk == 0) return 0;
    const AdamHyper h = make_hyper(lr, coef1, coef2, eps, 0.0, step > 0 ? step : 1, 0, grad_scale);
    const double b1 = rule_has_betas(rule) ? coef1 : 0.0, b2 = rule_has_betas(rule) ? coef2 : 0.0;
    NNHIP_RULE_DISPATCH(rule, launch_rule_multi, blob, n_tensors, nblk, h, dstate, b1, b2, chunk, grad_div, st);
    NNHIP_LAUNCH_CHECK("optim_rule_multi_kernel");
    return 0;
}
