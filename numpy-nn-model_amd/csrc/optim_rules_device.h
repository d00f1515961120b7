// optim_rules_device.h -- the element updates of SGD, Momentum, RMSprop, Adagrad, Adadelta, Adamax and NAdam (neunet/optim.py:76-244)
// for the kernels of optim_rules.hip.  Adam / AdamW stay in adam_device.h; the device-side stepping protocol (adam_dev_*) and the
// hyper-parameter struct are shared with them.
#pragma once
#include "adam_device.h"

namespace nnhip {

// A rule's hyper-parameters travel in an AdamHyper (make_hyper rounds them where NumPy does): lr, eps, grad_scale as they are;
// b1 / one_m_b1 = the rule's first coefficient c and (float)(1 - c) (Momentum's momentum, RMSprop's alpha, Adadelta's rho, beta1);
// b2 / one_m_b2 = beta2; bc1 / bc2 = 1 - beta^t (Adamax, NAdam).  wd and decay_mode are unused.
template <int RULE> struct RuleTraits;
template <> struct RuleTraits<NNHIP_OPT_SGD>      { static constexpr int kState = 0; static constexpr bool kBetas = false; };
template <> struct RuleTraits<NNHIP_OPT_MOMENTUM> { static constexpr int kState = 1; static constexpr bool kBetas = false; };
template <> struct RuleTraits<NNHIP_OPT_RMSPROP>  { static constexpr int kState = 1; static constexpr bool kBetas = false; };
template <> struct RuleTraits<NNHIP_OPT_ADAGRAD>  { static constexpr int kState = 1; static constexpr bool kBetas = false; };
template <> struct RuleTraits<NNHIP_OPT_ADADELTA> { static constexpr int kState = 2; static constexpr bool kBetas = false; };
template <> struct RuleTraits<NNHIP_OPT_ADAMAX>   { static constexpr int kState = 2; static constexpr bool kBetas = true; };
template <> struct RuleTraits<NNHIP_OPT_NADAM>    { static constexpr int kState = 2; static constexpr bool kBetas = true; };

inline int rule_state_count(int rule) {
    switch (rule) {
        case NNHIP_OPT_SGD: return 0;
        case NNHIP_OPT_MOMENTUM: case NNHIP_OPT_RMSPROP: case NNHIP_OPT_ADAGRAD: return 1;
        case NNHIP_OPT_ADADELTA: case NNHIP_OPT_ADAMAX: case NNHIP_OPT_NADAM: return 2;
        default: return -1;
    }
}
inline bool rule_has_betas(int rule) { return rule == NNHIP_OPT_ADAMAX || rule == NNHIP_OPT_NADAM; }

// One element.  `m` / `v` are registers the caller loaded from the rule's first / second state stream (and stores back) when the
// rule has that stream, and dead otherwise.  No floating-point contraction, for adam1's reason (adam_device.h): the rule must give
// the same bits wherever it is inlined -- the vector path, the scalar path, the per-tensor and the multi-tensor kernel.
template <int RULE>
__device__ __forceinline__ void rule1(float& p, float g, float& m, float& v, const AdamHyper& h) {
#pragma clang fp contract(off)
    g *= h.grad_scale;
    if constexpr (RULE == NNHIP_OPT_SGD) {
        p = p - h.lr * g;                                        // optim.py:86
    } else if constexpr (RULE == NNHIP_OPT_MOMENTUM) {
        m = h.b1 * m + h.one_m_b1 * g;                           // optim.py:105
        p = p - m * h.lr;                                        // optim.py:106
    } else if constexpr (RULE == NNHIP_OPT_RMSPROP) {
        m = h.b1 * m + h.one_m_b1 * (g * g);                     // optim.py:127
        p = p - h.lr * g / (sqrtf(m) + h.eps);                   // optim.py:128
    } else if constexpr (RULE == NNHIP_OPT_ADAGRAD) {
        m = m + g * g;                                           // optim.py:148
        p = p - h.lr * g / (sqrtf(m) + h.eps);                   // optim.py:149
    } else if constexpr (RULE == NNHIP_OPT_ADADELTA) {           // lr is not part of the reference's rule
        m = h.b1 * m + h.one_m_b1 * (g * g);                     // optim.py:171
        const float dx = -(sqrtf(v + h.eps) / sqrtf(m + h.eps)) * g;   // optim.py:172-175
        v = h.b1 * v + h.one_m_b1 * (dx * dx);                   // optim.py:176
        p = p + dx;                                              // optim.py:177
    } else if constexpr (RULE == NNHIP_OPT_ADAMAX) {
        m = h.b1 * m + h.one_m_b1 * g;                           // optim.py:202
        const float a = h.b2 * v, b = fabsf(g);
        v = (a > b || a != a) ? a : b;                           // optim.py:203 -- np.maximum: a NaN on either side stays
        const float mh = m / h.bc1;                              // optim.py:205
        p = p - h.lr * mh / (v + h.eps);                         // optim.py:207
    } else {
        static_assert(RULE == NNHIP_OPT_NADAM, "unknown optimizer rule");
        m = h.b1 * m + h.one_m_b1 * g;                           // optim.py:232
        v = h.b2 * v + h.one_m_b2 * (g * g);                     // optim.py:233
        const float mh = m / h.bc1 + h.one_m_b1 * g / h.bc1;     // optim.py:235-237
        const float vh = v / h.bc2;                              // optim.py:238
        p = p - h.lr * mh / (sqrtf(vh) + h.eps);                 // optim.py:240
    }
}

// The optimizer handle's plan (optim.hip): one blob of `n_tables` pointer tables (n device pointers each, in the order given),
// the sizes and the block -> (tensor, chunk) map, compared with the last upload and sent only when it changed.  Checks the sizes
// and the pointers of non-empty tensors (`who` names the entry in the message).  *nblk == 0: nothing to launch.  `slot`: which of the
// handle's plan caches (0 = the update's, 1 = the gradient norm's, grad_norm.hip).
int fused_optimizer_plan(void* opt, const char* who, int n, int n_tables, const void* const* const* tables, const int64_t* sizes,
                         hipStream_t st, const unsigned char** dev_blob, int* nblk, int* chunk, int slot = 0);
int fused_optimizer_state(void* opt, int step, float** dev_state, const float** grad_div);
// The handle's scratch for the gradient norm's in-launch finish: one zeroed ticket word and >= nblk floats (grow-only; growing inside
// a stream capture is NNHIP_ENOMEM).
int fused_optimizer_norm_scratch(void* opt, const char* who, int nblk, hipStream_t st, unsigned** ticket, float** partials);

}  // namespace nnhip
