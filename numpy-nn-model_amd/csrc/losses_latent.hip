// losses_latent.hip -- what the VAE / GAN examples need besides their layers (examples/vae.ipynb, examples/gan.ipynb):
// BCELoss (neunet/nn/losses.py:25-56) and the VAE's two latent-space expressions, the reparameterisation z = mu + eps exp(logvar / 2)
// and the KL term -1/2 sum(1 + logvar - mu^2 - exp(logvar)).  Loss and gradient come from one pass, as in mse_kernel (pool_norm.hip);
// the two reductions are the fixed-order block sums of common.h (one block up to 16384 elements; beyond, per-block partials in the
// library workspace and a second, one-block launch).
#include <math.h>

#include "common.h"

namespace nnhip {

// One element of BCELoss: term = -(y log p + (1 - y) log(1 - p)) w, the reference's expression literally -- NO clamp: p = 0 or 1
// gives inf (or NaN where 0 * inf meets), as np.log does.  The gradient written is d(reduced loss)/dp = -(y / p - (1 - y) / (1 - p)) w scale,
// or with fold (p is a Sigmoid's output, the gradient goes to the Sigmoid's input z) dz = (p - y) w scale: the p (1 - p) of the Sigmoid
// backward (activations.py:12-13) cancelled against the two divisions analytically, finite at a saturated p.
struct BceTerm {
    const float* p; const float* y; const float* w; float ws; float* dp; float* out; float scale; int fold;
    __device__ float operator()(int64_t i) const {
        const float pi = p[i], yi = y[i], wi = w ? w[i] : ws;
        const float t = -((yi * logf(pi) + (1.0f - yi) * logf(1.0f - pi)) * wi);
        if (dp) dp[i] = fold ? (pi - yi) * wi * scale : -(yi / pi - (1.0f - yi) / (1.0f - pi)) * wi * scale;
        if (out) out[i] = t;                                  // reduction 'none'
        return t;
    }
};
// One element of the KL term: 1 + logvar - mu^2 - exp(logvar) (the sum is scaled by -1/2); d/dmu = mu, d/dlogvar = (exp(logvar) - 1) / 2.
struct KldTerm {
    const float* mu; const float* lv; float* dmu; float* dlv;
    __device__ float operator()(int64_t i) const {
        const float m = mu[i], l = lv[i], e = expf(l);
        if (dmu) { dmu[i] = m; dlv[i] = 0.5f * (e - 1.0f); }
        return 1.0f + l - m * m - e;
    }
};

// One element of L1Loss (neunet/nn/losses.py:139): |p - t|; d/dp = sign(p - t) scale, sign(0) = 0 as np.sign (neunet/autograd.py:599)
struct L1Term {
    const float* p; const float* y; float* dp; float* out; float scale;
    __device__ float operator()(int64_t i) const {
        const float d = p[i] - y[i], t = fabsf(d);
        if (dp) dp[i] = d > 0.f ? scale : (d < 0.f ? -scale : d * scale);     // d == 0 -> 0, a NaN difference -> NaN (np.sign)
        if (out) out[i] = t;
        return t;
    }
};
// One element of KLDivLoss (neunet/nn/losses.py:163-166), the reference's expression literally: t (log t - p) -- t = 0 gives
// 0 * -inf = NaN as np.log does -- or, with a log-space target, exp(t) (t - p); d/dp = -t scale or -exp(t) scale
struct KLDivTerm {
    const float* p; const float* y; float* dp; float* out; float scale; int log_target;
    __device__ float operator()(int64_t i) const {
        const float pi = p[i], yi = y[i];
        const float w = log_target ? expf(yi) : yi;
        const float t = log_target ? w * (yi - pi) : w * (logf(yi) - pi);
        if (dp) dp[i] = -w * scale;
        if (out) out[i] = t;
        return t;
    }
};

template <class T>
__global__ __launch_bounds__(1024) void ll_small_kernel(T term, int64_t n, float scale, float* __restrict__ loss) {
    __shared__ float red[16];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += term(i);
    s = block_sum<16>(s, red);
    if (threadIdx.x == 0 && loss) loss[0] = s * scale;
}
template <class T>
__global__ __launch_bounds__(256) void ll_part_kernel(T term, int64_t n, float* __restrict__ part) {
    __shared__ float red[4];
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += term(i);
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0 && part) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void ll_final_kernel(const float* __restrict__ part, int nparts, float scale, float* __restrict__ loss) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0) loss[0] = s * scale;
}

constexpr int64_t LL_SMALL = 16384;       // one 1024-thread block: 16 elements per thread

// reduce = false: the elementwise pass only (reduction 'none'), no sum is written
template <class T>
static int ll_launch(const char* fn, T term, int64_t n, float scale, float* loss, bool reduce, hipStream_t st) {
    if (n <= LL_SMALL) {
        hipLaunchKernelGGL(ll_small_kernel<T>, dim3(1), dim3(1024), 0, st, term, n, scale, reduce ? loss : nullptr);
        NNHIP_LAUNCH_CHECK("ll_small_kernel");
        return 0;
    }
    int64_t blocks = ceil_div(n, 1024);
    if (blocks > 1024) blocks = 1024;
    float* part = nullptr;
    if (reduce) {
        part = static_cast<float*>(workspace((size_t)blocks * sizeof(float)));
        NNHIP_CHECK_ARG(part != nullptr, NNHIP_ENOMEM, "%s: workspace allocation failed", fn);
    }
    hipLaunchKernelGGL(ll_part_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, term, n, part);
    NNHIP_LAUNCH_CHECK("ll_part_kernel");
    if (reduce) {
        hipLaunchKernelGGL(ll_final_kernel, dim3(1), dim3(256), 0, st, part, (int)blocks, scale, loss);
        NNHIP_LAUNCH_CHECK("ll_final_kernel");
    }
    return 0;
}

// ---- NLLLoss (neunet/nn/losses.py:83-126) ------------------------------------------------------------------------------------------
// Position p = n * inner + i of logp [outer, C, inner] with label y = labels[p]: it COUNTS when y != ignore and 0 <= y < C; then
// w = class_weight[y] (or 1), term = -logp[n, y, i] w and the gradient's one value is -w scale at logp[n, y, i].  A position that
// does not count reads neither logp nor the weights (the reference indexes weight[y] before it masks, losses.py:115).
int fill_f32(float* p, float v, int64_t n, hipStream_t st);   // elementwise.hip

struct NllArgs {
    const float* logp; const void* labels; const float* cw; float* terms; float* dlogp; float* pos_grad;
    int64_t ignore, C, inner, P;
    int lbytes;
};
// true when position p counts: its weight and the offset of its logp entry
__device__ __forceinline__ bool nll_position(const NllArgs& a, int64_t p, float& w, int64_t& off) {
    const int64_t y = load_label(a.labels, p, a.lbytes);
    if (y == a.ignore || y < 0 || y >= a.C) return false;
    const int64_t n = p / a.inner, i = p - n * a.inner;
    off = (n * a.C + y) * a.inner + i;
    w = a.cw ? a.cw[y] : 1.0f;
    return true;
}
// one position's contribution to (sum of terms, sum of weights); reduction 'none' keeps the term
__device__ __forceinline__ void nll_term(const NllArgs& a, int64_t p, float& s, float& d) {
    float w = 0.f, term = 0.f;
    int64_t off;
    if (nll_position(a, p, w, off)) term = -a.logp[off] * w;
    if (a.terms) a.terms[p] = term;
    s += term;
    d += w;
}
__device__ __forceinline__ void nll_grad(const NllArgs& a, int64_t p, float scale) {
    float w, g = 0.f;
    int64_t off;
    if (nll_position(a, p, w, off)) {
        g = -w * scale;
        if (a.dlogp) a.dlogp[off] = g;
    }
    if (a.pos_grad) a.pos_grad[p] = g;
}
// mode: 0 'none' (scale 1), 1 'mean' (scale 1 / sum of weights; a zero denominator gives loss 0 and a zero gradient), 2 'sum'
__device__ __forceinline__ float nll_scale(int mode, float d) { return mode == 1 ? (d > 0.f ? 1.0f / d : 0.f) : 1.0f; }
// up to LL_SMALL positions: one block forms both sums, then writes the gradient with the scale it has just derived
__global__ __launch_bounds__(1024) void nll_small_kernel(NllArgs a, int mode, float* __restrict__ loss) {
    __shared__ float red[32];
    float s = 0.f, d = 0.f;
    for (int64_t p = threadIdx.x; p < a.P; p += 1024) nll_term(a, p, s, d);
    block_sum2<16>(s, d, red);
    if (threadIdx.x == 0 && mode != 0) loss[0] = mode == 1 ? (d > 0.f ? s / d : 0.f) : s;
    if (!a.dlogp && !a.pos_grad) return;
    const float scale = nll_scale(mode, d);
    for (int64_t p = threadIdx.x; p < a.P; p += 1024) nll_grad(a, p, scale);
}
// beyond: per-block partial (term, weight) sums, a one-block finish that writes the loss and leaves the scale in scale_out for
// the gradient pass
__global__ __launch_bounds__(256) void nll_part_kernel(NllArgs a, float* __restrict__ part) {
    __shared__ float red[8];
    float s = 0.f, d = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.P; p += (int64_t)gridDim.x * 256) nll_term(a, p, s, d);
    block_sum2<4>(s, d, red);
    if (threadIdx.x == 0 && part) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = d; }
}
__global__ __launch_bounds__(256) void nll_final_kernel(const float* __restrict__ part, int nparts, int mode, float* __restrict__ loss,
                                                        float* __restrict__ scale_out) {
    __shared__ float red[8];
    float s = 0.f, d = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) { s += part[2 * i]; d += part[2 * i + 1]; }
    block_sum2<4>(s, d, red);
    if (threadIdx.x == 0) {
        loss[0] = mode == 1 ? (d > 0.f ? s / d : 0.f) : s;
        scale_out[0] = nll_scale(mode, d);
    }
}
__global__ __launch_bounds__(256) void nll_grad_kernel(NllArgs a, const float* scale_dev) {
    const float scale = scale_dev ? ld_dev_f32(scale_dev) : 1.0f;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.P; p += (int64_t)gridDim.x * 256) nll_grad(a, p, scale);
}

// z = mu + eps * std, std = exp(logvar / 2)
__global__ __launch_bounds__(256) void reparam_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                          const float* __restrict__ eps, float* __restrict__ z,
                                                          float* __restrict__ sd, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float s = expf(0.5f * lv[i]);
        sd[i] = s;
        z[i] = mu[i] + eps[i] * s;
    }
}
// dmu = g ; dlogvar = g * eps * 0.5 * std
__global__ __launch_bounds__(256) void reparam_bwd_kernel(const float* __restrict__ g, const float* __restrict__ eps,
                                                          const float* __restrict__ sd, float* __restrict__ dmu,
                                                          float* __restrict__ dlv, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i];
        dmu[i] = gi;
        dlv[i] = gi * eps[i] * 0.5f * sd[i];
    }
}
static inline unsigned ll_blocks(int64_t n) {
    const int64_t b = ceil_div(n, 256);
    return (unsigned)(b < 65535 ? b : 65535);
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipBCELossForwardBackward(const float* pred, const float* target, const float* weight, float weight_scalar,
                                           float* loss, float* dpred, int64_t n, char reduction, int sigmoid_fold, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n > 0, NNHIP_EINVAL, "nnhipBCELossForwardBackward: n must be > 0");
    NNHIP_CHECK_ARG(reduction == 'm' || reduction == 's' || reduction == 'n', NNHIP_EINVAL,
                    "nnhipBCELossForwardBackward: reduction must be 'm', 's' or 'n'");
    NNHIP_CHECK_ARG(pred && target && loss, NNHIP_EINVAL, "nnhipBCELossForwardBackward: null pointer");
    const float scale = reduction == 'm' ? 1.0f / (float)n : 1.0f;
    const bool none = reduction == 'n';
    BceTerm term{pred, target, weight, weight_scalar, dpred, none ? loss : nullptr, scale, sigmoid_fold ? 1 : 0};
    return ll_launch("nnhipBCELossForwardBackward", term, n, scale, loss, !none, (hipStream_t)s);
}

extern "C" int nnhipGaussianKLDForwardBackward(const float* mu, const float* logvar, float* loss, float* dmu, float* dlogvar,
                                               int64_t n, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n > 0, NNHIP_EINVAL, "nnhipGaussianKLDForwardBackward: n must be > 0");
    NNHIP_CHECK_ARG(mu && logvar && loss, NNHIP_EINVAL, "nnhipGaussianKLDForwardBackward: null pointer");
    NNHIP_CHECK_ARG((dmu == nullptr) == (dlogvar == nullptr), NNHIP_EINVAL, "nnhipGaussianKLDForwardBackward: dmu and dlogvar go together");
    KldTerm term{mu, logvar, dmu, dlogvar};
    return ll_launch("nnhipGaussianKLDForwardBackward", term, n, -0.5f, loss, true, (hipStream_t)s);
}

extern "C" int nnhipGaussianReparamForward(const float* mu, const float* logvar, const float* eps, float* z, float* std_out,
                                           int64_t n, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n >= 0, NNHIP_EINVAL, "nnhipGaussianReparamForward: negative size");
    if (n == 0) return 0;
    NNHIP_CHECK_ARG(mu && logvar && eps && z && std_out, NNHIP_EINVAL, "nnhipGaussianReparamForward: null pointer");
    hipLaunchKernelGGL(reparam_fwd_kernel, dim3(ll_blocks(n)), dim3(256), 0, (hipStream_t)s, mu, logvar, eps, z, std_out, n);
    NNHIP_LAUNCH_CHECK("reparam_fwd_kernel");
    return 0;
}
extern "C" int nnhipGaussianReparamBackward(const float* dz, const float* eps, const float* std_saved, float* dmu, float* dlogvar,
                                            int64_t n, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n >= 0, NNHIP_EINVAL, "nnhipGaussianReparamBackward: negative size");
    if (n == 0) return 0;
    NNHIP_CHECK_ARG(dz && eps && std_saved && dmu && dlogvar, NNHIP_EINVAL, "nnhipGaussianReparamBackward: null pointer");
    hipLaunchKernelGGL(reparam_bwd_kernel, dim3(ll_blocks(n)), dim3(256), 0, (hipStream_t)s, dz, eps, std_saved, dmu, dlogvar, n);
    NNHIP_LAUNCH_CHECK("reparam_bwd_kernel");
    return 0;
}

extern "C" int nnhipL1LossForwardBackward(const float* pred, const float* target, float* loss, float* dpred, int64_t n, char reduction,
                                          nnhipStream_t s) {
    NNHIP_CHECK_ARG(n > 0, NNHIP_EINVAL, "nnhipL1LossForwardBackward: n must be > 0");
    NNHIP_CHECK_ARG(reduction == 'm' || reduction == 's' || reduction == 'n', NNHIP_EINVAL,
                    "nnhipL1LossForwardBackward: reduction must be 'm', 's' or 'n'");
    NNHIP_CHECK_ARG(pred && target && loss, NNHIP_EINVAL, "nnhipL1LossForwardBackward: null pointer");
    const float scale = reduction == 'm' ? 1.0f / (float)n : 1.0f;
    const bool none = reduction == 'n';
    L1Term term{pred, target, dpred, none ? loss : nullptr, scale};
    return ll_launch("nnhipL1LossForwardBackward", term, n, scale, loss, !none, (hipStream_t)s);
}

extern "C" int nnhipKLDivLossForwardBackward(const float* pred, const float* target, float* loss, float* dpred, int64_t n, int64_t batch,
                                             int log_target, char reduction, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n > 0, NNHIP_EINVAL, "nnhipKLDivLossForwardBackward: n must be > 0");
    NNHIP_CHECK_ARG(reduction == 'm' || reduction == 'b' || reduction == 's' || reduction == 'n', NNHIP_EINVAL,
                    "nnhipKLDivLossForwardBackward: reduction must be 'm', 'b', 's' or 'n'");
    NNHIP_CHECK_ARG(reduction != 'b' || batch > 0, NNHIP_EINVAL, "nnhipKLDivLossForwardBackward: batch must be > 0 for 'b' (batchmean)");
    NNHIP_CHECK_ARG(pred && target && loss, NNHIP_EINVAL, "nnhipKLDivLossForwardBackward: null pointer");
    const float scale = reduction == 'm' ? 1.0f / (float)n : reduction == 'b' ? 1.0f / (float)batch : 1.0f;
    const bool none = reduction == 'n';
    KLDivTerm term{pred, target, dpred, none ? loss : nullptr, scale, log_target ? 1 : 0};
    return ll_launch("nnhipKLDivLossForwardBackward", term, n, scale, loss, !none, (hipStream_t)s);
}

extern "C" int nnhipNLLLossForwardBackward(const float* logp, const void* labels, int32_t label_bytes, const float* class_weight_or_null,
                                           int64_t ignore_index, int64_t outer, int64_t n_cols, int64_t inner, char reduction, float* loss,
                                           float* dlogp_or_null, float* pos_grad_or_null, nnhipStream_t s) {
    NNHIP_CHECK_ARG(outer >= 0 && n_cols >= 0 && inner >= 0, NNHIP_EINVAL, "nnhipNLLLossForwardBackward: negative size");
    NNHIP_CHECK_ARG(reduction == 'm' || reduction == 's' || reduction == 'n', NNHIP_EINVAL,
                    "nnhipNLLLossForwardBackward: reduction must be 'm', 's' or 'n'");
    NNHIP_CHECK_ARG(label_bytes == 2 || label_bytes == 4 || label_bytes == 8, NNHIP_EINVAL,
                    "nnhipNLLLossForwardBackward: label_bytes must be 2, 4 or 8");
    NNHIP_CHECK_ARG(logp && labels && loss, NNHIP_EINVAL, "nnhipNLLLossForwardBackward: null pointer");
    NNHIP_CHECK_ARG(outer == 0 || inner == 0 || n_cols == 0 || outer <= INT64_MAX / inner / n_cols, NNHIP_EINVAL,
                    "nnhipNLLLossForwardBackward: outer * n_cols * inner overflows");
    hipStream_t st = (hipStream_t)s;
    const int64_t P = outer * inner;
    const int mode = reduction == 'n' ? 0 : reduction == 'm' ? 1 : 2;
    if (dlogp_or_null) {
        const int rc = fill_f32(dlogp_or_null, 0.f, P * n_cols, st);
        if (rc) return rc;
    }
    NllArgs a{logp, labels, class_weight_or_null, mode == 0 ? loss : nullptr, dlogp_or_null, pos_grad_or_null,
              ignore_index, n_cols, inner > 0 ? inner : 1, P, (int)label_bytes};
    if (P <= LL_SMALL) {     // (P == 0: the block writes loss[0] = 0 for 'm' / 's' and nothing else)
        hipLaunchKernelGGL(nll_small_kernel, dim3(1), dim3(1024), 0, st, a, mode, loss);
        NNHIP_LAUNCH_CHECK("nll_small_kernel");
        return 0;
    }
    const bool grads = dlogp_or_null || pos_grad_or_null;
    int64_t blocks = ceil_div(P, 1024);
    if (blocks > 1024) blocks = 1024;
    float* part = nullptr;
    if (mode != 0) {
        part = static_cast<float*>(workspace((size_t)(2 * blocks + 1) * sizeof(float)));
        NNHIP_CHECK_ARG(part != nullptr, NNHIP_ENOMEM, "nnhipNLLLossForwardBackward: workspace allocation failed");
    }
    if (mode != 0 || a.terms) {
        hipLaunchKernelGGL(nll_part_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, part);
        NNHIP_LAUNCH_CHECK("nll_part_kernel");
    }
    if (mode != 0) {
        hipLaunchKernelGGL(nll_final_kernel, dim3(1), dim3(256), 0, st, part, (int)blocks, mode, loss, part + 2 * blocks);
        NNHIP_LAUNCH_CHECK("nll_final_kernel");
    }
    if (grads) {
        a.terms = nullptr;
        hipLaunchKernelGGL(nll_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, mode != 0 ? part + 2 * blocks : nullptr);
        NNHIP_LAUNCH_CHECK("nll_grad_kernel");
    }
    return 0;
}
