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
