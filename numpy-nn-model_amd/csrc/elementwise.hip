// elementwise.hip -- bandwidth-bound elementwise kernels: ReLU, Swish, SwiGLU gate, scale, add.
// All are float4 grid-stride loops (16 B/lane = 1 KiB per wave instruction), capped at 8 blocks/CU,
// with a scalar tail.  sigmoid = v_rcp_f32(1 + v_exp_f32(-x log2 e)): the two hardware transcendentals are
// 1 ulp each, so x*sigmoid(x) stays within ~3 ulp of NumPy's float32 result (tests/test_hip_parity.py sweeps
// [-88, 88]); the library expf + IEEE divide were ~30 VALU instructions per element and made the *simplest*
// kernel of the C3 pass (Swish forward) slower than Softmax forward on the same 268 MB (round-1 VERDICT).
#include <stdlib.h>

#include "ew_map.h"

namespace nnhip {

// f = max(0, x)               (neunet/nn/activations.py:54-56: np.maximum propagates a NaN, fmaxf(NaN, 0) would return 0 and
// hide a diverged activation from everything downstream): one unordered compare, `not (x <= 0)` is true for x > 0 and for NaN
struct ReluF { __device__ float operator()(float x) const { return !(x <= 0.f) ? x : 0.f; } };
// dIn = dOut * (out > 0)      (neunet/nn/activations.py:44-45)
struct ReluB { __device__ float operator()(float dy, float y) const { return y > 0.f ? dy : 0.f; } };
// f = x * sigmoid(beta x)     (neunet/nn/activations.py:225-230)
struct SwishF {
    float beta;
    __device__ float operator()(float x) const { return x * sigmoid_fast_(beta * x); }
};
// dx = dy * (beta f + s (1 - beta f)), s = sigmoid(beta x)   (neunet/nn/activations.py:212-216)
struct SwishB {
    float beta;
    __device__ float operator()(float dy, float x) const {
        const float s = sigmoid_fast_(beta * x);
        const float f = x * s;
        return dy * (beta * f + s * (1.f - beta * f));
    }
};
// GELU, tanh form (neunet/nn/activations.py:412-417): 0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3).  Since
// 0.5 (1 + tanh u) = sigmoid(2u) the kernel evaluates x * sigmoid(2u): one exp2 and one rcp, and no 1 + tanh cancellation
// on the negative side.
constexpr float kGeluK = 0.7978845608028654f, kGeluC = 0.044715f;
struct GeluF {
    __device__ float operator()(float x) const { return x * sigmoid_fast_(2.f * kGeluK * (x + kGeluC * x * x * x)); }
};
// The exact derivative of that form: s + x s (1 - s) 2 du/dx, s = sigmoid(2u), du/dx = sqrt(2/pi) (1 + 3 * 0.044715 x^2).
// (The reference's backward, activations.py:396-401, is the same expression with its constants rounded to six digits.)
struct GeluB {
    __device__ float operator()(float dy, float x) const {
        const float x2 = x * x;
        const float s = sigmoid_fast_(2.f * kGeluK * (x + kGeluC * x2 * x));
        const float t = x * s * (1.f - s);            // exactly 0 once the sigmoid has saturated: skip the polynomial there, whose
        return dy * (t == 0.f ? s : fmaf(t, 2.f * kGeluK * fmaf(3.f * kGeluC, x2, 1.f), s));   // x^2 overflows for |x| > 1.8e19 (0 * inf)
    }
};
// f = tanh(x)                 (neunet/nn/activations.py:118-120)
struct TanhF { __device__ float operator()(float x) const { return tanhf(x); } };
// dIn = dOut * (1 - f^2), f the activation's OUTPUT   (neunet/nn/activations.py:107-110)
struct TanhB { __device__ float operator()(float dy, float f) const { return dy * (1.0f - f * f); } };
// ---- Softplus, Softsign, Mish, TanhExp, ELU, SELU, log (neunet/nn/activations.py:140-194, 250-383; neunet/autograd.py:357) ---------
// The same mathematical functions as the reference's expressions, in forms that stay finite and keep relative accuracy where its
// float32 ones overflow or cancel (include/neunet_hip.h lists them).  Every backward functor reads the forward INPUT.  A NaN input
// gives NaN from every functor: no fmaxf / fminf on the value path (they drop a NaN), and the selects send a NaN down the branch
// that computes with it.
// log(1 + e) for 0 <= e <= 1: log(u) + (e - (u - 1)) / u with u = fl(1 + e) -- the second term puts back what the rounding of 1 + e
// lost (exactly e once u == 1), so the result keeps its relative accuracy down to e = exp(-103)
__device__ __forceinline__ float log1p_unit_(float e) {
    const float u = 1.0f + e;
    return fmaf(e - (u - 1.0f), __builtin_amdgcn_rcpf(u), logf(u));
}
// f = log(1 + exp(x)) = max(x, 0) + log1p(exp(-|x|))   (activations.py:156; |NaN| carries the NaN through the second term)
struct SoftplusF {
    __device__ float operator()(float x) const { return (x > 0.f ? x : 0.f) + log1p_unit_(exp_fast_(-fabsf(x))); }
};
// dx = dy * sigmoid(x)                                 (activations.py:146)
struct SoftplusB { __device__ float operator()(float dy, float x) const { return dy * sigmoid_fast_(x); } };
// f = x / (1 + |x|) ; dx = dy / (1 + |x|)^2            (activations.py:190, 180).  IEEE divisions: 1 + |x| reaches 3.4e38, whose
// hardware reciprocal is a denormal
struct SoftsignF { __device__ float operator()(float x) const { return x / (1.0f + fabsf(x)); } };
struct SoftsignB {
    __device__ float operator()(float dy, float x) const {
        const float r = 1.0f / (1.0f + fabsf(x));
        return dy * (r * r);
    }
};
// Mish: f = x t, t = tanh(softplus(x)) (activations.py:274).  With n = exp(x): tanh(log(1 + n)) = ((1 + n)^2 - 1) / ((1 + n)^2 + 1) =
// p / (p + 2), p = n (n + 2) -- one exp and one reciprocal, no log, no cancellation on either side (t -> n for x -> -inf).  Beyond
// x = 20, p > 2e17 and t is 1 to the last bit (and n^2 would overflow at 44): f = x, f' = 1 there.
// f' = t + x sigmoid(x) (1 - t^2), 1 - t^2 = (1 - t)(1 + t) = 2 (1 + t) / (p + 2), sigmoid(x) = n / (1 + n): the reference's
// backward (activations.py:258-262) is the same derivative written with exp(3x), which overflows at x = 29.6.
struct MishF {
    __device__ float operator()(float x) const {
        if (x > 20.f) return x;
        const float n = exp_fast_(x), p = n * (n + 2.0f);
        return x * (p * __builtin_amdgcn_rcpf(p + 2.0f));
    }
};
struct MishB {
    __device__ float operator()(float dy, float x) const {
        if (x > 20.f) return dy;
        const float n = exp_fast_(x), p = n * (n + 2.0f);
        const float rq = __builtin_amdgcn_rcpf(p + 2.0f), t = p * rq;
        const float sg = n * __builtin_amdgcn_rcpf(1.0f + n);
        return dy * fmaf(x * sg, 2.0f * rq * (1.0f + t), t);
    }
};
// TanhExp: f = x t, t = tanh(exp(x)) (activations.py:312); f' = t + x exp(x) (1 - t^2) (activations.py:301), with
// 1 - t^2 = 4 q / (1 + q)^2, q = exp(-2 exp(x)) (no cancellation).  Above x = 88.7 exp(x) is inf and 1 - t^2 is 0: the second term
// is exactly 0 from the moment 1 - t^2 is (x > ~3.9), so it is skipped there instead of forming inf * 0.
struct TanhExpF { __device__ float operator()(float x) const { return x * tanhf(exp_fast_(x)); } };
struct TanhExpB {
    __device__ float operator()(float dy, float x) const {
        const float n = exp_fast_(x), t = tanhf(n);
        const float q = exp_fast_(-2.0f * n), r = __builtin_amdgcn_rcpf(1.0f + q);
        const float omt2 = 4.0f * q * r * r;
        return dy * (omt2 == 0.f ? t : fmaf(x * n, omt2, t));
    }
};
// ELU: f = x <= 0 ? alpha (exp(x) - 1) : x (activations.py:349), expm1 instead of the cancelling exp(x) - 1;
// f' = x <= 0 ? alpha exp(x) : 1 (activations.py:337 forms it as alpha + f, which cancels for alpha != 1).  f'(0) = alpha.
struct EluF {
    float alpha;
    __device__ float operator()(float x) const { return x <= 0.f ? alpha * expm1f(x) : x; }
};
struct EluB {
    float alpha;
    __device__ float operator()(float dy, float x) const { return x > 0.f ? dy : dy * (alpha * exp_fast_(x)); }
};
// SELU: f = lambda (x > 0 ? x : a (exp(x) - 1)) ; f' = lambda (x > 0 ? 1 : a exp(x))   (activations.py:372-378, 363); f'(0) = lambda a
constexpr float kSeluAlpha = 1.6732632423543772848170429916717f, kSeluLambda = 1.0507009873554804934193349852946f;
struct SeluF { __device__ float operator()(float x) const { return kSeluLambda * (x > 0.f ? x : kSeluAlpha * expm1f(x)); } };
struct SeluB {
    __device__ float operator()(float dy, float x) const { return dy * (kSeluLambda * (x > 0.f ? 1.0f : kSeluAlpha * exp_fast_(x))); }
};
// Tensor.log (neunet/autograd.py:357): f = log(x), literally (log(0) = -inf, a negative x gives NaN) ; dx = dy / x
struct LogF { __device__ float operator()(float x) const { return logf(x); } };
struct LogB { __device__ float operator()(float dy, float x) const { return dy / x; } };
// Tensor.exp / sqrt / sin / cos / abs (neunet/autograd.py:339-440, 610-626): the library functions, literally; every backward
// functor reads the forward INPUT.  sqrt' is the reference's 0.5 x^-0.5 (inf at 0, NaN below), abs' is sign(x) (0 at 0, as np.sign)
struct ExpF { __device__ float operator()(float x) const { return expf(x); } };
struct ExpB { __device__ float operator()(float dy, float x) const { return dy * expf(x); } };
struct SqrtF { __device__ float operator()(float x) const { return sqrtf(x); } };
struct SqrtB { __device__ float operator()(float dy, float x) const { return dy * 0.5f / sqrtf(x); } };
struct SinF { __device__ float operator()(float x) const { return sinf(x); } };
struct SinB { __device__ float operator()(float dy, float x) const { return dy * cosf(x); } };
struct CosF { __device__ float operator()(float x) const { return cosf(x); } };
struct CosB { __device__ float operator()(float dy, float x) const { return dy * -sinf(x); } };
struct AbsF { __device__ float operator()(float x) const { return fabsf(x); } };
struct AbsB { __device__ float operator()(float dy, float x) const { return dy * (x > 0.f ? 1.f : (x < 0.f ? -1.f : (x == x ? 0.f : x))); } };
struct ScaleF {
    float alpha;
    __device__ float operator()(float x) const { return alpha * x; }
};

// SwiGLU gate.  in rows = [gate(h) | up(h)] (width 2h), out rows width h.
// (fused_swish_and_mul.cu:13-57 semantics; oracle = Swish(gate)*up on the reference tape)
template <bool VEC>
__global__ __launch_bounds__(EW_THREADS) void swiglu_fwd_kernel(float* __restrict__ out,
                                                                const float* __restrict__ in,
                                                                float beta, int64_t h, int64_t size) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    if constexpr (VEC) {  // h % 4 == 0
        const int64_t hv = h >> 2, nv = size >> 2;
        for (int64_t i = gid; i < nv; i += gsz) {
            const int64_t row = i / hv, c = i - row * hv;
            const float4 g = reinterpret_cast<const float4*>(in)[row * 2 * hv + c];
            const float4 u = reinterpret_cast<const float4*>(in)[row * 2 * hv + hv + c];
            float4 y;
            y.x = g.x * sigmoid_fast_(beta * g.x) * u.x;
            y.y = g.y * sigmoid_fast_(beta * g.y) * u.y;
            y.z = g.z * sigmoid_fast_(beta * g.z) * u.z;
            y.w = g.w * sigmoid_fast_(beta * g.w) * u.w;
            reinterpret_cast<float4*>(out)[i] = y;
        }
    } else {
        for (int64_t i = gid; i < size; i += gsz) {
            const int64_t row = i / h, c = i - row * h;
            const float g = in[row * 2 * h + c], u = in[row * 2 * h + h + c];
            out[i] = g * sigmoid_fast_(beta * g) * u;
        }
    }
}

__device__ __forceinline__ void swiglu_bwd1(float dy, float g, float u, float beta, float& dg,
                                            float& du) {
    const float s = sigmoid_fast_(beta * g);
    const float f = g * s;
    du = dy * f;
    dg = dy * u * (beta * f + s * (1.f - beta * f));
}

template <bool VEC>
__global__ __launch_bounds__(EW_THREADS) void swiglu_bwd_kernel(float* __restrict__ din,
                                                                const float* __restrict__ dout,
                                                                const float* __restrict__ in,
                                                                float beta, int64_t h, int64_t size) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    if constexpr (VEC) {
        const int64_t hv = h >> 2, nv = size >> 2;
        for (int64_t i = gid; i < nv; i += gsz) {
            const int64_t row = i / hv, c = i - row * hv;
            const float4 g = reinterpret_cast<const float4*>(in)[row * 2 * hv + c];
            const float4 u = reinterpret_cast<const float4*>(in)[row * 2 * hv + hv + c];
            const float4 dy = reinterpret_cast<const float4*>(dout)[i];
            float4 dg, du;
            swiglu_bwd1(dy.x, g.x, u.x, beta, dg.x, du.x);
            swiglu_bwd1(dy.y, g.y, u.y, beta, dg.y, du.y);
            swiglu_bwd1(dy.z, g.z, u.z, beta, dg.z, du.z);
            swiglu_bwd1(dy.w, g.w, u.w, beta, dg.w, du.w);
            reinterpret_cast<float4*>(din)[row * 2 * hv + c] = dg;
            reinterpret_cast<float4*>(din)[row * 2 * hv + hv + c] = du;
        }
    } else {
        for (int64_t i = gid; i < size; i += gsz) {
            const int64_t row = i / h, c = i - row * h;
            float dg, du;
            swiglu_bwd1(dout[i], in[row * 2 * h + c], in[row * 2 * h + h + c], beta, dg, du);
            din[row * 2 * h + c] = dg;
            din[row * 2 * h + h + c] = du;
        }
    }
}

struct FillF {
    float v;
    __device__ float operator()(float) const { return v; }
};
int fill_f32(float* p, float v, int64_t n, hipStream_t st) {
    if (n <= 0) return 0;
    if (!p) { set_last_error("fill_f32: null pointer"); return NNHIP_EINVAL; }
    return launch_map1(p, p, n, FillF{v}, st, "fill");
}

// internal: used by linear.hip for dZ = dY * swish'(z), in place over z
int mul_f32(float* out, const float* a, const float* b, int64_t n, hipStream_t st) { return launch_map2(out, a, b, n, MulF{}, st, "mul"); }
int swish_backward_inplace(float* z_inout, const float* dY, float beta, int64_t n, hipStream_t st) {
    return launch_map2(z_inout, dY, z_inout, n, SwishB{beta}, st, "swish_backward(inplace)");
}

}  // namespace nnhip

using namespace nnhip;

#define NNHIP_PTRS(fn, ...)                                                        \
    do {                                                                           \
        const void* _ps[] = {__VA_ARGS__};                                         \
        for (const void* _p : _ps) {                                               \
            NNHIP_CHECK_ARG(_p != nullptr, NNHIP_EINVAL, fn ": null pointer");      \
            NNHIP_CHECK_ARG(aligned4(_p), NNHIP_EALIGN, fn ": misaligned pointer"); \
        }                                                                          \
    } while (0)

extern "C" int nnhipReLUForward(float* out, const float* in, int64_t size, nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipReLUForward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipReLUForward", out, in);
    return launch_map1(out, in, size, ReluF{}, (hipStream_t)s, "relu_forward");
}
extern "C" int nnhipReLUBackward(float* dIn, const float* dOut, const float* out, int64_t size,
                                 nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipReLUBackward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipReLUBackward", dIn, dOut, out);
    return launch_map2(dIn, dOut, out, size, ReluB{}, (hipStream_t)s, "relu_backward");
}
extern "C" int nnhipSwishForward(float* out, const float* in, float beta, int64_t size,
                                 nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipSwishForward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipSwishForward", out, in);
    return launch_map1(out, in, size, SwishF{beta}, (hipStream_t)s, "swish_forward");
}
extern "C" int nnhipSwishBackward(float* dIn, const float* dOut, const float* in, float beta,
                                  int64_t size, nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipSwishBackward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipSwishBackward", dIn, dOut, in);
    return launch_map2(dIn, dOut, in, size, SwishB{beta}, (hipStream_t)s, "swish_backward");
}
extern "C" int nnhipGELUForward(float* out, const float* in, int64_t size, nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipGELUForward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipGELUForward", out, in);
    return launch_map1(out, in, size, GeluF{}, (hipStream_t)s, "gelu_forward");
}
extern "C" int nnhipGELUBackward(float* dIn, const float* dOut, const float* in, int64_t size, nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipGELUBackward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipGELUBackward", dIn, dOut, in);
    return launch_map2(dIn, dOut, in, size, GeluB{}, (hipStream_t)s, "gelu_backward");
}
extern "C" int nnhipTanhForward(float* out, const float* in, int64_t size, nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipTanhForward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipTanhForward", out, in);
    return launch_map1(out, in, size, TanhF{}, (hipStream_t)s, "tanh_forward");
}
extern "C" int nnhipTanhBackward(float* dIn, const float* dOut, const float* out, int64_t size, nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipTanhBackward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipTanhBackward", dIn, dOut, out);
    return launch_map2(dIn, dOut, out, size, TanhB{}, (hipStream_t)s, "tanh_backward");
}
// kinds 0..6 (ABI 222) and 8..12 (ABI 223: the Tensor maps); 7 is not assigned
static bool act_kind_ok(int kind) { return (kind >= NNHIP_ACT_SOFTPLUS && kind <= NNHIP_ACT_LOG) || (kind >= NNHIP_ACT_EXP && kind <= NNHIP_ACT_ABS); }
extern "C" int nnhipActivationForward(int kind, float* out, const float* in, float alpha, int64_t size, nnhipStream_t s) {
    NNHIP_CHECK_ARG(act_kind_ok(kind), NNHIP_EINVAL, "nnhipActivationForward: unknown kind %d", kind);
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipActivationForward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipActivationForward", out, in);
    hipStream_t st = (hipStream_t)s;
    switch (kind) {
        case NNHIP_ACT_SOFTPLUS: return launch_map1(out, in, size, SoftplusF{}, st, "softplus_forward");
        case NNHIP_ACT_SOFTSIGN: return launch_map1(out, in, size, SoftsignF{}, st, "softsign_forward");
        case NNHIP_ACT_MISH: return launch_map1(out, in, size, MishF{}, st, "mish_forward");
        case NNHIP_ACT_TANHEXP: return launch_map1(out, in, size, TanhExpF{}, st, "tanhexp_forward");
        case NNHIP_ACT_ELU: return launch_map1(out, in, size, EluF{alpha}, st, "elu_forward");
        case NNHIP_ACT_SELU: return launch_map1(out, in, size, SeluF{}, st, "selu_forward");
        case NNHIP_ACT_EXP: return launch_map1(out, in, size, ExpF{}, st, "exp_forward");
        case NNHIP_ACT_SQRT: return launch_map1(out, in, size, SqrtF{}, st, "sqrt_forward");
        case NNHIP_ACT_SIN: return launch_map1(out, in, size, SinF{}, st, "sin_forward");
        case NNHIP_ACT_COS: return launch_map1(out, in, size, CosF{}, st, "cos_forward");
        case NNHIP_ACT_ABS: return launch_map1(out, in, size, AbsF{}, st, "abs_forward");
        default: return launch_map1(out, in, size, LogF{}, st, "log_forward");
    }
}
extern "C" int nnhipActivationBackward(int kind, float* dIn, const float* dOut, const float* in, float alpha, int64_t size,
                                       nnhipStream_t s) {
    NNHIP_CHECK_ARG(act_kind_ok(kind), NNHIP_EINVAL, "nnhipActivationBackward: unknown kind %d", kind);
    NNHIP_CHECK_ARG(size >= 0, NNHIP_EINVAL, "nnhipActivationBackward: negative size");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipActivationBackward", dIn, dOut, in);
    hipStream_t st = (hipStream_t)s;
    switch (kind) {
        case NNHIP_ACT_SOFTPLUS: return launch_map2(dIn, dOut, in, size, SoftplusB{}, st, "softplus_backward");
        case NNHIP_ACT_SOFTSIGN: return launch_map2(dIn, dOut, in, size, SoftsignB{}, st, "softsign_backward");
        case NNHIP_ACT_MISH: return launch_map2(dIn, dOut, in, size, MishB{}, st, "mish_backward");
        case NNHIP_ACT_TANHEXP: return launch_map2(dIn, dOut, in, size, TanhExpB{}, st, "tanhexp_backward");
        case NNHIP_ACT_ELU: return launch_map2(dIn, dOut, in, size, EluB{alpha}, st, "elu_backward");
        case NNHIP_ACT_SELU: return launch_map2(dIn, dOut, in, size, SeluB{}, st, "selu_backward");
        case NNHIP_ACT_EXP: return launch_map2(dIn, dOut, in, size, ExpB{}, st, "exp_backward");
        case NNHIP_ACT_SQRT: return launch_map2(dIn, dOut, in, size, SqrtB{}, st, "sqrt_backward");
        case NNHIP_ACT_SIN: return launch_map2(dIn, dOut, in, size, SinB{}, st, "sin_backward");
        case NNHIP_ACT_COS: return launch_map2(dIn, dOut, in, size, CosB{}, st, "cos_backward");
        case NNHIP_ACT_ABS: return launch_map2(dIn, dOut, in, size, AbsB{}, st, "abs_backward");
        default: return launch_map2(dIn, dOut, in, size, LogB{}, st, "log_backward");
    }
}
extern "C" int nnhipFusedSwishAndMul(float* out, const float* in, float beta, int64_t hidden,
                                     int64_t size, nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0 && hidden > 0 && size % hidden == 0, NNHIP_EINVAL,
                    "nnhipFusedSwishAndMul: size must be a non-negative multiple of hidden > 0");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipFusedSwishAndMul", out, in);
    const bool vec = (hidden % 4 == 0) && aligned16(out) && aligned16(in);
    if (vec)
        hipLaunchKernelGGL(swiglu_fwd_kernel<true>, dim3(ew_blocks(size >> 2)), dim3(EW_THREADS), 0,
                           (hipStream_t)s, out, in, beta, hidden, size);
    else
        hipLaunchKernelGGL(swiglu_fwd_kernel<false>, dim3(ew_blocks(size)), dim3(EW_THREADS), 0,
                           (hipStream_t)s, out, in, beta, hidden, size);
    NNHIP_LAUNCH_CHECK("swiglu_fwd_kernel");
    return 0;
}
extern "C" int nnhipFusedSwishAndMulBackward(float* dIn, const float* dOut, const float* in,
                                             float beta, int64_t hidden, int64_t size,
                                             nnhipStream_t s) {
    NNHIP_CHECK_ARG(size >= 0 && hidden > 0 && size % hidden == 0, NNHIP_EINVAL,
                    "nnhipFusedSwishAndMulBackward: size must be a non-negative multiple of hidden > 0");
    if (size == 0) return 0;
    NNHIP_PTRS("nnhipFusedSwishAndMulBackward", dIn, dOut, in);
    const bool vec = (hidden % 4 == 0) && aligned16(dIn) && aligned16(dOut) && aligned16(in);
    if (vec)
        hipLaunchKernelGGL(swiglu_bwd_kernel<true>, dim3(ew_blocks(size >> 2)), dim3(EW_THREADS), 0,
                           (hipStream_t)s, dIn, dOut, in, beta, hidden, size);
    else
        hipLaunchKernelGGL(swiglu_bwd_kernel<false>, dim3(ew_blocks(size)), dim3(EW_THREADS), 0,
                           (hipStream_t)s, dIn, dOut, in, beta, hidden, size);
    NNHIP_LAUNCH_CHECK("swiglu_bwd_kernel");
    return 0;
}
// ---- Dropout (neunet/nn/layers/dropout.py:17-37): out = in * mask, mask = Bernoulli(1 - p) / (1 - p) -------------------------
// The mask is a counter-based hash of (seed [+ a device word], element index) -- the same construction as the fused
// attention's dropout (attention.hip: at_hash) -- so it is never stored: the backward pass calls the same entry with the
// upstream gradient as `in` and gets dX = dY * mask.  `seed_dev` (optional device uint32, e.g. the optimizer's step
// counter) is added to the seed inside the kernel: a captured hipGraph then draws a fresh mask on every replay.
// The reference draws its mask with the host NumPy RNG: streams cannot match, parity is tested with injected masks
// (nnhipMul) and statistically (keep rate, scale, forward/backward consistency).
__global__ __launch_bounds__(256) void dropout_hash_kernel(float* __restrict__ out, const float* __restrict__ in, int64_t n,
                                                           unsigned seed, const unsigned* __restrict__ seed_dev, unsigned threshold,
                                                           float scale, bool vec) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, gsz = (int64_t)gridDim.x * 256;
    const unsigned sd = (seed + (seed_dev ? __hip_atomic_load(seed_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u)) * 0x85EBCA6Bu + 0x9E3779B9u;
    auto keep = [&](int64_t i) {
        unsigned x = sd ^ ((unsigned)i * 0x9E3779B1u) ^ ((unsigned)(i >> 32) * 0xC2B2AE35u);
        x ^= x >> 16; x *= 0x7FEB352Du;
        x ^= x >> 15; x *= 0x846CA68Bu;
        x ^= x >> 16;
        return x >= threshold ? scale : 0.f;
    };
    if (vec) {
        const int64_t nv = n >> 2;
        for (int64_t i = gid; i < nv; i += gsz) {
            const float4 x = reinterpret_cast<const float4*>(in)[i];
            reinterpret_cast<float4*>(out)[i] = make_float4(x.x * keep(4 * i), x.y * keep(4 * i + 1), x.z * keep(4 * i + 2), x.w * keep(4 * i + 3));
        }
        for (int64_t i = (nv << 2) + gid; i < n; i += gsz) out[i] = in[i] * keep(i);
    } else {
        for (int64_t i = gid; i < n; i += gsz) out[i] = in[i] * keep(i);
    }
}
extern "C" int nnhipDropout(float* out, const float* in, int64_t n, float p, uint32_t seed, const uint32_t* seed_dev,
                            nnhipStream_t s) {
    NNHIP_CHECK_ARG(n >= 0 && p >= 0.f && p <= 1.f, NNHIP_EINVAL, "nnhipDropout: need n >= 0 and 0 <= p <= 1");
    if (n == 0) return 0;
    NNHIP_PTRS("nnhipDropout", out, in);
    const double th = (double)p * 4294967296.0;
    const unsigned threshold = (unsigned)(th < 4294967295.0 ? th : 4294967295.0);
    const float scale = p < 1.f ? 1.0f / (1.0f - p) : 0.f;
    const bool vec = aligned16(out) && aligned16(in);
    hipLaunchKernelGGL(dropout_hash_kernel, dim3(ew_blocks(vec ? (n >> 2) + 1 : n)), dim3(EW_THREADS), 0, (hipStream_t)s, out, in, n,
                       (unsigned)seed, reinterpret_cast<const unsigned*>(seed_dev), threshold, scale, vec);
    NNHIP_LAUNCH_CHECK("dropout_hash_kernel");
    return 0;
}
__global__ void increment_u32_kernel(unsigned* p, unsigned by) { *p += by; }
extern "C" int nnhipIncrementU32(uint32_t* word, uint32_t by, nnhipStream_t s) {
    NNHIP_CHECK_ARG(word != nullptr, NNHIP_EINVAL, "nnhipIncrementU32: null pointer");
    hipLaunchKernelGGL(increment_u32_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, reinterpret_cast<unsigned*>(word), (unsigned)by);
    NNHIP_LAUNCH_CHECK("increment_u32_kernel");
    return 0;
}
extern "C" int nnhipScale(float* x, float alpha, int64_t n, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n >= 0, NNHIP_EINVAL, "nnhipScale: negative size");
    if (n == 0) return 0;
    NNHIP_PTRS("nnhipScale", x);
    return launch_map1(x, x, n, ScaleF{alpha}, (hipStream_t)s, "scale");
}
// out[r, c] = in[r, c] * scale[r * scale_stride]: the product with an upstream gradient that a loss node's backward forms
// (cross_entropy.py:111-114 `grad_y_pred * grad`, losses.py:9-22): scale_stride = 0 -- one DEVICE scalar (loss.backward(g) on a
// reduced loss), 1 -- one factor per row (reduction 'none').  One thread per element.
__global__ __launch_bounds__(256) void scale_rows_kernel(float* __restrict__ out, const float* __restrict__ in, const float* __restrict__ scale,
                                                         int64_t rows, int64_t cols, int64_t scale_stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    out[i] = in[i] * scale[(i / cols) * scale_stride];
}
extern "C" int nnhipScaleRows(float* out, const float* in, const float* scale, int64_t rows, int64_t cols, int64_t scale_stride, nnhipStream_t s) {
    NNHIP_CHECK_ARG(rows >= 0 && cols >= 0 && (scale_stride == 0 || scale_stride == 1), NNHIP_EINVAL, "nnhipScaleRows: bad sizes");
    if (rows * cols == 0) return 0;
    NNHIP_PTRS("nnhipScaleRows", out, in, scale);
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)ceil_div(rows * cols, 256)), dim3(256), 0, (hipStream_t)s, out, in, scale, rows, cols,
                       scale_stride);
    NNHIP_LAUNCH_CHECK("scale_rows_kernel");
    return 0;
}
extern "C" int nnhipAdd(float* out, const float* a, const float* b, int64_t n, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n >= 0, NNHIP_EINVAL, "nnhipAdd: negative size");
    if (n == 0) return 0;
    NNHIP_PTRS("nnhipAdd", out, a, b);
    return launch_map2(out, a, b, n, AddF{}, (hipStream_t)s, "add");
}
extern "C" int nnhipMul(float* out, const float* a, const float* b, int64_t n, nnhipStream_t s) {
    NNHIP_CHECK_ARG(n >= 0, NNHIP_EINVAL, "nnhipMul: negative size");
    if (n == 0) return 0;
    NNHIP_PTRS("nnhipMul", out, a, b);
    return launch_map2(out, a, b, n, MulF{}, (hipStream_t)s, "mul");
}
