// avgpool.hip -- AvgPool2d (neunet/nn/layers/avgpool2d.py:14-46 backward, :126-172 forward) on NCHW fp32.
// The window mean counts the zero padding: out = (sum of the taps inside the image) / (kh kw), always.  No dilation.
// Three tiers, picked on the host by avgpool_tier() (tests/avgpool_ref.py restates it):
//   general  one thread per output (forward) / per input element (backward, a gather over the covering windows): every descriptor.
//   tiles    kernel == stride, no padding, H = Ho kh, W = Wo kw (every 2x2/2 pool): one thread per window -- or per pair of windows at
//            kw = 2 -- no per-pixel division or modulo; 16-byte accesses where the row length AND the base pointers allow them.
//   global   kh = H, kw = W, no padding (Ho = Wo = 1): one wave per (b, c) plane, one 256-thread block per plane above
//            kAvgGlobalWaveMax elements; the backward is a broadcast.
// Every tier sums in a fixed order, scales the sum by a host-computed 1 / (kh kw), writes every element of its output exactly once and
// uses no atomics, memset or workspace: reruns are bit-identical and the launches are legal inside a hipGraph.
// Element offsets: both entries refuse tensors of 2^31 elements or more, so every offset fits 31 bits; the index divisions are 32-bit.
#include <atomic>

#include "common.h"

namespace nnhip {

constexpr int kAvgGlobalWaveMax = 1024;      // planes up to here: one wave each (16 strided loads per lane at most)

// ---- general ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(float* __restrict__ out, const float* __restrict__ x, unsigned total, int H,
                                                          int W, int Ho, int Wo, int kh, int kw, int sh, int sw, int pu, int pl,
                                                          float inv) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned hw = (unsigned)Ho * (unsigned)Wo, bc = i / hw, rem = i - bc * hw;
    const int ho = (int)(rem / (unsigned)Wo), wo = (int)(rem - (unsigned)ho * (unsigned)Wo);
    const float* __restrict__ p = x + (int64_t)bc * H * W;
    // the taps inside the image: rows [y0, y1), columns [x0, x1) -- the padding adds zeros, which are left out
    const int ys = ho * sh - pu, xs = wo * sw - pl;
    const int y0 = ys > 0 ? ys : 0, y1 = ys + kh < H ? ys + kh : H;
    const int x0 = xs > 0 ? xs : 0, x1 = xs + kw < W ? xs + kw : W;
    float s = 0.f;
    for (int y = y0; y < y1; ++y)
        for (int xx = x0; xx < x1; ++xx) s += p[(int64_t)y * W + xx];
    out[i] = s * inv;
}

// dX[y, x] = inv * sum of dY over the windows [ho_lo, ho_hi] x [wo_lo, wo_hi] that cover (y, x); none: +0
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(float* __restrict__ dx, const float* __restrict__ dy, unsigned total, int H,
                                                          int W, int Ho, int Wo, int kh, int kw, int sh, int sw, int pu, int pl,
                                                          float inv) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned hw = (unsigned)H * (unsigned)W, bc = i / hw, rem = i - bc * hw;
    const int y = (int)(rem / (unsigned)W), xx = (int)(rem - (unsigned)y * (unsigned)W);
    const int yp = y + pu, xp = xx + pl;                   // in the padded image: window ho covers rows [ho sh, ho sh + kh)
    const int ho_hi = yp / sh < Ho - 1 ? yp / sh : Ho - 1, wo_hi = xp / sw < Wo - 1 ? xp / sw : Wo - 1;
    const int ho_lo = yp < kh ? 0 : (yp - kh) / sh + 1, wo_lo = xp < kw ? 0 : (xp - kw) / sw + 1;
    const float* __restrict__ g = dy + (int64_t)bc * Ho * Wo;
    float s = 0.f;
    for (int ho = ho_lo; ho <= ho_hi; ++ho)
        for (int wo = wo_lo; wo <= wo_hi; ++wo) s += g[(int64_t)ho * Wo + wo];
    dx[i] = s * inv;
}

// ---- tiles -----------------------------------------------------------------------------------------------------------------
// MODE 0: one window per thread, scalar accesses, any kh x kw.
// MODE 1: kw = 2, W % 4 == 0: one PAIR of adjacent windows per thread -- a float4 of x per row, a float2 of out (x 16-byte, out 8-byte
//         aligned; W % 4 == 0 keeps every row start and every pair on those boundaries).
// MODE 2: kw = 4: one window per thread, a float4 of x per row (x 16-byte aligned; W = 4 Wo).
// `units` = windows (MODE 0, 2) or pairs (MODE 1); upr = units per output row.  The taps are summed in (r, s) order in every mode.
template <int MODE>
__global__ __launch_bounds__(256) void avgpool_fwd_tiles_kernel(float* __restrict__ out, const float* __restrict__ x, unsigned units,
                                                                unsigned upr, int W, int kh, int kw, float inv) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const unsigned row_o = u / upr, col = u - row_o * upr;                // row_o = bc * Ho + ho; H = Ho kh: input row row_o * kh
    const float* __restrict__ p = x + (int64_t)row_o * kh * W;
    if constexpr (MODE == 1) {
        float s0 = 0.f, s1 = 0.f;
        for (int r = 0; r < kh; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(p + (int64_t)r * W + 4 * (int64_t)col);
            s0 += v.x; s0 += v.y;
            s1 += v.z; s1 += v.w;
        }
        *reinterpret_cast<float2*>(out + 2 * (int64_t)u) = make_float2(s0 * inv, s1 * inv);
    } else if constexpr (MODE == 2) {
        float s = 0.f;
        for (int r = 0; r < kh; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(p + (int64_t)r * W + 4 * (int64_t)col);
            s += v.x; s += v.y; s += v.z; s += v.w;
        }
        out[u] = s * inv;
    } else {
        float s = 0.f;
        for (int r = 0; r < kh; ++r)
            for (int c = 0; c < kw; ++c) s += p[(int64_t)r * W + (int64_t)col * kw + c];
        out[u] = s * inv;
    }
}
// the backward writes each window's kh x kw copies of dY * inv (MODE 1: dY 8-byte, dX 16-byte aligned; MODE 2: dX 16-byte aligned)
template <int MODE>
__global__ __launch_bounds__(256) void avgpool_bwd_tiles_kernel(float* __restrict__ dx, const float* __restrict__ dy, unsigned units,
                                                                unsigned upr, int W, int kh, int kw, float inv) {
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const unsigned row_o = u / upr, col = u - row_o * upr;
    float* __restrict__ p = dx + (int64_t)row_o * kh * W;
    if constexpr (MODE == 1) {
        const float2 g = *reinterpret_cast<const float2*>(dy + 2 * (int64_t)u);
        const float4 v = make_float4(g.x * inv, g.x * inv, g.y * inv, g.y * inv);
        for (int r = 0; r < kh; ++r) *reinterpret_cast<float4*>(p + (int64_t)r * W + 4 * (int64_t)col) = v;
    } else if constexpr (MODE == 2) {
        const float g = dy[u] * inv;
        const float4 v = make_float4(g, g, g, g);
        for (int r = 0; r < kh; ++r) *reinterpret_cast<float4*>(p + (int64_t)r * W + 4 * (int64_t)col) = v;
    } else {
        const float g = dy[u] * inv;
        for (int r = 0; r < kh; ++r)
            for (int c = 0; c < kw; ++c) p[(int64_t)r * W + (int64_t)col * kw + c] = g;
    }
}

// ---- global ----------------------------------------------------------------------------------------------------------------
// NW = 1: four independent waves per 256-thread block, one plane each (no barrier: a wave past the last plane just leaves).
// NW = 4: the whole block on one plane.  Lane-strided partial sums, then the fixed-order wave / block reduction of common.h.
template <int NW>
__global__ __launch_bounds__(256) void avgpool_global_fwd_kernel(float* __restrict__ out, const float* __restrict__ x, unsigned planes,
                                                                 int HW, float inv) {
    __shared__ float red[4];
    const unsigned plane = NW == 1 ? blockIdx.x * 4u + (threadIdx.x >> 6) : blockIdx.x;
    if (plane >= planes) return;                                          // wave-uniform (NW = 1) / block-uniform (NW = 4)
    const float* __restrict__ p = x + (int64_t)plane * HW;
    const int t = NW == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    float s = 0.f;
    for (int i = t; i < HW; i += 64 * NW) s += p[i];
    s = block_sum<NW>(s, red);
    if (t == 0) out[plane] = s * inv;
}
template <int NW>
__global__ __launch_bounds__(256) void avgpool_global_bwd_kernel(float* __restrict__ dx, const float* __restrict__ dy, unsigned planes,
                                                                 int HW, float inv) {
    const unsigned plane = NW == 1 ? blockIdx.x * 4u + (threadIdx.x >> 6) : blockIdx.x;
    if (plane >= planes) return;
    float* __restrict__ p = dx + (int64_t)plane * HW;
    const int t = NW == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const float g = dy[plane] * inv;
    for (int i = t; i < HW; i += 64 * NW) p[i] = g;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static std::atomic<int> g_avg_route{NNHIP_AVGPOOL_ROUTE_AUTO};

struct AvgGeom {
    int Ho, Wo;
    int64_t n_in, n_out;
};
constexpr int64_t kAvgLimit = (int64_t)1 << 31;

static int avgpool_check(const char* fn, const nnhipPool2dDesc* d, AvgGeom& g) {
    NNHIP_CHECK_ARG(d != nullptr, NNHIP_EINVAL, "%s: null descriptor", fn);
    NNHIP_CHECK_ARG(d->B >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1 && d->kh >= 1 && d->kw >= 1 && d->sh >= 1 && d->sw >= 1, NNHIP_EINVAL,
                    "%s: a size, kernel or stride extent < 1", fn);
    NNHIP_CHECK_ARG(d->pu >= 0 && d->pd >= 0 && d->pl >= 0 && d->pr >= 0, NNHIP_EINVAL, "%s: negative padding", fn);
    NNHIP_CHECK_ARG((d->dh == 0 || d->dh == 1) && (d->dw == 0 || d->dw == 1), NNHIP_EINVAL, "%s: AvgPool2d has no dilation (dh, dw must be 0 or 1)", fn);
    const int64_t all[] = {d->B, d->C, d->H, d->W, d->kh, d->kw, d->sh, d->sw, d->pu, d->pd, d->pl, d->pr};
    for (int64_t v : all) NNHIP_CHECK_ARG(v < kAvgLimit, NNHIP_EINVAL, "%s: a descriptor field of 2^31 or more", fn);
    const int64_t Hp = d->H + d->pu + d->pd, Wp = d->W + d->pl + d->pr;          // each term < 2^31: no overflow
    NNHIP_CHECK_ARG(Hp >= d->kh && Wp >= d->kw, NNHIP_EINVAL, "%s: the window is larger than the padded input (output extent < 1)", fn);
    const int64_t ho = (Hp - d->kh) / d->sh + 1, wo = (Wp - d->kw) / d->sw + 1;  // avgpool2d.py:118-123
    NNHIP_CHECK_ARG(Hp < kAvgLimit && Wp < kAvgLimit && d->kh * d->kw < kAvgLimit, NNHIP_EINVAL, "%s: a padded extent or window of 2^31 elements or more", fn);
    int64_t n_in = d->B, n_out = d->B;
    const int64_t fin[] = {d->C, d->H, d->W}, fout[] = {d->C, ho, wo};
    for (int k = 0; k < 3; ++k) {
        n_in *= fin[k];
        n_out *= fout[k];
        NNHIP_CHECK_ARG(n_in < kAvgLimit && n_out < kAvgLimit, NNHIP_EINVAL, "%s: an input or output of 2^31 elements or more", fn);
    }
    g.Ho = (int)ho; g.Wo = (int)wo; g.n_in = n_in; g.n_out = n_out;
    return 0;
}

// The tier of a (checked) descriptor.  global before tiles: a window that is the whole plane satisfies both when kernel == stride.
static int avgpool_tier(const nnhipPool2dDesc* d, const AvgGeom& g) {
    if (g_avg_route.load() == NNHIP_AVGPOOL_ROUTE_GENERAL) return NNHIP_AVGPOOL_TIER_GENERAL;
    if (d->pu + d->pd + d->pl + d->pr != 0) return NNHIP_AVGPOOL_TIER_GENERAL;
    if (d->kh == d->H && d->kw == d->W)
        return d->H * d->W <= kAvgGlobalWaveMax ? NNHIP_AVGPOOL_TIER_GLOBAL_WAVE : NNHIP_AVGPOOL_TIER_GLOBAL_BLOCK;
    if (d->kh == d->sh && d->kw == d->sw && d->H == g.Ho * d->kh && d->W == g.Wo * d->kw) return NNHIP_AVGPOOL_TIER_TILES;
    return NNHIP_AVGPOOL_TIER_GENERAL;
}
// tiles: 1 (pairs of 2-wide windows) or 2 (4-wide windows) when the row length and both base pointers allow the 16-byte accesses
static int avgpool_tiles_mode(const nnhipPool2dDesc* d, const void* full, const void* pooled) {
    if (d->kw == 2 && d->W % 4 == 0 && aligned16(full) && aligned8(pooled)) return 1;
    if (d->kw == 4 && aligned16(full)) return 2;
    return 0;
}

template <bool FWD, class TO, class TI>
static int avgpool_launch(const char* fn, TO* dst, TI* src, const nnhipPool2dDesc* d, nnhipStream_t s) {
    AvgGeom g;
    if (int rc = avgpool_check(fn, d, g)) return rc;
    NNHIP_CHECK_ARG(dst && src, NNHIP_EINVAL, "%s: null pointer", fn);
    NNHIP_CHECK_ARG(aligned4(dst) && aligned4(src), NNHIP_EALIGN, "%s: pointer not 4-byte aligned", fn);
    const hipStream_t st = (hipStream_t)s;
    const float inv = 1.0f / (float)(d->kh * d->kw);
    const int H = (int)d->H, W = (int)d->W, kh = (int)d->kh, kw = (int)d->kw;
    const unsigned planes = (unsigned)(d->B * d->C);
    switch (avgpool_tier(d, g)) {
        case NNHIP_AVGPOOL_TIER_GLOBAL_WAVE:
            if constexpr (FWD) hipLaunchKernelGGL(avgpool_global_fwd_kernel<1>, dim3((unsigned)ceil_div(planes, 4)), dim3(256), 0, st, dst, src, planes, H * W, inv);
            else hipLaunchKernelGGL(avgpool_global_bwd_kernel<1>, dim3((unsigned)ceil_div(planes, 4)), dim3(256), 0, st, dst, src, planes, H * W, inv);
            break;
        case NNHIP_AVGPOOL_TIER_GLOBAL_BLOCK:
            if constexpr (FWD) hipLaunchKernelGGL(avgpool_global_fwd_kernel<4>, dim3(planes), dim3(256), 0, st, dst, src, planes, H * W, inv);
            else hipLaunchKernelGGL(avgpool_global_bwd_kernel<4>, dim3(planes), dim3(256), 0, st, dst, src, planes, H * W, inv);
            break;
        case NNHIP_AVGPOOL_TIER_TILES: {
            // the full-resolution tensor is the forward's source and the backward's destination
            const int mode = FWD ? avgpool_tiles_mode(d, src, dst) : avgpool_tiles_mode(d, dst, src);
            const unsigned upr = (unsigned)(mode == 1 ? g.Wo / 2 : g.Wo), units = (unsigned)(mode == 1 ? g.n_out / 2 : g.n_out);
            const dim3 grid((unsigned)ceil_div(units, 256));
#define AVG_TILES(M)                                                                                                                 \
    if constexpr (FWD) hipLaunchKernelGGL(avgpool_fwd_tiles_kernel<M>, grid, dim3(256), 0, st, dst, src, units, upr, W, kh, kw, inv); \
    else hipLaunchKernelGGL(avgpool_bwd_tiles_kernel<M>, grid, dim3(256), 0, st, dst, src, units, upr, W, kh, kw, inv)
            if (mode == 1) { AVG_TILES(1); } else if (mode == 2) { AVG_TILES(2); } else { AVG_TILES(0); }
#undef AVG_TILES
            break;
        }
        default:
            if constexpr (FWD)
                hipLaunchKernelGGL(avgpool_fwd_kernel, dim3((unsigned)ceil_div(g.n_out, 256)), dim3(256), 0, st, dst, src, (unsigned)g.n_out, H, W,
                                   g.Ho, g.Wo, kh, kw, (int)d->sh, (int)d->sw, (int)d->pu, (int)d->pl, inv);
            else
                hipLaunchKernelGGL(avgpool_bwd_kernel, dim3((unsigned)ceil_div(g.n_in, 256)), dim3(256), 0, st, dst, src, (unsigned)g.n_in, H, W,
                                   g.Ho, g.Wo, kh, kw, (int)d->sh, (int)d->sw, (int)d->pu, (int)d->pl, inv);
    }
    NNHIP_LAUNCH_CHECK(fn);
    return 0;
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipAvgPool2dForward(float* out, const float* X, const nnhipPool2dDesc* d, nnhipStream_t s) {
    return avgpool_launch<true>("nnhipAvgPool2dForward", out, X, d, s);
}
extern "C" int nnhipAvgPool2dBackward(float* dX, const float* dY, const nnhipPool2dDesc* d, nnhipStream_t s) {
    return avgpool_launch<false>("nnhipAvgPool2dBackward", dX, dY, d, s);
}
extern "C" int nnhipAvgPool2dTier(const nnhipPool2dDesc* d) {
    AvgGeom g;
    if (int rc = avgpool_check("nnhipAvgPool2dTier", d, g)) return rc;
    return avgpool_tier(d, g);
}
extern "C" int nnhipSetAvgPool2dRoute(int route) {
    if (route != NNHIP_AVGPOOL_ROUTE_AUTO && route != NNHIP_AVGPOOL_ROUTE_GENERAL) return g_avg_route.load();
    return g_avg_route.exchange(route);
}
