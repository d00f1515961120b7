// conv_transpose.hip -- ConvTranspose2d: entry points, the stride-phase forward kernel, and the small kernels of its backward.
// CPU semantics: neunet/nn/layers/convtranspose2d.py:249-262 (output size), :293-384 (forward: the weight [out][in][kh][kw],
// NOT flipped, correlated with the zero-stuffed, edge-padded, cropped input) and :16-120 (backward).  In closed form
//     O[b,o,y,x] = bias[o] + sum_{i,k,l} W[o,i,k,l] X[b,i,h,w],   h sh = y + pu - (kh-1-k) dh,   w sw = x + pl - (kw-1-l) dw
// over the terms whose divisions are exact and whose (h, w) lie inside the input.  With r = kh-1-k, s = kw-1-l this is the input
// gradient of the "mirrored" Conv2d (conv_common.h) -- three routes compute it:
//   conv2d : stride 1 and padding <= d (k-1): it IS a Conv2d of the same weight with padding d (k-1) - p (+ output padding at the
//            bottom / right); forward and all three gradients go to nnhipConv2d*, with every kernel tier those have.
//   gather : conv_tap_kernel<DGRAD> (conv_mfma.hip): every tap for every output pixel, the buffer load returning 0 where
//            (y + pu - r dh) is no multiple of the stride.  Handles every descriptor; at stride s only 1 / (sh sw) of its MFMAs
//            multiply anything.
//   phase  : conv_phase_kernel below.  The output pixels with ((y + pu) mod sh, (x + pl) mod sw) = (py, px) form a dense grid
//            that exactly the taps with r dh = py (mod sh), s dw = px (mod sw) reach: per phase a dense implicit GEMM over its own
//            taps, the same pipeline as conv_tap_kernel with a block-uniform tap list.
// Backward at stride > 1: dX is the strided Conv2d forward of dO (conv_tap_kernel<forward>), dW the Conv2d weight gradient with dO
// in the input role and X in the output-gradient role (conv_wgrad_mfma_kernel) followed by a tap-flip / (in, out) transpose, db a
// per-channel sum.  Everything is deterministic; dW / db are written, not accumulated.
#include <atomic>

#include "conv_tap.h"

namespace nnhip {

// =================================================================================================================================
// The phase kernel.  GEMM rows = output channels m, columns = (image, yq, xq) of ONE phase (blockIdx.y) with y = yf + yq sh,
// x = xf + xq sw; reduction = (tap of the phase, input channel), tap outermost.  The repacked weights are conv_repack's
// [tap][Mp][Csp] with tap = r kw + s: every tap belongs to exactly one phase, so the phase's own taps are a strided subset of that
// operand (r = r0 + jr rstep, s = s0 + js sstep) and no per-phase copy is needed.
// A phase without taps (stride > kernel, or gcd(d, s) > 1) has no k-tile: its pixels get bias (or 0).
// =================================================================================================================================
struct ConvPhaseArgs {
    const float* Wr;     // [kh*kw][Mp][Csp]
    const float* Src;    // X [B][Cs][Hs][Ws]
    const float* bias;   // [M] or null
    float* Dst;          // O [B][M][Hd][Wd]
    int B, M, Mp, Cs, Csp, Hs, Ws, Hd, Wd, kh, kw;
    int sh, sw, dh, dw, pu, pl;
    int rstep, sstep;    // sh / gcd(dh, sh), sw / gcd(dw, sw): distance between two taps of one phase
    int tiles_m;         // gridDim.x = tiles_m * (pixel tiles of the largest phase); gridDim.y = sh * sw
};

// the phase's first output coordinate and its number of coordinates along one axis
__host__ __device__ inline void phase_axis(int p, int pad, int stride, int out, int& first, int& count) {
    first = ((p - pad) % stride + stride) % stride;
    count = first < out ? (out - 1 - first) / stride + 1 : 0;
}
// the phase's first tap along one axis (k: none) and its number of taps: r d = p (mod stride), r = r0, r0 + step, ...
__host__ __device__ inline void phase_taps(int p, int d, int stride, int step, int k, int& r0, int& count) {
    r0 = k;
    const int lim = k < stride ? k : stride;             // the residues of r d repeat with period `step` <= stride
    for (int r = 0; r < lim; ++r)
        if ((int)(((int64_t)r * d) % stride) == p) { r0 = r; break; }
    count = r0 < k ? (k - 1 - r0) / step + 1 : 0;
}

template <int WM>
__global__ __launch_bounds__(256, WM == 2 ? 2 : 3) void conv_phase_kernel(const ConvPhaseArgs a) {
    using C = TapCfg<WM>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / C::WN, wn = wave % C::WN, l31 = lane & 31, lh = lane >> 5;
    // ---- this block's phase (uniform) ------------------------------------------------------------------------------------------------
    const int py = (int)blockIdx.y / a.sw, pxp = (int)blockIdx.y - py * a.sw;
    int yf, nyq, xf, nxq;
    phase_axis(py, a.pu, a.sh, a.Hd, yf, nyq);
    phase_axis(pxp, a.pl, a.sw, a.Wd, xf, nxq);
    const int HWq = nyq * nxq;
    const int64_t N = (int64_t)a.B * HWq;                                // the phase's GEMM columns
    const int tm = (int)blockIdx.x % a.tiles_m, tn = (int)blockIdx.x / a.tiles_m;   // m fastest: neighbours share source pixels
    const int m0 = tm * C::BM;
    const int64_t n0 = (int64_t)tn * C::BN;
    if (n0 >= N) return;                                                 // a smaller phase than the grid was sized for (block-uniform)
    int r0, nr, s0, ns;
    phase_taps(py, a.dh, a.sh, a.rstep, a.kh, r0, nr);
    phase_taps(pxp, a.dw, a.sw, a.sstep, a.kw, s0, ns);
    const int nt = nr * ns;
    const int HWs = a.Hs * a.Ws;
    const unsigned HWs4 = (unsigned)HWs * 4u;

    // ---- B side: this thread gathers ONE output pixel of the phase, KPT consecutive source channels per tile ------------------------
    const int px = tid % C::BN;
    const int khalf = __builtin_amdgcn_readfirstlane(tid / C::BN);
    const int64_t n = n0 + px;
    const bool n_ok = n < N;
    int b = 0, yq = 0, xq = 0;
    if (n_ok) {
        b = (int)(n / HWq);
        const int rem = (int)(n - (int64_t)b * HWq);
        yq = rem / nxq;
        xq = rem - yq * nxq;
    }
    const int y0 = yf + yq * a.sh + a.pu, x0 = xf + xq * a.sw + a.pl;     // = py (mod sh), px (mod sw)
    const unsigned img = (unsigned)b * (unsigned)a.Cs * (unsigned)HWs;
    // tap j of the phase (uniform): its index in Wr, and this pixel's source element -- the divisions are exact by construction,
    // so the border check is all that is left
    auto tap_index = [&](int j) -> int {
        if (j >= nt) return 0;
        const int jr = j / ns;
        return (r0 + jr * a.rstep) * a.kw + s0 + (j - jr * ns) * a.sstep;
    };
    auto tap_voff = [&](int j) -> unsigned {
        if (j >= nt) return CV_SENT;
        const int jr = j / ns;
        const int ty = y0 - (r0 + jr * a.rstep) * a.dh, tx = x0 - (s0 + (j - jr * ns) * a.sstep) * a.dw;
        const int ys = ty / a.sh, xs = tx / a.sw;
        const bool ok = n_ok && ty >= 0 && tx >= 0 && ys < a.Hs && xs < a.Ws;
        return ok ? (img + (unsigned)(ys * a.Ws + xs)) * 4u : CV_SENT;
    };
    const __amdgpu_buffer_rsrc_t rsB = conv_rsrc(a.Src, (int64_t)a.B * a.Cs * HWs * 4);
    const int sB = px * C::ALD + khalf * C::KPT;

    // ---- A side: NVA float4 of the repacked weights per tile -------------------------------------------------------------------------
    const __amdgpu_buffer_rsrc_t rsA = conv_rsrc(a.Wr, (int64_t)a.kh * a.kw * a.Mp * a.Csp * 4);
    unsigned voffA[C::NVA];
    int sA[C::NVA];
#pragma unroll
    for (int p = 0; p < C::NVA; ++p) {
        const int idx = tid + 256 * p, rr = idx / (C::BK / 4), k4 = (idx % (C::BK / 4)) * 4;
        voffA[p] = (unsigned)(rr * a.Csp + k4) * 4u;
        sA[p] = rr * C::ALD + k4;
    }
    const unsigned tapstrideA = (unsigned)a.Mp * (unsigned)a.Csp * 4u;
    const unsigned rowA = (unsigned)m0 * (unsigned)a.Csp * 4u;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // fetch state: the tile to be fetched NEXT is (tap ftap of the phase, channels fc0 ...); it runs two tiles ahead of the multiply.
    // Past the last tap the gather reads nothing and the weight loads stay on tap 0 (fetched, never multiplied).
    const int ctiles = a.Csp / C::BK;
    const int T = nt * ctiles;
    int ftap = 0, fc0 = 0;
    unsigned fvoff = tap_voff(0), fsoff = (unsigned)tap_index(0) * tapstrideA + rowA;
    auto advance = [&]() {
        fc0 += C::BK;
        if (fc0 >= a.Csp) {
            fc0 = 0;
            ++ftap;
            fvoff = tap_voff(ftap);
            fsoff = (unsigned)tap_index(ftap) * tapstrideA + rowA;
        }
    };
    float4 ra[C::NVA], ra2[C::NVA];
    float rb[16], rb2[16];
    auto fetch = [&](float4 (&fa)[C::NVA], float (&fb)[16]) {
        const unsigned soffA = fsoff + (unsigned)fc0 * 4u;
        const int cbase = fc0 + khalf * C::KPT;
#pragma unroll
        for (int p = 0; p < C::NVA; ++p) fa[p] = bload4(rsA, voffA[p], soffA);
#pragma unroll
        for (int j = 0; j < C::KPT; ++j) fb[j] = bload1(rsB, cbase + j < a.Cs ? fvoff : CV_SENT, (unsigned)(cbase + j) * HWs4);
    };
    fetch(ra, rb);
    advance();
#pragma unroll
    for (int p = 0; p < C::NVA; ++p) *reinterpret_cast<float4*>(&smem[sA[p]]) = ra[p];
#pragma unroll
    for (int j = 0; j < C::KPT; j += 4) *reinterpret_cast<float4*>(&smem[C::A_SIZE + sB + j]) = make_float4(rb[j], rb[j + 1], rb[j + 2], rb[j + 3]);
    fetch(ra, rb);
    advance();
    __syncthreads();
    int t = 0;
    for (; t + 1 < T; t += 2) {
        tap_k_step<WM>(acc, ra2, rb2, ra, rb, smem, 0, rsA, rsB, voffA, fsoff + (unsigned)fc0 * 4u, fvoff, fc0 + khalf * C::KPT, a.Cs, HWs4, sA,
                       sB, wm, wn, l31, lh);
        advance();
        tap_k_step<WM>(acc, ra, rb, ra2, rb2, smem, 1, rsA, rsB, voffA, fsoff + (unsigned)fc0 * 4u, fvoff, fc0 + khalf * C::KPT, a.Cs, HWs4, sA,
                       sB, wm, wn, l31, lh);
        advance();
    }
    if (t < T) {
        tap_k_step<WM>(acc, ra2, rb2, ra, rb, smem, 0, rsA, rsB, voffA, fsoff + (unsigned)fc0 * 4u, fvoff, fc0 + khalf * C::KPT, a.Cs, HWs4, sA,
                       sB, wm, wn, l31, lh);
    }

    // ---- epilogue: a lane owns a column (pixel) of each accumulator; the phase's pixels are sw apart in a row of O ------------------
    const int HWd = a.Hd * a.Wd;
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
        const int64_t col = n0 + wn * 64 + nn * 32 + l31;
        if (col >= N) continue;
        const int cb_ = (int)(col / HWq);
        const int rem = (int)(col - (int64_t)cb_ * HWq);
        const int cy = rem / nxq, cx = rem - cy * nxq;
        float* dst = a.Dst + ((int64_t)cb_ * a.M) * HWd + (int64_t)(yf + cy * a.sh) * a.Wd + (xf + cx * a.sw);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (m < a.M) dst[(int64_t)m * HWd] = acc[i][nn][e] + (a.bias ? a.bias[m] : 0.f);
            }
    }
}

static int gcd_int(int x, int y) {
    while (y) { const int t = x % y; x = y; y = t; }
    return x;
}

// the grid's second dimension carries the phase
constexpr int64_t kMaxPhases = 65535;

static int launch_conv_phase(const float* X, const float* Wt, const float* bias, float* O, const ConvGeom& g, hipStream_t st) {
    const int M = g.Cin, Cs = g.Cout;                                    // mirrored geometry: rows = the layer's output channels
    const int wm = M > 64 ? 2 : 1;
    const int BM = 64 * wm, BN = 256 / wm, BK = wm == 2 ? 32 : 16;
    const int taps = g.kh * g.kw;
    const int Mp = (int)ceil_div(M, BM) * BM, Csp = (int)ceil_div(Cs, BK) * BK;
    const int64_t wr_floats = (int64_t)taps * Mp * Csp;
    const int64_t src_bytes = (int64_t)g.B * Cs * g.Ho * g.Wo * 4;
    // (+ one k-tile of channels: the scalar channel offset of a padded channel, added to the out-of-range marker, must not wrap)
    NNHIP_CHECK_ARG(src_bytes + (int64_t)BK * g.Ho * g.Wo * 4 < ((int64_t)1 << 31) && wr_floats * 4 < ((int64_t)1 << 31), NNHIP_EINVAL,
                    "conv_transpose2d: the implicit-GEMM kernel addresses each operand with 32-bit byte offsets (tensor >= 2 GiB)");
    const int tiles_m = Mp / BM;
    const int64_t nq_max = (int64_t)g.B * ceil_div(g.H, g.sh) * ceil_div(g.W, g.sw);   // columns of the largest phase
    const int64_t tiles_n = ceil_div(nq_max, BN);
    NNHIP_CHECK_ARG(tiles_n * tiles_m < ((int64_t)1 << 27), NNHIP_EINVAL, "conv_transpose2d: too many tiles");
    float* Wr = static_cast<float*>(workspace((size_t)wr_floats * sizeof(float)));
    NNHIP_CHECK_ARG(Wr != nullptr, NNHIP_ENOMEM, "conv_transpose2d: workspace allocation failed");
    if (int rc = conv_repack(Wt, Wr, g, Mp, Csp, true, true, st)) return rc;

    ConvPhaseArgs a;
    a.Wr = Wr; a.Src = X; a.bias = bias; a.Dst = O;
    a.B = g.B; a.M = M; a.Mp = Mp; a.Cs = Cs; a.Csp = Csp; a.Hs = g.Ho; a.Ws = g.Wo; a.Hd = g.H; a.Wd = g.W; a.kh = g.kh; a.kw = g.kw;
    a.sh = g.sh; a.sw = g.sw; a.dh = g.dh; a.dw = g.dw; a.pu = g.pu; a.pl = g.pl;
    a.rstep = g.sh / gcd_int(g.dh, g.sh);
    a.sstep = g.sw / gcd_int(g.dw, g.sw);
    a.tiles_m = tiles_m;
    const dim3 grid((unsigned)(tiles_n * tiles_m), (unsigned)(g.sh * g.sw));
    if (wm == 2) {
        auto kern = conv_phase_kernel<2>;
        static bool attr = false;
        if (!attr) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TapCfg<2>::LDS);
            if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(conv_phase_kernel)");
            attr = true;
        }
        hipLaunchKernelGGL(kern, grid, dim3(256), TapCfg<2>::LDS, st, a);
    } else {
        hipLaunchKernelGGL(conv_phase_kernel<1>, grid, dim3(256), TapCfg<1>::LDS, st, a);
    }
    NNHIP_LAUNCH_CHECK("conv_phase_kernel");
    return 0;
}

// =================================================================================================================================
// backward helpers
// =================================================================================================================================
// dW[o][i][tap] = G[i][o][taps - 1 - tap]: the mirrored Conv2d's weight gradient -> the layer's layout
__global__ __launch_bounds__(256) void convt_dw_permute_kernel(const float* __restrict__ G, float* __restrict__ dW, int Cout, int Cin, int taps) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)Cout * Cin * taps) return;
    const int tap = (int)(idx % taps);
    const int i = (int)((idx / taps) % Cin);
    const int o = (int)(idx / ((int64_t)taps * Cin));
    dW[idx] = G[((int64_t)i * Cout + o) * taps + (taps - 1 - tap)];
}

// db[o] = sum_{b, p} dO[b][o][p]: one block per channel, each thread a fixed stride of (b, p), the block sum in a fixed order
__global__ __launch_bounds__(256) void convt_db_kernel(const float* __restrict__ dO, float* __restrict__ db, int B, int Cout, int HW) {
    __shared__ float red[4];
    const int o = blockIdx.x;
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* row = dO + ((int64_t)b * Cout + o) * HW;
        for (int p = threadIdx.x; p < HW; p += 256) s += row[p];
    }
    s = block_sum<4>(s, red);
    if (threadIdx.x == 0) db[o] = s;
}

// =================================================================================================================================
// descriptor -> plan
// =================================================================================================================================
struct ConvTPlan {
    ConvGeom g;              // the mirrored Conv2d geometry (conv_common.h)
    nnhipConv2dDesc cd;      // the equivalent Conv2d (route conv2d only)
    int Ho, Wo;
    bool as_conv2d;          // stride 1, padding <= d (k-1)
    bool full_phases;        // every stride phase has at least one tap
};

static bool mul_below(std::initializer_list<int64_t> f, int64_t lim) {
    int64_t v = 1;
    for (int64_t x : f) {
        if (x <= 0) return x == 0;
        if (v > lim / x) return false;
        v *= x;
    }
    return v < lim;
}

static int make_plan(const nnhipConvTranspose2dDesc* d, ConvTPlan& p) {
    NNHIP_CHECK_ARG(d != nullptr, NNHIP_EINVAL, "conv_transpose2d: null descriptor");
    const int64_t dim_lim = (int64_t)1 << 31;
    NNHIP_CHECK_ARG(d->B >= 0 && d->Cin > 0 && d->H > 0 && d->W > 0 && d->Cout > 0 && d->kh > 0 && d->kw > 0 && d->sh > 0 && d->sw > 0 &&
                        d->dh > 0 && d->dw > 0 && d->pu >= 0 && d->pd >= 0 && d->pl >= 0 && d->pr >= 0 && d->oph >= 0 && d->opw >= 0,
                    NNHIP_EINVAL, "conv_transpose2d: bad descriptor");
    for (int64_t v : {d->B, d->Cin, d->H, d->W, d->Cout, d->kh, d->kw, d->sh, d->sw, d->dh, d->dw, d->pu, d->pd, d->pl, d->pr})
        NNHIP_CHECK_ARG(v < dim_lim / 4, NNHIP_EINVAL, "conv_transpose2d: dimension too large");
    NNHIP_CHECK_ARG(d->oph < (d->sh > d->dh ? d->sh : d->dh) && d->opw < (d->sw > d->dw ? d->sw : d->dw), NNHIP_EINVAL,
                    "conv_transpose2d: output_padding must be smaller than max(stride, dilation)");
    const int64_t Ho = (d->H - 1) * d->sh - (d->pu + d->pd) + d->dh * (d->kh - 1) + d->oph + 1;     // convtranspose2d.py:249-262
    const int64_t Wo = (d->W - 1) * d->sw - (d->pl + d->pr) + d->dw * (d->kw - 1) + d->opw + 1;
    NNHIP_CHECK_ARG(Ho > 0 && Wo > 0, NNHIP_EINVAL, "conv_transpose2d: empty output");
    NNHIP_CHECK_ARG(Ho < dim_lim / 4 && Wo < dim_lim / 4 && mul_below({d->B, d->Cin, d->H, d->W, 4}, dim_lim) &&
                        mul_below({d->B, d->Cout, Ho, Wo, 4}, dim_lim) && mul_below({d->Cout, d->Cin, d->kh, d->kw, 4}, dim_lim) &&
                        mul_below({d->dh, d->kh}, dim_lim / 4) && mul_below({d->dw, d->kw}, dim_lim / 4),
                    NNHIP_EINVAL, "conv_transpose2d: tensors of 2 GiB or more are not supported");
    ConvGeom& g = p.g;
    g.B = (int)d->B; g.Cin = (int)d->Cout; g.H = (int)Ho; g.W = (int)Wo; g.Cout = (int)d->Cin; g.Ho = (int)d->H; g.Wo = (int)d->W;
    g.kh = (int)d->kh; g.kw = (int)d->kw; g.sh = (int)d->sh; g.sw = (int)d->sw; g.dh = (int)d->dh; g.dw = (int)d->dw;
    g.pu = (int)d->pu; g.pl = (int)d->pl;
    p.Ho = (int)Ho; p.Wo = (int)Wo;
    const int64_t eh = d->dh * (d->kh - 1), ew = d->dw * (d->kw - 1);
    p.as_conv2d = d->sh == 1 && d->sw == 1 && d->pu <= eh && d->pl <= ew && eh - d->pd + d->oph >= 0 && ew - d->pr + d->opw >= 0;
    p.cd = nnhipConv2dDesc{d->B, d->Cin, d->H, d->W, d->Cout, d->kh, d->kw, 1, 1, d->dh, d->dw,
                           eh - d->pu, eh - d->pd + d->oph, ew - d->pl, ew - d->pr + d->opw};
    // r d runs through every residue of the stride iff gcd(d, s) = 1 and there are at least s taps
    p.full_phases = gcd_int(g.dh, g.sh) == 1 && gcd_int(g.dw, g.sw) == 1 && g.kh >= g.sh && g.kw >= g.sw;
    return 0;
}

static std::atomic<int> g_route{NNHIP_CONVT_ROUTE_AUTO};

// The route of a forward.  `auto` at stride > 1: the phase route where every phase has a tap -- it then issues 1 / (sh sw) of the
// gather route's MFMAs -- and the gather route otherwise (a phase without taps would spend blocks on writing bias).  Measured on an
// MI355X for the one shape class the DDPM U-Net has (kernel 4, stride 2, padding 1, batch 64; EXPERIMENTS 5.15,
// profiles/convt_kbench.txt, routes alternating in one process, spread of the round medians <= 8 %): phase / gather =
// 0.155 / 0.271 ms at 512 channels 4 -> 8, 0.090 / 0.267 at 256 8 -> 16, 0.087 / 0.256 at 128 16 -> 32, 0.039 / 0.053 at 64 8 -> 16,
// 0.027 / 0.063 at 32 16 -> 32: the phase route is 1.3x - 3.0x faster everywhere and stays.  Other classes (other kernels / strides,
// dilation, phases with unequal tap counts) are NOT measured and follow the same rule until they are.
static int resolve_route(const ConvTPlan& p, int requested) {
    if (p.as_conv2d) return NNHIP_CONVT_ROUTE_CONV2D;
    const int64_t phases = (int64_t)p.g.sh * p.g.sw;
    if (phases == 1 || phases > kMaxPhases) return NNHIP_CONVT_ROUTE_GATHER;
    if (requested == NNHIP_CONVT_ROUTE_PHASE || requested == NNHIP_CONVT_ROUTE_GATHER) return requested;
    return p.full_phases ? NNHIP_CONVT_ROUTE_PHASE : NNHIP_CONVT_ROUTE_GATHER;
}

}  // namespace nnhip

using namespace nnhip;

extern "C" int nnhipSetConvTransposeRoute(int route) {
    if (route < NNHIP_CONVT_ROUTE_AUTO || route > NNHIP_CONVT_ROUTE_GATHER) return g_route.load();
    return g_route.exchange(route);
}
extern "C" int nnhipGetConvTransposeRoute(void) { return g_route.load(); }

extern "C" int nnhipConvTranspose2dPlan(const nnhipConvTranspose2dDesc* d, int32_t* route, int32_t* phase_taps_out, int32_t* phase_pixels,
                                        int32_t capacity) {
    ConvTPlan p;
    if (make_plan(d, p)) return NNHIP_EINVAL;
    const ConvGeom& g = p.g;
    const int64_t phases = (int64_t)g.sh * g.sw;
    NNHIP_CHECK_ARG(route && phase_taps_out && phase_pixels, NNHIP_EINVAL, "nnhipConvTranspose2dPlan: null pointer");
    NNHIP_CHECK_ARG(capacity >= phases, NNHIP_EINVAL, "nnhipConvTranspose2dPlan: capacity %d is below the %lld stride phases", (int)capacity,
                    (long long)phases);
    *route = resolve_route(p, NNHIP_CONVT_ROUTE_AUTO);
    const int rstep = g.sh / gcd_int(g.dh, g.sh), sstep = g.sw / gcd_int(g.dw, g.sw);
    for (int py = 0; py < g.sh; ++py) {
        int yf, nyq, r0, nr;
        phase_axis(py, g.pu, g.sh, g.H, yf, nyq);
        phase_taps(py, g.dh, g.sh, rstep, g.kh, r0, nr);
        for (int px = 0; px < g.sw; ++px) {
            int xf, nxq, s0, ns;
            phase_axis(px, g.pl, g.sw, g.W, xf, nxq);
            phase_taps(px, g.dw, g.sw, sstep, g.kw, s0, ns);
            phase_taps_out[py * g.sw + px] = nr * ns;
            phase_pixels[py * g.sw + px] = nyq * nxq;
        }
    }
    return (int)phases;
}

extern "C" int nnhipConvTranspose2dForward(const float* X, const float* W, const float* bias, float* O, const nnhipConvTranspose2dDesc* d,
                                           nnhipStream_t s) {
    ConvTPlan p;
    if (int rc = make_plan(d, p)) return rc;
    if (p.g.B == 0) return 0;
    NNHIP_CHECK_ARG(X && W && O, NNHIP_EINVAL, "nnhipConvTranspose2dForward: null pointer");
    switch (resolve_route(p, g_route.load())) {
        case NNHIP_CONVT_ROUTE_CONV2D: return nnhipConv2dForward(X, W, bias, O, &p.cd, s);
        case NNHIP_CONVT_ROUTE_PHASE: return launch_conv_phase(X, W, bias, O, p.g, (hipStream_t)s);
        default: return conv_mfma_tconv_gather(X, W, bias, O, p.g, (hipStream_t)s);
    }
}

extern "C" int nnhipConvTranspose2dBackward(const float* X, const float* W, const float* dO, float* dX, float* dW, float* db,
                                            const nnhipConvTranspose2dDesc* d, nnhipStream_t s) {
    ConvTPlan p;
    if (int rc = make_plan(d, p)) return rc;
    if (p.g.B == 0) return 0;
    NNHIP_CHECK_ARG(X && W && dO, NNHIP_EINVAL, "nnhipConvTranspose2dBackward: null pointer");
    if (p.as_conv2d) return nnhipConv2dBackward(X, W, dO, dX, dW, db, &p.cd, s);
    hipStream_t st = (hipStream_t)s;
    const ConvGeom& g = p.g;
    if (dX) {
        if (int rc = conv_mfma_tconv_dgrad(dO, W, dX, g, st)) return rc;
    }
    if (dW) {
        // the mirrored weight gradient [in][out][taps] lands in the library's second scratch block (the wgrad kernels' slabs take
        // the general workspace while it is live), then moves to the layer's [out][in][taps] with the taps reversed
        const int64_t nw = (int64_t)g.Cin * g.Cout * g.kh * g.kw;
        float* G = static_cast<float*>(workspace_arena(2, (size_t)nw * sizeof(float)));
        NNHIP_CHECK_ARG(G != nullptr, NNHIP_ENOMEM, "nnhipConvTranspose2dBackward: workspace allocation failed");
        if (int rc = conv_mfma_wgrad(dO, X, G, nullptr, g, st)) return rc;
        hipLaunchKernelGGL(convt_dw_permute_kernel, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0, st, G, dW, g.Cin, g.Cout, g.kh * g.kw);
        NNHIP_LAUNCH_CHECK("convt_dw_permute_kernel");
    }
    if (db) {
        hipLaunchKernelGGL(convt_db_kernel, dim3((unsigned)g.Cin), dim3(256), 0, st, dO, db, g.B, g.Cin, g.H * g.W);
        NNHIP_LAUNCH_CHECK("convt_db_kernel");
    }
    return 0;
}
