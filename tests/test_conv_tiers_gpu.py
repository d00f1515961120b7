"""GPU: every kernel, route and developer switch of csrc/conv2d.hip + csrc/conv_mfma.hip on behalf of Conv2d, through the C ABI
(include/neunet_hip.h) into NaN-filled, NaN-fenced buffers, against the float64 restatements of tests/conv_ref.py.  The dispatch is
restated there as route(); tests/test_conv_ref.py checks (on the CPU) that the case table reaches every instantiation.  The conv section
of tests/test_hip_parity.py keeps the reference's fixtures, the layer API and the full-size samples.

Dispatch (kernel: condition -> cases of conv_ref.CASES; "child X": reached only under the switch setting X of conv_ref.SETTINGS):

    conv_direct_fwd_quad_kernel<8|16>     Cin, Cout <= 16, taps <= 25; 3x3, B Ho Wo <= 131072, Cin >= 4, Cout > 4      nt_c{5,6,8,9,16}_o{7,16}, quad_c4_o5,
                                                                                                                        quad_c9_o5, quad_s2, quad_d2, asym_quad
    conv_direct_fwd_kernel<4|8|16>        direct otherwise: 3x3 buffer path / generic loop                              nt_c*_o1, nt_c{1,3}_o*, quad_c3_o5, quad_c4_o4,
                                          (above 131072 positions with Cin >= 4: big_fwd_c11 = groups of 8 + 3)         taps25_c3 (generic), asym_direct, big_*; child nosplit
    conv_direct_dgrad_quad2_kernel<4|8>   3x3, B H W <= 131072, Cout >= 4, 2 < Cin <= 8, unit stride and dilation       nt_c{3,5,6,8}_o{7,16}, quad_c{3,4}_o*, asym_quad
    conv_direct_dgrad_quad_kernel<4|8>    the same at stride or dilation != 1                                           quad_s2, quad_d2; child quad1
    conv_direct_dgrad_kernel<4|8|16>      direct otherwise                                                              nt_c1_*, nt_c*_o1, nt_c{9,16}_*, big_dgrad_c5 (<8>, 3x3
                                                                                                                        above 131072), big_fwd_c11 (<16>); child nosplit
    conv_tap_kernel<fwd|dgrad, 1|2>       not direct; wm = 2 when M > 64 (fwd M = Cout, dgrad M = Cin)                  wg_*, c200_*, lim_c17_o16, lim_c16_o17, taps49_c3,
      + conv_repack_kernel                                                                                              taps26_c2, asym_igemm*; child igemm (every small case)
      + conv_tap_reduce_kernel            tail > 0 and splits > 1 (whole rounds + split tail: tile64_main_tail)         most of the above; none under child nosplit
    conv_mfma_wgrad_kernel<NT,false>      direct, 3x3, wg_lds <= 60 KiB, nt <= 10, m_lds <= 60 KiB; NT = 1,2,3,5,10     nt_c{1|2,3|5|6,8|9,16}_*, dwg_c16_o4, dwg_c1_86
    conv_direct_wgrad_kernel<CO,CIP>      direct, 3x3, wg_lds <= 60 KiB < m_lds                                         dwg_c16, dwg_c16_o6 (<8,16>), dwg_c1 (<8,1>);
                                                                                                                        all ten under child nosplit
    conv_wgrad_mfma_kernel<WM,CB,A,F>     otherwise; WM = 2 when Cout > 64; CB = 32..256 >= Cin; A: Ho Wo % 4 == 0 and  wg_c{17,33,65,129}_o{24,65}_{2x2,3x3,8x8,7x9}, c200_*,
      + conv_wgrad_mfma_reduce_kernel     dO 16-byte aligned; F (flat k): per-image tiles waste > 1/33                  dwg_c16_o7, dwg_c1_88, igemm_c16_32, taps*, big_*
    conv_wgrad_reduce_kernel              after either small-channel wgrad kernel                                       (with them)
    conv_wgrad_reduce_group_kernel        >= 2 queued reduces at a flush                                                test_deferred_reduce_queue
    conv_pool_fwd_kernel<8|16>            fused forward, Cin <= 4, >= 32768 windows                                     pf_window8, pf_window16
    conv_pool_fwd_quad_kernel<8|16,S>     fused forward where the plain forward takes the quad kernel; S: statistics    pf_quad*, ps_quad*
    conv_mfma_wgrad_kernel<NT,true>       nnhipConv2dWeightGradPooled                                                   pw_*

Bounds, none tuned.  O and dX: |got - float64| <= 32 x 2^-24 x sum |a||b| + 4 x 2^-24 |ref| + 1e-30 per element (dot_bound of
test_hip_parity.py, c = 32, the rule test_conv2d_mfma_full_size_samples applies to 124 sampled entries).  dW and db: 1e-4 of
max(|ref|, rms(ref)) (assert_close_scaled: the project's rule for sums over batch x pixels).  Separately requested outputs, deferred
reduces, the pooled weight gradient against nnhipConv2dBackward, and every route a switch does not touch: bit-identical.

Worst error / bound per route (every test prints its own with -s).  "float32 on the CPU": the oracle's float32 einsums against the same
float64 reference and bound on the small cases; "kernels": the first MI355X run (EXPERIMENTS.md 5.24).  No ratio above 0.16.

    route                                      tensor    float32 on the CPU    kernels
    conv_direct_fwd_kernel                     O         0.097                 0.154  (big_dgrad_c5; small cases 0.10)
    conv_direct_fwd_quad_kernel                O         0.060                 0.056
    conv_tap_kernel<fwd> / <dgrad>             O / dX    0.051 / 0.054         0.160 / 0.152  (tile64_main_tail; small cases 0.08)
    conv_direct_dgrad_kernel                   dX        0.087                 0.141  (big_fwd_c11)
    conv_direct_dgrad_quad2 / quad_kernel      dX        0.040 / 0.044         0.039 / 0.036
    conv_mfma_wgrad_kernel<NT,false>           dW / db   0.029 / 0.010         0.023 / 0.013
    conv_direct_wgrad_kernel                   dW / db   0.038 / 0.002         0.004 / 0.002
    conv_wgrad_mfma_kernel                     dW / db   0.030 / 0.004         0.018 / 0.005
    children nosplit / igemm / quad1           any       --                    0.155 / 0.079 / 0.122
    one-float-offset pointers (scalar paths)   any       --                    0.062
    fused forward: P at the returned index     P         --                    0.117  (near-ties: at most 1.0e-5 of the windows)
    fused forward statistics                   mean, M2  --                    0.142
    pooled weight gradient                     dW / db   --                    0.002"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conv_child import (FencedAt, TENSORS, backward, call, cdesc, cpool, dev_at, digest, forward, references, run_case, scaled_bound, worst)
from conv_ref import (BY_NAME, CASES, ENV, POOL_FWD_CASES, POOL_STATS_CASES, POOL_WGRAD_CASES, SETTINGS, U24, child_cases, conv2d_forward64, conv_leaky_pool64, dgrad_abs_sum,
                      leaky64, make_inputs, near_ties, pooled_wgrad64, route, setting_env, stats_blocks, switches, window_view)
from lstm_abi import dev
from test_hip_parity import assert_close_scaled, assert_within
from vision_ref import PoolDesc, sum_bound

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
TIE_CAP = 0.005
ALPHAS = (0.01, 1.0)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    assert not [v for v in ENV.values() if v in os.environ], "this module needs the default dispatch in the parent process"
    return neunet_hip


def pool_of(d, kh=2, kw=2):
    Ho, Wo = d.out_hw()
    return PoolDesc(d.B, d.Cout, Ho, Wo, kh, kw)


# ===================================================================================================== a. every table case
_default = {}


def default_run(name):
    """The default-switch in-process run of a case, once per module run (the switch tests compare digests with it)."""
    if name not in _default:
        _default[name] = run_case(BY_NAME[name], keep=not BY_NAME[name].big)
    return _default[name]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_default_switches(hip, case):
    r = default_run(case.name)
    rt = route(case.desc)
    print(f"\n[conv {case.name}] " + " | ".join(rt[p]["kernel"] for p in ("fwd", "dgrad", "wgrad")) + " -- error / bound: " +
          ", ".join(f"{k} {v:.3f}" for k, v in r["ratios"].items()))
    assert not r["problems"], r["problems"]
    for k in TENSORS:
        assert r["ratios"][k] <= 1.0, (k, r["ratios"][k])


# ===================================================================================================== b. ABI edges
def test_batch_zero_touches_nothing(hip):
    d = BY_NAME["nt_c5_o7"].desc
    X, Wt, b, dO = make_inputs("nt_c5_o7", d)
    x, w, bd, g = dev(X), dev(Wt), dev(b), dev(dO)
    d0 = d.replace(B=0)
    o = FencedAt((d.B, d.Cout) + d.out_hw())
    assert call("nnhipConv2dForward", x, w, bd, o.view, cdesc(d0)) == 0
    f = [FencedAt((d.B, d.Cin, d.H, d.W)), FencedAt((d.Cout, d.Cin, 3, 3)), FencedAt((d.Cout,))]
    assert call("nnhipConv2dBackward", x, w, g, f[0].view, f[1].view, f[2].view, cdesc(d0)) == 0
    torch.cuda.synchronize()
    assert o.untouched() and all(t.untouched() for t in f)


MISALIGNED = ["nt_c1_o7",            # direct fwd <8>, direct dgrad <4>, conv_mfma_wgrad_kernel<1>
              "nt_c8_o16",           # quad fwd <16>, quad2 dgrad <8>, conv_mfma_wgrad_kernel<5>
              "wg_c17_o24_8x8"]      # conv_tap_kernel fwd / dgrad with cvec (64 pixels), conv_wgrad_mfma_kernel with avec


@pytest.mark.parametrize("which", ["X", "W", "dO", "out"])
@pytest.mark.parametrize("name", MISALIGNED)
def test_one_float_offset_pointers(hip, name, which):
    """One pointer at a time 4-byte but not 16-byte aligned.  The direct, quad and small-channel wgrad kernels never look at the
    alignment: bit-identical.  conv_tap_kernel drops cvec when its output is misaligned and conv_wgrad_mfma_kernel drops avec when dO
    is: the scalar variants hold the bounds; everything route() says is unchanged stays bit-identical."""
    case = BY_NAME[name]
    d = case.desc
    base = default_run(name)
    ref = references(case)
    X, Wt, b, dO = make_inputs(name, d)
    x, w, bd, g = dev_at(X, which == "X"), dev_at(Wt, which == "W"), dev(b), dev_at(dO, which == "dO")
    off = int(which == "out")
    o = forward(d, x, w, bd, off)
    outs, _ = backward(d, x, w, g, off=off)
    torch.cuda.synchronize()
    got = dict(O=o, **outs)
    r_al, r_off = route(d), route(d, aligned=False)
    same = dict(O=which != "out" or r_al["fwd"] == r_off["fwd"], dX=which != "out" or r_al["dgrad"] == r_off["dgrad"],
                dW=which != "dO" or r_al["wgrad"] == r_off["wgrad"], db=which != "dO" or r_al["wgrad"] == r_off["wgrad"])
    ratios = {}
    for k, f in got.items():
        assert f.guards_intact(), f"{k}: wrote outside the buffer"
        ratios[k] = worst(f.host(), *ref[k])
        assert ratios[k] <= 1.0, (k, ratios[k])
        if same[k]:
            assert digest(f.view) == base["digests"][k], f"{k}: not bit-identical to the aligned call"
    print(f"\n[conv {name} {which}+4B] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) +
          "; scalar variant: " + (", ".join(k for k, v in same.items() if not v) or "none"))


def test_refusals(hip):
    """EINVAL decided on the host before any launch (conv2d.hip: make_geom's three NNHIP_CHECK_ARG -- null descriptor, bad descriptor,
    empty output; the `null pointer` checks at the top of nnhipConv2dForward / Backward / WeightGradPooled / conv_pool_forward; the
    `unsupported geometry` checks behind pooled_wgrad_ok / conv_pool_fwd_ok; nnhipConv2dLeakyMaxPoolForwardStats' StatsBlocks check).
    Every call gets valid buffers of the full size, so a refusal that went missing would still write only memory it owns."""
    from neunet_hip._lib import NeunetHipError
    d = BY_NAME["nt_c5_o7"].desc
    X, Wt, b, dO = make_inputs("nt_c5_o7", d)
    x, w, bd, g = dev(X), dev(Wt), dev(b), dev(dO)
    o = FencedAt((d.B, d.Cout) + d.out_hw())
    fx, fw, fb = FencedAt((d.B, d.Cin, d.H, d.W)), FencedAt((d.Cout, d.Cin, 3, 3)), FencedAt((d.Cout,))

    def refused(message, name, *args):
        """The call answers NNHIP_EINVAL (-1) with the text of the NNHIP_CHECK_ARG named."""
        with pytest.raises(NeunetHipError, match=re.escape(f"{name} failed with status -1: ") + ".*" + re.escape(message)):
            call(name, *args)
    # make_geom(): "conv2d: null descriptor", "conv2d: bad descriptor" (a zero or negative field), "conv2d: empty output" (Ho = 0)
    bad = [(None, "conv2d: null descriptor")] + \
          [(d.replace(**kw), "conv2d: bad descriptor") for kw in (dict(Cin=0), dict(sh=0), dict(dw=0), dict(pu=-1), dict(B=-1), dict(kw=-3))] + \
          [(d.replace(H=1, pu=0, pd=0), "conv2d: empty output")]
    for dd, msg in bad:
        cd = None if dd is None else cdesc(dd)
        refused(msg, "nnhipConv2dForward", x, w, bd, o.view, cd)
        refused(msg, "nnhipConv2dBackward", x, w, g, fx.view, fw.view, fb.view, cd)
    # the first NNHIP_CHECK_ARG after make_geom() and the B == 0 return of each entry
    for args in ((None, w, bd, o.view), (x, None, bd, o.view), (x, w, bd, None)):
        refused("nnhipConv2dForward: null pointer", "nnhipConv2dForward", *args, cdesc(d))
    for args in ((None, w, g), (x, None, g), (x, w, None)):
        refused("nnhipConv2dBackward: null pointer", "nnhipConv2dBackward", *args, fx.view, fw.view, fb.view, cdesc(d))
    # the fused entries on geometries their ...Ok queries reject: a 7 x 9 output is not tiled by 2 x 2 windows
    p = pool_of(d)
    assert call("nnhipConv2dWeightGradPooledOk", cdesc(d), cpool(p)) == 0 and call("nnhipConv2dLeakyMaxPoolForwardOk", cdesc(d), cpool(p)) == 0
    P = FencedAt((d.B, d.Cout, 3, 4))
    arg = torch.full((d.B, d.Cout, 3, 4), -7, dtype=torch.int32, device="cuda")
    dP, arg0 = P.view.nan_to_num(), arg.clamp(min=0)
    refused("nnhipConv2dWeightGradPooled: unsupported geometry", "nnhipConv2dWeightGradPooled", x, dP, arg0, None, 1.0, fw.view, fb.view,
            cdesc(d), cpool(p))
    refused("nnhipConv2dWeightGradPooled: null pointer", "nnhipConv2dWeightGradPooled", x, dP, arg0, None, 1.0, None, None, cdesc(d), cpool(p))
    refused("nnhipConv2dLeakyMaxPoolForward: unsupported geometry", "nnhipConv2dLeakyMaxPoolForward", x, w, bd, 0.01, P.view, arg, cdesc(d), cpool(p))
    refused("nnhipConv2dLeakyMaxPoolForward: null pointer", "nnhipConv2dLeakyMaxPoolForward", x, w, bd, 0.01, None, arg, cdesc(d), cpool(p))
    # a geometry the fused forward takes, alpha <= 0; and the statistics variant where StatsBlocks is 0 (105 windows)
    name, dq, _ = POOL_FWD_CASES[3]
    Xq, Wq, bq, _ = make_inputs(name, dq)
    pq = pool_of(dq)
    assert call("nnhipConv2dLeakyMaxPoolForwardOk", cdesc(dq), cpool(pq)) == 1 and call("nnhipConv2dLeakyMaxPoolStatsBlocks", cdesc(dq), cpool(pq)) == 0
    Pq = FencedAt((dq.B, dq.Cout, 5, 7))
    argq = torch.full((dq.B, dq.Cout, 5, 7), -7, dtype=torch.int32, device="cuda")
    st = FencedAt((4, dq.Cout, 2))
    refused("alpha must be > 0", "nnhipConv2dLeakyMaxPoolForward", dev(Xq), dev(Wq), dev(bq), 0.0, Pq.view, argq, cdesc(dq), cpool(pq))
    refused("no statistics variant for this geometry", "nnhipConv2dLeakyMaxPoolForwardStats", dev(Xq), dev(Wq), dev(bq), 0.01, Pq.view, argq,
            cdesc(dq), cpool(pq), st.view)
    torch.cuda.synchronize()
    assert all(t.untouched() for t in (o, fx, fw, fb, P, Pq, st)) and bool((arg == -7).all()) and bool((argq == -7).all())


# ===================================================================================================== c. the fused entries
def int_fenced(shape, fill=-7):
    n = int(np.prod(shape))
    whole = torch.full((n + 128,), fill, dtype=torch.int32, device="cuda")
    return whole, whole[64:64 + n].view(*shape)


def fused_forward(name, d, alpha, stats=False):
    X, Wt, b, _ = make_inputs(name, d)
    Ho, Wo = d.out_hw()
    p = pool_of(d)
    P = FencedAt((d.B, d.Cout, Ho // 2, Wo // 2))
    whole, arg = int_fenced((d.B, d.Cout, Ho // 2, Wo // 2))
    st = None
    if stats:
        nb = call("nnhipConv2dLeakyMaxPoolStatsBlocks", cdesc(d), cpool(p))
        assert nb == stats_blocks(d, p, switches()) > 0
        st = FencedAt((nb, d.Cout, 2))
        call("nnhipConv2dLeakyMaxPoolForwardStats", dev(X), dev(Wt), dev(b), alpha, P.view, arg, cdesc(d), cpool(p), st.view)
    else:
        assert call("nnhipConv2dLeakyMaxPoolForwardOk", cdesc(d), cpool(p)) == 1
        call("nnhipConv2dLeakyMaxPoolForward", dev(X), dev(Wt), dev(b), alpha, P.view, arg, cdesc(d), cpool(p))
    torch.cuda.synchronize()
    assert P.guards_intact() and bool((whole[:64] == -7).all()) and bool((whole[-64:] == -7).all()), "wrote outside P / argmax"
    assert st is None or st.guards_intact()
    got_P, got_arg = P.host(), arg.cpu().numpy()
    assert not np.isnan(got_P).any() and got_arg.min() >= 0 and got_arg.max() <= 3
    # ---- against float64
    Pr, ar, V, Vb = conv_leaky_pool64(X, Wt, b, alpha, d)
    tie = near_ties(V, Vb)
    share = float(tie.mean())
    assert share <= TIE_CAP, share
    assert np.array_equal(got_arg[~tie], ar[~tie]), f"{name}: arg-max differs at {int((got_arg != ar)[~tie].sum())} windows that are no near-tie"
    wv, wb = window_view(V), window_view(Vb)
    at = np.take_along_axis(wv, got_arg[..., None].astype(np.int64), -1)[..., 0]        # the float64 value at the RETURNED index
    at_b = np.take_along_axis(wb, got_arg[..., None].astype(np.int64), -1)[..., 0]
    r_at = worst(got_P, at, at_b)
    r_max = worst(got_P[~tie], Pr[~tie], wb.max(axis=-1)[~tie])
    print(f"\n[conv+pool {name} alpha {alpha}] near-ties {share:.2e} of {tie.size} windows; P error / bound: at the returned index {r_at:.3f}, "
          f"against the float64 maximum {r_max:.3f}")
    assert r_at <= 1.0 and r_max <= 1.0
    return got_P, st


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name,d,why", POOL_FWD_CASES, ids=[c[0] for c in POOL_FWD_CASES])
def test_fused_forward(hip, name, d, why, alpha):
    fused_forward(name, d, alpha)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name,d,why", POOL_STATS_CASES, ids=[c[0] for c in POOL_STATS_CASES])
def test_fused_forward_stats(hip, name, d, why, alpha):
    """Per block of 64 windows (n = b Hq Wq + window, 64 consecutive n) and channel: (mean, M2) against float64 statistics of the kernel's
    OWN P.  Sum bounds (vision_ref.sum_bound): each of the 64 values passes through one element per lane, a tree of 6 additions (four
    xor steps, then (a + b) + (c + d) over the waves) and at most 4 roundings of its own (subtraction, square, the 1 / 64): c = 11.
    M2 is taken from the ROUNDED mean: + 64 dmean^2, + 2 x 2^-24 M2 (bn_stat_bounds' structure)."""
    got_P, st = fused_forward(name, d, alpha, stats=True)
    B, C, Hq, Wq = got_P.shape
    blocks = got_P.astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, 64, C)
    mean = blocks.mean(axis=1)
    dev2 = (blocks - mean[:, None, :]) ** 2
    M2 = dev2.sum(axis=1)
    dmean = sum_bound(blocks, 11, axis=1) / 64 + U24 * np.abs(mean)
    dM2 = sum_bound(dev2, 11, axis=1) + 64 * dmean ** 2 + 2 * U24 * M2
    got = st.host()
    print(f"[conv+pool stats {name}] error / bound: mean {worst(got[..., 0], mean, dmean):.3f}, M2 {worst(got[..., 1], M2, dM2):.3f}")
    assert_within(got[..., 0], mean, dmean, "block mean")
    assert_within(got[..., 1], M2, dM2, "block M2")
    # the statistics variant returns the same P and arg-max bits as the plain one
    plain, _ = fused_forward(name, d, alpha)
    assert np.array_equal(plain.view(np.int32), got_P.view(np.int32))


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name,d,pool,why", POOL_WGRAD_CASES, ids=[c[0] for c in POOL_WGRAD_CASES])
def test_pooled_weight_gradient(hip, name, d, pool, why, alpha):
    """nnhipConv2dWeightGradPooled.  The arg-max and the pooled output are those of the float64 chain (so the kernel's inputs are exact
    and no tie can matter), with pooled values of exactly +0.0 and -0.0 planted: the kernel's rule is  P <= 0 -> dP * alpha  (both zeros
    take alpha, as LeakyReLU's backward does on its output).  dW, db: against the float64 chain, and bit-identical to
    nnhipConv2dBackward(dX = NULL) fed the dO the chain implies.  Also pooled = NULL (no activation: dP passes unchanged)."""
    kh, kw = pool
    rng = np.random.default_rng(len(name) + kh * 10 + kw)
    X, Wt, b, _ = make_inputs(name, d)
    V = leaky64(conv2d_forward64(X, Wt, b, d), alpha)
    win = window_view(V, kh, kw)
    arg = np.argmax(win, axis=-1).astype(np.int32)
    pooled = np.max(win, axis=-1).astype(np.float32)
    flat = pooled.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    dP = rng.uniform(-1, 1, pooled.shape).astype(np.float32)
    p = pool_of(d, kh, kw)
    assert call("nnhipConv2dWeightGradPooledOk", cdesc(d), cpool(p)) == 1
    x, w0 = dev(X), dev(Wt)
    for with_pooled in (True, False):
        pl = pooled if with_pooled else None
        dWr, dbr, dO32 = pooled_wgrad64(X, dP, arg, pl, alpha, pool, d)
        fw, fb = FencedAt((d.Cout, d.Cin, 3, 3)), FencedAt((d.Cout,))
        call("nnhipConv2dWeightGradPooled", x, dev(dP), torch.from_numpy(arg).cuda(), None if pl is None else dev(pl), alpha, fw.view, fb.view,
             cdesc(d), cpool(p))
        plain, _ = backward(d, x, w0, dev(dO32), want=("dW", "db"))
        torch.cuda.synchronize()
        assert fw.guards_intact() and fb.guards_intact()
        print(f"\n[pooled wgrad {name} alpha {alpha} pooled {with_pooled}] error / bound: dW {worst(fw.host(), dWr, scaled_bound(dWr)):.3f}, "
              f"db {worst(fb.host(), dbr, scaled_bound(dbr)):.3f}")
        assert_close_scaled(fw.host(), dWr, err_msg="dW")
        assert_close_scaled(fb.host(), dbr, err_msg="db")
        assert torch.equal(fw.view, plain["dW"].view) and torch.equal(fb.view, plain["db"].view), "not the bits of nnhipConv2dBackward on the implied dO"
        # dW alone and db alone
        only_w, only_b = FencedAt((d.Cout, d.Cin, 3, 3)), FencedAt((d.Cout,))
        args = (x, dev(dP), torch.from_numpy(arg).cuda(), None if pl is None else dev(pl), alpha)
        call("nnhipConv2dWeightGradPooled", *args, only_w.view, None, cdesc(d), cpool(p))
        call("nnhipConv2dWeightGradPooled", *args, None, only_b.view, cdesc(d), cpool(p))
        assert torch.equal(only_w.view, fw.view) and torch.equal(only_b.view, fb.view)


# ===================================================================================================== d. the deferred reduce queue
def test_deferred_reduce_queue(hip):
    """nnhipWeightGradDefer on: 1 queued small-channel wgrad (conv_wgrad_reduce_kernel), 2 and 4 (conv_wgrad_reduce_group_kernel, a full
    queue), 5 (the fifth flushes the four before it), a job larger than the arena (it grows), and jobs on a second stream.  A stream
    change flushes what the first stream queued, and the arena is reused from offset 0: the new stream must not overwrite partials the
    flushed reduce has yet to read.  The queue's guard orders the new stream behind that reduce (it did not: the kernels of
    one nnhipConv2dBackward call went to two unordered streams); the steps here run without any synchronisation in between, so a
    missing order shows as a wrong or NaN gradient whenever the timing allows.  Every dW / db is bit-identical to the same call with
    deferral off ("same arithmetic, same order per output")."""
    names = ["nt_c1_o7", "nt_c5_o16", "nt_c16_o7", "dwg_c16", "nt_c3_o1", "lim_c16_o16"]
    big = BY_NAME["lim_c16_o16"].desc.replace(B=300)                        # 300 x 16 x 145 partials: larger than anything queued before it
    jobs = [(n, BY_NAME[n].desc) for n in names] + [("grow", big)]
    assert all(route(d)["wgrad"]["aux"] == ["conv_wgrad_reduce_kernel"] for _, d in jobs)
    ins, base = {}, {}
    for n, d in jobs:
        X, Wt, _, dO = make_inputs(n, d)
        ins[n] = (dev(X), dev(Wt), dev(dO))
        out, _ = backward(d, *ins[n], want=("dW", "db"))
        base[n] = (out["dW"].view.clone(), out["db"].view.clone())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def fences(d):
        return dict(dW=FencedAt((d.Cout, d.Cin, 3, 3)), db=FencedAt((d.Cout,)))

    def queue(n, d, stream=None, f=None):
        f = f or fences(d)
        call("nnhipConv2dBackward", *ins[n], None, f["dW"].view, f["db"].view, cdesc(d), stream=stream)
        return n, f

    def ready(*idx):
        """Output buffers filled with NaN BEFORE anything is queued (the fill runs on torch's current stream, which a job on `side`
        would not wait for), so that the calls below follow each other with no synchronisation in between."""
        fs = [fences(jobs[i][1]) for i in idx]
        torch.cuda.synchronize()
        return fs

    def check(queued):
        torch.cuda.synchronize()
        for n, f in queued:
            assert f["dW"].guards_intact() and f["db"].guards_intact()
            assert torch.equal(f["dW"].view, base[n][0]) and torch.equal(f["db"].view, base[n][1]), f"{n}: deferred reduce differs"
    call("nnhipWeightGradDefer", 1)
    try:
        for count in (1, 2, 4, 5):
            queued = [queue(*jobs[i]) for i in range(count)]
            call("nnhipWeightGradFlush")
            check(queued)
        queued = [queue(*jobs[0]), queue(*jobs[6]), queue(*jobs[1])]         # the second needs a larger arena: flush, grow, go on
        call("nnhipWeightGradFlush")
        check(queued)
        # a stream change: the two reduces queued on the default stream are flushed there and the new job's partials go to offset 0 of the same
        # arena from `side`.  No synchronisation here: the queue's guard orders `side` behind the flushed reduce itself (until it did, the
        # kernel on `side` could overwrite partials the reduce on the default stream had yet to read)
        fs = ready(2, 3, 4)
        queued = [queue(*jobs[2], f=fs[0]), queue(*jobs[3], f=fs[1]), queue(*jobs[4], stream=side.cuda_stream, f=fs[2])]
        call("nnhipWeightGradFlush", stream=side.cuda_stream)
        check(queued)
        # the same hazard without a queued job: flushed on one stream, the arena reused from the other at once, both ways round
        # A few milliseconds of matrix products go to the first stream between its jobs and its flush, so its reduce is still waiting
        # when the second stream's job is issued: without the order that job's kernel overwrites the partials at offset 0 before
        # the reduce has read them, every time.
        a = torch.ones(4096, 4096, device="cuda")
        for first, second in ((None, side.cuda_stream), (side.cuda_stream, None)) * 2:
            fs = ready(6, 1, 0, 5)
            queued = [queue(*jobs[6], stream=first, f=fs[0]), queue(*jobs[1], stream=first, f=fs[1])]
            with torch.cuda.stream(side if first else torch.cuda.default_stream()):
                keep = [a @ a for _ in range(4)]
            call("nnhipWeightGradFlush", stream=first)
            queued += [queue(*jobs[0], stream=second, f=fs[2]), queue(*jobs[5], stream=second, f=fs[3])]
            call("nnhipWeightGradFlush", stream=second)
            check(queued)
            del keep
    finally:
        call("nnhipWeightGradDefer", 0)


def test_deferred_reduce_queue_after_its_stream_is_destroyed(hip):
    """A reduce queued and flushed on a stream that is then synchronised and DESTROYED, the next one on the default stream: the arena's
    guard only compares the old handle.  (It used to record an event on it and ask whether it was capturing: undefined behaviour.)"""
    import ctypes
    import gc
    n, d = "nt_c1_o7", BY_NAME["nt_c1_o7"].desc
    X, Wt, _, dO = make_inputs(n, d)
    ins = (dev(X), dev(Wt), dev(dO))
    base, _ = backward(d, *ins, want=("dW", "db"))
    fs = [dict(dW=FencedAt((d.Cout, d.Cin, 3, 3)), db=FencedAt((d.Cout,))) for _ in range(2)]
    hiprt = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p()
    assert hiprt.hipStreamCreate(ctypes.byref(raw)) == 0
    st = torch.cuda.ExternalStream(raw.value)
    torch.cuda.synchronize()
    call("nnhipWeightGradDefer", 1)
    try:
        assert call("nnhipConv2dBackward", *ins, None, fs[0]["dW"].view, fs[0]["db"].view, cdesc(d), stream=raw.value) == 0
        assert call("nnhipWeightGradFlush", stream=raw.value) == 0
        st.synchronize()
        del st
        gc.collect()
        assert hiprt.hipStreamDestroy(raw) == 0
        assert call("nnhipConv2dBackward", *ins, None, fs[1]["dW"].view, fs[1]["db"].view, cdesc(d)) == 0
        assert call("nnhipWeightGradFlush") == 0
    finally:
        call("nnhipWeightGradDefer", 0)
    torch.cuda.synchronize()
    for f, where in zip(fs, ("on the stream destroyed since", "on the default stream behind it")):
        assert f["dW"].guards_intact() and f["db"].guards_intact()
        assert torch.equal(f["dW"].view, base["dW"].view) and torch.equal(f["db"].view, base["db"].view), f"{where}: deferred reduce differs"
        torch.cuda.synchronize()


# ===================================================================================================== the developer switches
_children, _dead = {}, []
MIN_MOVED = dict(nosplit=60, igemm=150, quad1=10)      # outputs route() sends elsewhere under the setting (test_conv_ref.py counts the cases)
CHILD_TIMEOUT = 240      # start-up (torch + library: ~15 s) + the child's float64 restatement (~5 s of CPU) + ~60 cases x 9 calls, x 8 for a slow machine


def child(setting):
    """tests/conv_child.py in a fresh interpreter under `setting`, once per module run; children never overlap.  A child that ends by
    timeout, by a signal or with status 134 / 139 stops every later child test at once: nothing more is started."""
    if _dead:
        pytest.fail(f"an earlier child process ended abnormally ({_dead[0]}); no further child is started")
    if setting not in _children:
        env = {k: v for k, v in os.environ.items() if not k.startswith("NNHIP_CONV_")}
        env.update(setting_env(setting))
        dump = os.path.join(tempfile.mkdtemp(prefix="conv_child_"), setting + ".npz")
        try:
            r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_child.py"), dump], env=env,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _dead.append(f"{setting}: timeout")
            pytest.fail(_dead[0])
        if r.returncode < 0 or r.returncode in (134, 139):
            _dead.append(f"{setting}: status {r.returncode}")
            pytest.fail(_dead[0] + "\n" + r.stderr[-4000:])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _children[setting] = json.loads(r.stdout.strip().splitlines()[-1])
        _children[setting]["dX"] = dict(np.load(dump))
        os.remove(dump)
        os.rmdir(os.path.dirname(dump))
        print(r.stderr[-200000:])
    return _children[setting]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_switch_setting(hip, setting):
    """Under each setting: the child saw the switches, ran child_cases(), every tensor of every case is within the bounds of (a), no
    invariant broke, and every output whose route() entry the setting leaves unchanged has the digest of the default-switch in-process
    run (the kernels are deterministic: fixed summation orders throughout).  No digest is compared ACROSS kernels: "same formulas,
    same summation order over (ci, r, s)" (conv2d.hip, above the direct kernels) describes the one-thread-per-position kernels; the quad
    kernels split the reduction channels over four lanes and add the four partial sums in a tree, and the implicit-GEMM kernels sum in
    MFMA order, so neither is promised the bits of the other.  The one cross-kernel promise, quad2 against quad, has its own test below."""
    res = child(setting)
    want_env = setting_env(setting)
    assert {k: v for k, v in res["env"].items() if v != ""} == want_env
    cc = child_cases()
    assert list(res["cases"]) == [c.name for c in cc]
    sw = switches(setting)
    part_of = dict(O="fwd", O_nobias="fwd", dX="dgrad", dW="wgrad", db="wgrad")
    worst_ratio, compared, moved = {k: 0.0 for k in TENSORS}, 0, 0
    for c in cc:
        r = res["cases"][c.name]
        assert not r["problems"], (c.name, r["problems"])
        base, r0, r1 = default_run(c.name), route(c.desc), route(c.desc, sw)
        for k in TENSORS:
            assert r["ratios"][k] <= 1.0, (c.name, k, r["ratios"][k])
            worst_ratio[k] = max(worst_ratio[k], r["ratios"][k])
            if r0[part_of[k]] == r1[part_of[k]]:
                compared += 1
                assert r["digests"][k] == base["digests"][k], f"{c.name} {k}: the setting does not touch this route, yet the bits differ"
            else:
                moved += 1
    print(f"\n[conv child {setting}] {want_env}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst_ratio.items()) +
          f"; {moved} outputs on another kernel or plan, {compared} bit-identical to the default run")
    assert moved >= MIN_MOVED[setting]


def test_fused_switches_off(hip):
    """NNHIP_CONV_POOL_FWD=0, NNHIP_CONV_POOLED_WGRAD=0 and NNHIP_CONV_DEFER_REDUCE=0 together, in a fresh process (conv_child.py
    --fused-off: a few seconds, three small shapes).  route() has no entry they move, so they are no part of conv_ref.ENV; their default
    state is what pf_*, pw_* and test_deferred_reduce_queue run.  Off: the two queries answer 0 for the first fused cases (this process,
    with the defaults, answers 1), and nt_c8_o16's dW and db from a deferred nnhipConv2dBackward -- reduced at once, not queued -- are
    the bits of the default run."""
    from conv_child import FUSED_OFF
    if _dead:
        pytest.fail(f"an earlier child process ended abnormally ({_dead[0]}); no further child is started")
    _, df, _ = POOL_FWD_CASES[0]
    _, dw, win, _ = POOL_WGRAD_CASES[0]
    assert call("nnhipConv2dLeakyMaxPoolForwardOk", cdesc(df), cpool(pool_of(df))) == 1
    assert call("nnhipConv2dWeightGradPooledOk", cdesc(dw), cpool(pool_of(dw, *win))) == 1
    base = default_run("nt_c8_o16")
    env = {k: v for k, v in os.environ.items() if not k.startswith("NNHIP_CONV_")}
    env.update({k: "0" for k in FUSED_OFF})
    try:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_child.py"), "--fused-off"], env=env,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append("fused-off: timeout")
        pytest.fail(_dead[0])
    if r.returncode < 0 or r.returncode in (134, 139):
        _dead.append(f"fused-off: status {r.returncode}")
        pytest.fail(_dead[0] + "\n" + r.stderr[-4000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["env"] == {k: "0" for k in FUSED_OFF}
    assert res["pool_fwd_ok"] == 0 and res["pooled_wgrad_ok"] == 0
    assert res["guards_intact"]
    assert res["digests"] == {k: base["digests"][k] for k in ("dW", "db")}, "deferral ignored: dW / db differ from the default run"


def test_quad2_against_quad(hip):
    """conv2d.hip on conv_direct_dgrad_quad2_kernel: "Same products in the same order per output (co = s, s + 4, ...; taps in order;
    quad tree)" as the position-per-quad kernel.  That is a statement about the source, not about the bits: the compiler contracts
    every multiply-add of quad2 into an FMA, but compiles 32 of the 144 multiply-adds per accumulator of the position-per-quad kernel
    (its channel groups co >= 8) to packed multiplies and separate additions (gfx950 disassembly), so those products are rounded once
    more and the additions after them round differently.  Asserted: the switch moves every quad2 case to the other kernel and the two
    results lie within the sum of the bounds each is held to against float64.  Printed, not asserted (it is the compiler's choice):
    how many cases are bit-identical and the largest difference in units of 2^-24 sum |a||b|.  First MI355X run: 8 of 12 identical
    (every case with Cout <= 8: there the uncontracted products multiply zeros), 0.92 units at Cout = 16."""
    res = child("quad1")
    n = same = 0
    units = 0.0
    for c in child_cases():
        if route(c.desc)["dgrad"]["kernel"].startswith("conv_direct_dgrad_quad2_kernel"):
            assert route(c.desc, switches("quad1"))["dgrad"]["kernel"].startswith("conv_direct_dgrad_quad_kernel")
            _, Wt, _, dO = make_inputs(c.name, c.desc)
            a, b = res["dX"][c.name], default_run(c.name)["host"]["dX"]
            assert worst(a, b.astype(np.float64), 2 * references(c)["dX"][1]) <= 1.0, c.name
            units = max(units, worst(a, b.astype(np.float64), U24 * dgrad_abs_sum(Wt, dO, c.desc) + 1e-30))
            same += res["cases"][c.name]["digests"]["dX"] == default_run(c.name)["digests"]["dX"]
            n += 1
    print(f"\n[conv quad2 vs quad] {n} cases, {same} bit-identical; largest |difference| = {units:.3f} x 2^-24 sum |a||b|")
    assert n >= 10
