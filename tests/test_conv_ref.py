"""CPU: tests/conv_ref.py held against the oracle and the reference's fixtures, route() held against the figures the sources' own comments
state, the instantiation coverage of the case table, the reciprocal divisions of conv_mfma_wgrad_kernel, and the near-tie share of the
fused forward's cases.  No GPU, no library."""
import numpy as np
import pytest

from oracle import neunet_oracle as O
from conv_ref import (CASES, BY_NAME, POOL_FWD_CASES, POOL_STATS_CASES, POOL_WGRAD_CASES, SETTINGS, U24, ConvDesc, child_cases,
                      conv2d_backward64, conv2d_forward64, conv_leaky_pool64, dgrad_abs_sum, dot_rule, forward_abs_sum, kernels_of,
                      make_inputs, near_ties, pooled_dO32, recip_div, route, switches)
from vision_ref import PoolDesc

SMALL = [c for c in CASES if not c.big]
ALPHAS = (0.01, 1.0)
TIE_CAP = 0.005


def pool_of(d, kh=2, kw=2):
    Ho, Wo = d.out_hw()
    return PoolDesc(d.B, d.Cout, Ho, Wo, kh, kw)


def oracle_args(d):
    return (d.sh, d.sw), (d.pu, d.pd, d.pl, d.pr), (d.dh, d.dw)


# ===================================================================================================== conv_ref against the oracle
@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_reference_agrees_with_oracle(case):
    """conv2d_forward64 / backward64 against oracle.conv2d_forward / backward (float32 einsums) within the oracle's own rounding:
    32 x 2^-24 x sum |a||b| per element (dot_bound, c = 32) + four roundings of the result."""
    d = case.desc
    X, Wt, b, dO = make_inputs(case.name, d)
    st, pad, dil = oracle_args(d)
    ref = conv2d_forward64(X, Wt, b, d)
    got = O.conv2d_forward(X, Wt, b, st, pad, dil)
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= dot_rule(ref, forward_abs_sum(X, Wt, d)))
    dX, dW, db = conv2d_backward64(X, Wt, dO, d)
    oX, oW, ob = O.conv2d_backward(X, Wt, True, dO, st, pad, dil)
    assert np.all(np.abs(oX - dX) <= dot_rule(dX, dgrad_abs_sum(Wt, dO, d)))
    _, aW, ab = conv2d_backward64(np.abs(X), Wt, np.abs(dO), d)
    assert np.all(np.abs(oW - dW) <= dot_rule(dW, aW))
    assert np.all(np.abs(ob - db) <= dot_rule(db, ab))


@pytest.mark.parametrize("name", ["conv2d_s2p1d2", "conv2d_s2_uncovered", "conv2d_pad4", "conv2d_c5_l1", "conv2d_c5_l2"])
def test_reference_agrees_with_fixtures(golden, name):
    """The reference's recorded results, at the tolerance tests/test_oracle_golden.py holds the oracle to."""
    g = golden(name)
    Cout, Cin, kh, kw = g["W"].shape
    B, _, H, W = g["X"].shape
    d = ConvDesc(B, Cin, H, W, Cout, (kh, kw), tuple(int(s) for s in g["stride"]), tuple(int(p) for p in g["padding4"]),
                 tuple(int(v) for v in g["dilation"]))
    np.testing.assert_allclose(conv2d_forward64(g["X"], g["W"], g["b"].reshape(-1), d), g["O"], rtol=1e-5, atol=1e-5)
    dX, dW, db = conv2d_backward64(g["X"], g["W"], g["dO"], d)
    np.testing.assert_allclose(dX, g["dX"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dW, g["dW"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(db, g["db"].reshape(-1), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name,d,why", POOL_FWD_CASES[2:] + POOL_STATS_CASES, ids=[c[0] for c in POOL_FWD_CASES[2:] + POOL_STATS_CASES])
def test_fused_chain_agrees_with_oracle(name, d, why, alpha):
    """conv_leaky_pool64 against oracle.maxpool2d_forward(leaky_relu_forward(conv2d_forward)) in float32: the pooled value within the
    largest bound of the window's four values; the arg-max equal except at the near-ties (either index there)."""
    X, Wt, b, _ = make_inputs(name, d)
    P, arg, V, Vb = conv_leaky_pool64(X, Wt, b, alpha, d)
    conv = O.conv2d_forward(X, Wt, b, *oracle_args(d))
    act = conv if alpha == 1.0 else O.leaky_relu_forward(conv, np.float32(alpha))
    oP, oarg = O.maxpool2d_forward(act, (2, 2))
    tie = near_ties(V, Vb)
    assert np.array_equal(oarg[~tie], arg[~tie])
    wb = Vb.reshape(d.B, d.Cout, P.shape[2], 2, P.shape[3], 2).max(axis=(3, 5))
    assert np.all(np.abs(oP - P) <= wb)


# ===================================================================================================== coverage
# Every kernel instantiation the host code of conv2d.hip / conv_mfma.hip can launch on behalf of Conv2d, from the hipLaunchKernelGGL and
# launch_* sites (conv_direct_forward, conv_pool_forward, conv_direct_dgrad, conv_small_wgrad's launch_mfma_wgrad_plan and
# launch_direct_wgrad_width, launch_conv_tap, conv_mfma_wgrad, conv_reduce_launch, conv_reduce_group_launch).
WANTED = [
    "conv_direct_fwd_kernel<4>", "conv_direct_fwd_kernel<8>", "conv_direct_fwd_kernel<16>", "conv_direct_fwd_quad_kernel<8>",
    "conv_direct_fwd_quad_kernel<16>", "conv_direct_dgrad_kernel<4>", "conv_direct_dgrad_kernel<8>", "conv_direct_dgrad_kernel<16>",
    "conv_direct_dgrad_quad_kernel<4>", "conv_direct_dgrad_quad_kernel<8>", "conv_direct_dgrad_quad2_kernel<4>",
    "conv_direct_dgrad_quad2_kernel<8>", "conv_pool_fwd_kernel<8>", "conv_pool_fwd_kernel<16>", "conv_pool_fwd_quad_kernel<8,false>",
    "conv_pool_fwd_quad_kernel<8,true>", "conv_pool_fwd_quad_kernel<16,false>", "conv_pool_fwd_quad_kernel<16,true>",
    "conv_direct_wgrad_kernel<8,1>", "conv_direct_wgrad_kernel<8,2>", "conv_direct_wgrad_kernel<8,4>", "conv_direct_wgrad_kernel<8,8>",
    "conv_direct_wgrad_kernel<8,16>", "conv_direct_wgrad_kernel<16,1>", "conv_direct_wgrad_kernel<16,2>",
    "conv_direct_wgrad_kernel<16,4>", "conv_direct_wgrad_kernel<16,8>", "conv_direct_wgrad_kernel<16,16>",
    "conv_mfma_wgrad_kernel<1,false>", "conv_mfma_wgrad_kernel<1,true>", "conv_mfma_wgrad_kernel<2,false>",
    "conv_mfma_wgrad_kernel<2,true>", "conv_mfma_wgrad_kernel<3,false>", "conv_mfma_wgrad_kernel<3,true>",
    "conv_mfma_wgrad_kernel<5,false>", "conv_mfma_wgrad_kernel<5,true>", "conv_mfma_wgrad_kernel<10,false>",
    "conv_mfma_wgrad_kernel<10,true>", "conv_tap_kernel<fwd,1>", "conv_tap_kernel<fwd,2>", "conv_tap_kernel<dgrad,1>",
    "conv_tap_kernel<dgrad,2>", "conv_tap_reduce_kernel", "conv_repack_kernel", "conv_wgrad_reduce_kernel",
    "conv_wgrad_mfma_reduce_kernel", "conv_wgrad_mfma_kernel<1,32,false,false>", "conv_wgrad_mfma_kernel<1,32,false,true>",
    "conv_wgrad_mfma_kernel<1,32,true,false>", "conv_wgrad_mfma_kernel<1,32,true,true>", "conv_wgrad_mfma_kernel<1,64,false,false>",
    "conv_wgrad_mfma_kernel<1,64,false,true>", "conv_wgrad_mfma_kernel<1,64,true,false>", "conv_wgrad_mfma_kernel<1,64,true,true>",
    "conv_wgrad_mfma_kernel<1,128,false,false>", "conv_wgrad_mfma_kernel<1,128,false,true>", "conv_wgrad_mfma_kernel<1,128,true,false>",
    "conv_wgrad_mfma_kernel<1,128,true,true>", "conv_wgrad_mfma_kernel<1,256,false,false>", "conv_wgrad_mfma_kernel<1,256,false,true>",
    "conv_wgrad_mfma_kernel<1,256,true,false>", "conv_wgrad_mfma_kernel<1,256,true,true>", "conv_wgrad_mfma_kernel<2,32,false,false>",
    "conv_wgrad_mfma_kernel<2,32,false,true>", "conv_wgrad_mfma_kernel<2,32,true,false>", "conv_wgrad_mfma_kernel<2,32,true,true>",
    "conv_wgrad_mfma_kernel<2,64,false,false>", "conv_wgrad_mfma_kernel<2,64,false,true>", "conv_wgrad_mfma_kernel<2,64,true,false>",
    "conv_wgrad_mfma_kernel<2,64,true,true>", "conv_wgrad_mfma_kernel<2,128,false,false>", "conv_wgrad_mfma_kernel<2,128,false,true>",
    "conv_wgrad_mfma_kernel<2,128,true,false>", "conv_wgrad_mfma_kernel<2,128,true,true>",
]
# launched, but chosen by the state of the deferred-reduce queue, not by a descriptor: test_conv_tiers_gpu.py::test_deferred_reduce_queue
NOT_BY_DESCRIPTOR = {"conv_wgrad_reduce_group_kernel": "two or more queued reduces at a flush (conv_reduce_group_launch); no descriptor selects it"}
# instantiated and launchable by the host code, but no descriptor reaches them: none.  (conv_mfma_wgrad_kernel's 2 x 2 POOL branch on the
# general path needs an odd nXp = Cin Hp Wp next to an even Wo; unit stride makes Wp = Wo + 2 even, stride 2 makes it odd: pw_c3_22_oddnxp.)
UNREACHABLE = {}


def reached(setting=None):
    sw = switches(setting)
    cases = CASES if setting is None else child_cases()
    names = set()
    for c in cases:
        names |= kernels_of(route(c.desc, sw))
    if setting is None:
        for _, d, _ in POOL_FWD_CASES:
            names |= kernels_of({"p": route(d, sw, pool=pool_of(d))["pool_fwd"]})
        for _, d, _ in POOL_STATS_CASES:
            names |= kernels_of({"p": route(d, sw, pool=pool_of(d), stats=True)["pool_fwd"]})
        for _, d, pool, _ in POOL_WGRAD_CASES:
            names |= kernels_of({"p": route(d, sw, pool=pool_of(d, *pool))["pool_wgrad"]})
    return names


def test_every_instantiation_has_a_case():
    assert len(WANTED) == len(set(WANTED)) == 74
    got = reached()
    for s in SETTINGS:
        got |= reached(s)
    missing = [k for k in WANTED if k not in got and k not in UNREACHABLE]
    assert not missing, missing
    assert not (got - set(WANTED)), got - set(WANTED)                       # route() names nothing the list does not know
    assert not (set(UNREACHABLE) & got)


def test_default_routes_of_the_named_cases():
    """The routes the case table promises, through route() at the default switches."""
    r = {n: route(c.desc) for n, c in BY_NAME.items()}
    k = lambda n, part: r[n][part]["kernel"]                                # noqa: E731
    assert (k("big_fwd_c11", "fwd"), k("big_fwd_c11", "dgrad")) == ("conv_direct_fwd_kernel<8>", "conv_direct_dgrad_kernel<16>")
    assert r["big_fwd_c11"]["fwd"]["path"] == "3x3 buffer" and k("big_fwd_c11", "wgrad") == "conv_wgrad_mfma_kernel<1,32,true,false>"
    assert k("big_dgrad_c5", "dgrad") == "conv_direct_dgrad_kernel<8>" and r["big_dgrad_c5"]["dgrad"]["path"] == "3x3 buffer"
    assert k("dwg_c16", "wgrad") == "conv_direct_wgrad_kernel<8,16>" and (r["dwg_c16"]["wgrad"]["wg_lds"], r["dwg_c16"]["wgrad"]["m_lds"]) == (56784, 63712)
    assert k("dwg_c1", "wgrad") == "conv_direct_wgrad_kernel<8,1>" and (r["dwg_c1"]["wgrad"]["wg_lds"], r["dwg_c1"]["wgrad"]["m_lds"]) == (60552, 61988)
    assert k("dwg_c16_o4", "wgrad") == "conv_mfma_wgrad_kernel<10,false>" and r["dwg_c16_o4"]["wgrad"]["m_lds"] == 61008
    assert k("dwg_c16_o7", "wgrad").startswith("conv_wgrad_mfma_kernel<1,32") and k("igemm_c16_32", "wgrad").startswith("conv_wgrad_mfma_kernel<1,32")
    assert k("dwg_c1_86", "wgrad") == "conv_mfma_wgrad_kernel<1,false>" and k("dwg_c1_88", "wgrad").startswith("conv_wgrad_mfma_kernel")
    nts = {(ci, co): (r[f"nt_c{ci}_o{co}"]["wgrad"]["nt"], r[f"nt_c{ci}_o{co}"]["wgrad"]["nt_inst"]) for ci in (1, 3, 5, 6, 8, 9, 16) for co in (1, 7, 16)}
    assert {nts[(ci, 7)] for ci in (1, 3, 5, 6, 8, 9, 16)} == {(1, 1), (2, 2), (3, 3), (4, 5), (5, 5), (6, 10), (10, 10)}
    for n in ("taps49_c3", "taps26_c2"):
        f, w = r[n]["fwd"], r[n]["wgrad"]
        assert f["kernel"] == "conv_tap_kernel<fwd,1>" and f["Csp"] == 16 and f["Mp"] == 64 and w["CB"] == 32 and w["tgroups"] > 1
    assert r["taps49_c3"]["wgrad"]["tgroups"] == 7 and r["taps26_c2"]["wgrad"]["tgroups"] == 4
    assert k("taps25_c3", "fwd") == "conv_direct_fwd_kernel<4>" and r["taps25_c3"]["fwd"]["path"] == "generic"
    assert k("lim_c16_o16", "fwd").startswith("conv_direct") and k("lim_c17_o16", "fwd").startswith("conv_tap") and k("lim_c16_o17", "dgrad").startswith("conv_tap")
    assert (k("quad_c3_o5", "fwd"), k("quad_c4_o4", "fwd"), k("quad_c4_o5", "fwd")) == \
        ("conv_direct_fwd_kernel<8>", "conv_direct_fwd_kernel<4>", "conv_direct_fwd_quad_kernel<8>")
    assert (k("quad_c3_o5", "dgrad"), k("nt_c8_o16", "dgrad"), k("quad_c9_o5", "dgrad"), k("nt_c3_o1", "dgrad")) == \
        ("conv_direct_dgrad_quad2_kernel<4>", "conv_direct_dgrad_quad2_kernel<8>", "conv_direct_dgrad_kernel<16>", "conv_direct_dgrad_kernel<4>")
    assert (k("quad_s2", "dgrad"), k("quad_d2", "dgrad")) == ("conv_direct_dgrad_quad_kernel<4>", "conv_direct_dgrad_quad_kernel<8>")
    for part, M in (("fwd", 20), ("dgrad", 17)):
        p = r["tile64_main_tail"][part]
        assert (p["wm"], p["M"], p["tiles"], p["tn_main"], p["tail"]) == (1, M, 781, 768, 13) and p["splits"] > 1
    assert (k("asym_direct", "fwd"), k("asym_quad", "fwd"), k("asym_quad", "wgrad"), k("asym_igemm", "fwd")) == \
        ("conv_direct_fwd_kernel<4>", "conv_direct_fwd_quad_kernel<8>", "conv_mfma_wgrad_kernel<5,false>", "conv_tap_kernel<fwd,1>")
    assert k("c200_o24", "wgrad") == "conv_wgrad_mfma_kernel<1,256,false,true>" and k("c200_o65", "wgrad") == "conv_wgrad_mfma_kernel<2,128,false,true>"
    assert r["c200_o65"]["wgrad"]["cblks"] == 2


def test_child_settings_change_kernels():
    """Each switch setting moves enough child cases to another kernel (or plan) to be worth its process."""
    cc = child_cases()
    base = {c.name: route(c.desc) for c in cc}

    def moved(setting, part, pred=lambda new: True):
        sw = switches(setting)
        return sum(1 for c in cc if route(c.desc, sw)[part] != base[c.name][part] and pred(route(c.desc, sw)[part]))
    assert moved("nosplit", "fwd", lambda n: n["kernel"].startswith("conv_direct_fwd_kernel")) >= 12
    assert moved("nosplit", "dgrad", lambda n: n["kernel"].startswith("conv_direct_dgrad_kernel")) >= 10
    assert moved("nosplit", "wgrad", lambda n: n["kernel"].startswith("conv_direct_wgrad_kernel")) >= 25
    assert moved("nosplit", "fwd", lambda n: n["kernel"].startswith("conv_tap") and n["tail"] == 0) >= 8
    assert moved("nosplit", "wgrad", lambda n: n["kernel"].endswith("false>") and n["kernel"].startswith("conv_wgrad_mfma")) >= 8
    assert moved("igemm", "fwd", lambda n: n["kernel"].startswith("conv_tap")) >= 30
    assert moved("igemm", "dgrad", lambda n: n["kernel"].startswith("conv_tap")) >= 30
    assert moved("igemm", "wgrad", lambda n: n["kernel"].startswith("conv_wgrad_mfma") and n["kernel"].endswith("true>")) >= 30
    assert moved("quad1", "dgrad", lambda n: n["kernel"].startswith("conv_direct_dgrad_quad_kernel")) >= 10
    assert moved("quad1", "fwd") == 0 and moved("quad1", "wgrad") == 0
    ten = {route(c.desc, switches("nosplit"))["wgrad"]["kernel"] for c in cc}
    assert {f"conv_direct_wgrad_kernel<{co},{cip}>" for co in (8, 16) for cip in (1, 2, 4, 8, 16)} <= ten
    assert 35 <= len(cc) <= 70


# ===================================================================================================== the sources' own figures
def test_route_reproduces_the_figures_in_the_comments():
    # conv_mfma.hip, launch_conv_tap: "64->128 ch 56x56 B64: 1568 tiles = 3.06 rounds of 512"
    f = route(ConvDesc(64, 64, 56, 56, 128, 3, pad=1))["fwd"]
    assert (f["wm"], f["tiles"], f["tn_main"], f["tail"]) == (2, 1568, 1536, 32) and f["splits"] > 1
    # test_hip_parity.py: "541 pixel tiles: one whole round of 512 + 29" for (18, 32, 62, 62 -> 72)
    f = route(ConvDesc(18, 32, 62, 62, 72, 3, pad=1))["fwd"]
    assert (f["tiles"], f["tn_main"], f["tail"]) == (541, 512, 29)
    # conv2d.hip: C5's second layer takes the quad kernels, its first the one-thread-per-window fused forward
    l2 = ConvDesc(256, 8, 14, 14, 16, 3, pad=1)
    r = route(l2, pool=pool_of(l2))
    assert (r["fwd"]["kernel"], r["dgrad"]["kernel"], r["pool_fwd"]["kernel"]) == \
        ("conv_direct_fwd_quad_kernel<16>", "conv_direct_dgrad_quad2_kernel<8>", "conv_pool_fwd_quad_kernel<16,false>")
    l1 = ConvDesc(256, 1, 28, 28, 8, 3, pad=1)
    r = route(l1, pool=pool_of(l1))
    assert r["pool_fwd"]["kernel"] == "conv_pool_fwd_kernel<8>" and r["pool_wgrad"]["kernel"] == "conv_mfma_wgrad_kernel<1,true>"
    assert route(l2, pool=pool_of(l2), stats=True)["pool_fwd"] == dict(kernel="conv_pool_fwd_quad_kernel<16,true>", aux=[], stats_blocks=196)


# ===================================================================================================== reciprocal divisions
def test_reciprocal_division_is_exact_below_the_lds_limit():
    """conv_mfma_wgrad_kernel takes p / Wo as (int)((p + 0.5f) * (1.0f / Wo)) ("exact for the pixel counts that fit LDS"); its POOL path
    does the same with HWq and Wq.  Exhaustive over every divisor 1 .. 15360 and every p < 15360 (60 KiB / 4 B: the most pixels LDS
    holds).  Raising the LDS limit, or reordering the expression, has to pass here first."""
    n = 60 * 1024 // 4
    p = np.arange(n)
    step = 256
    for d0 in range(1, n + 1, step):
        div = np.arange(d0, min(d0 + step, n + 1))[:, None]
        bad = np.argwhere(recip_div(np.broadcast_to(p, (div.shape[0], n)), div) != p[None, :] // div)
        assert bad.size == 0, (int(div[bad[0][0], 0]), int(p[bad[0][1]]))


# ===================================================================================================== near-ties of the fused cases
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name,d,why", POOL_FWD_CASES + POOL_STATS_CASES, ids=[c[0] for c in POOL_FWD_CASES + POOL_STATS_CASES])
def test_near_tie_share_is_under_the_cap(name, d, why, alpha):
    """The windows excluded from the arg-max comparison of the fused forward (float64 top two closer than the sum of their bounds)
    are at most 0.5 % of each case -- evaluated with the float64 reference alone; the GPU test asserts the same share again."""
    X, Wt, b, _ = make_inputs(name, d)
    _, _, V, Vb = conv_leaky_pool64(X, Wt, b, alpha, d)
    assert near_ties(V, Vb).mean() <= TIE_CAP


def test_pooled_zero_rule():
    """The rule tests/test_conv_tiers_gpu.py::test_pooled_weight_gradient holds the kernel to, on the reference itself: a pooled value of +0.0 or -0.0 scales the gradient by alpha."""
    dP = np.ones((1, 1, 1, 3), np.float32)
    pooled = np.array([0.0, -0.0, 1e-30], np.float32).reshape(1, 1, 1, 3)
    dO = pooled_dO32(dP, np.zeros((1, 1, 1, 3), np.int32), pooled, 0.25, (1, 1))
    assert dO.reshape(-1).tolist() == [0.25, 0.25, 1.0]


def test_bound_constants():
    assert U24 == 2.0 ** -24 and dot_rule(np.array([2.0]), np.array([3.0]))[0] == 32 * U24 * 3 + 4 * U24 * 2 + 1e-30
