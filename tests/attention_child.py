"""Seeded attention problems, one nnhipAttentionForwardEx (+ nnhipAttentionBackwardEx) call through the C ABI with every output in a
NaN-filled, NaN-fenced buffer, and the comparison of a set of outputs with the float64 restatement (tests/attention_ref.py) under the
project's bound, 1e-4 of max(|ref|, rms(ref)) per element.  tests/test_attention_ref.py uses the problems and the comparison on the CPU.

Run as a script it is a fresh process for the switches the library reads once (NNHIP_ATTN_PAIR, NNHIP_ATTN_WAVES; needs a GPU):
python tests/attention_child.py   runs child_cases() under whatever the environment says, compares every tensor of every case with
float64 and prints ONE JSON object: the environment it saw and, per case, the shares of the bound, the worst error / bound ratio and
sha256 digests of O and LSE."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "numpy-nn-model_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from attention_ref import LOG2E, MASKED, attention, heads  # noqa: E402
from lstm_abi import Fenced, dev  # noqa: E402

TOL = 1e-4
MASKED2 = np.float32(np.float32(MASKED) * np.float32(LOG2E))   # AT_MASKED2 of csrc/attention.h: the -1e9 fill in log2 units, in float32
TENSORS = ("O", "LSE", "dQ", "dK", "dV")


# ------------------------------------------------------------------------------------------------------------------ dispatch
def block_rows(dh, waves=2):
    """Query rows per forward / dQ block (= keys per dK/dV block): 64 at head dim 64 with 2-wave blocks, else 128."""
    return 64 if dh == 64 and waves == 2 else 128


def pair_mode(BH, Tq, Tk, dh, causal, gen, waves=2, forced=-1):
    """The forward's dispatch restated (attn_pair() and attn_sb_applicable() in csrc/): does this call run in pair mode?"""
    if causal and not gen and Tq == 256 and Tk == 256 and dh == 64:
        return False                                            # the balanced T = 256 kernels (attention_sb.hip)
    nblk = -(-Tq // block_rows(dh, waves))
    if forced == 0:
        return False
    if forced == 1:
        return nblk >= 2
    return bool(causal) and 2 <= nblk <= 8 and BH * ((nblk + 1) // 2) >= 512


# ------------------------------------------------------------------------------------------------------------------- problems
def key_pattern(rng, name, Tk, lead=None):
    kv = np.ones(Tk, np.int32)
    if name == "trailing":
        kv[Tk - Tk // 5:] = 0
    elif name == "holes":
        kv = (rng.random(Tk) >= 0.2).astype(np.int32)
        kv[0] = 1
    elif name == "leading":                                    # under a causal mask the first rows see no key at all
        kv = (rng.random(Tk) >= 0.2).astype(np.int32)
        L = Tk // 3 if lead is None else min(lead, Tk - 1)
        kv[:L] = 0
        kv[L] = 1
    else:
        assert name == "none", name
    return kv


def make_problem(seed, B, H, Tq, Tk, dh, pads=("trailing", "holes", "leading"), mul=1.5, lead=None):
    """q, k ~ mul N(0, 1), v, dO ~ N(0, 1), scale = sqrt(8 dh) (the notebook's sqrt(d_model) at 8 heads): scores of standard deviation
    mul^2 / sqrt(8), a softmax that is neither flat nor one-hot.  Batch row b < len(pads) carries padding pattern pads[b]."""
    rng = np.random.default_rng(seed)
    D = H * dh
    p = dict(B=B, H=H, Tq=Tq, Tk=Tk, dh=dh, scale=float(np.sqrt(8.0 * dh)),
             q=(rng.standard_normal((B, Tq, D)) * mul).astype(np.float32), k=(rng.standard_normal((B, Tk, D)) * mul).astype(np.float32),
             v=rng.standard_normal((B, Tk, D)).astype(np.float32), dO=rng.standard_normal((B, Tq, D)).astype(np.float32), kv=None)
    if pads:
        p["kv"] = np.stack([key_pattern(rng, pads[b] if b < len(pads) else "none", Tk, lead) for b in range(B)])
    return p


def injected_dropout(seed, p, prob=0.1):
    return ((np.random.default_rng(seed).random((p["B"], p["H"], p["Tq"], p["Tk"])) >= prob) / (1.0 - prob)).astype(np.float32)


def random_dense(seed, p, empty_rows=(3,)):
    """A dense [B, Tq, Tk] mask: causal-or-not random visibility with a few rows without any visible key."""
    rng = np.random.default_rng(seed)
    m = (rng.random((p["B"], p["Tq"], p["Tk"])) >= 0.4).astype(np.int32)
    for r in empty_rows:
        if r < p["Tq"]:
            m[0, r] = 0
    return m


def hash_dropout(p, prob, seed):
    """The multipliers the kernels' counter hash yields for (prob, seed) (nnhipAttentionDropoutMask), as a host array."""
    import torch
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    out = torch.empty((p["B"], p["H"], p["Tq"], p["Tk"]), dtype=torch.float32, device="cuda")
    call_hip_function("nnhipAttentionDropoutMask", out, p["B"], p["H"], p["Tq"], p["Tk"], float(prob), int(seed), get_current_stream_ptr())
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------- one call
def run(p, causal, drop=None, dense=None, dropout_p=0.0, seed=0, backward=True, ld3=False, batch=None, ld=None, dO=None, entry="Ex"):
    """One forward (+ one backward on the forward's own O and LSE) through nnhipAttention{Forward,Backward}Ex.  drop: injected
    multipliers [B, H, Tq, Tk]; dense: [B, Tq, Tk] int mask; dropout_p / seed: the hash RNG.  ld3: q, k, v are the three column
    blocks of one [B, T, 3D] buffer and dQ, dK, dV those of another.  batch = (b0, b1): only those batch rows (a sub-batch call).
    ld: the ld_qkv argument (default H * dh; 0 means the same).  entry: "Ex" (opts = NULL unless something asks for the GEN kernels),
    "zeroed" (a zero-filled options struct) or "plain" (nnhipAttentionForward / nnhipAttentionBackward).
    Every output is NaN-filled and fenced; returns {O, LSE, dQ, dK, dV} as host arrays."""
    import torch
    from neunet_hip._lib import AttentionOptions, StridedView, call_hip_function, get_current_stream_ptr
    from neunet_hip.nn.experimental.attention import pack_attention_mask
    b0, b1 = batch or (0, p["B"])
    B, H, Tq, Tk, dh = b1 - b0, p["H"], p["Tq"], p["Tk"], p["dh"]
    D = H * dh
    st = get_current_stream_ptr()
    q, k, v, g = (np.ascontiguousarray(a[b0:b1]) for a in (p["q"], p["k"], p["v"], p["dO"] if dO is None else dO))
    if ld3:
        assert Tq == Tk
        buf = dev(np.concatenate([q, k, v], -1))
        qd, kd, vd = buf[..., 0:D], buf[..., D:2 * D], buf[..., 2 * D:]
        ldv = 3 * D
    else:
        qd, kd, vd = dev(q), dev(k), dev(v)
        ldv = D if ld is None else ld
    kvd = None if p["kv"] is None else torch.from_numpy(np.ascontiguousarray(p["kv"][b0:b1])).cuda()
    cs, keep = None, []
    if drop is not None or dense is not None or dropout_p:
        cs = AttentionOptions()
        if dense is not None:
            keep = list(pack_attention_mask(torch.from_numpy(np.ascontiguousarray(dense[b0:b1], np.int32)).cuda()))
            cs.mask_bits, cs.mask_bitsT, cs.row_any = (t.data_ptr() for t in keep)
        if drop is not None:
            keep.append(dev(drop[b0:b1]))
            cs.dropout_mask = keep[-1].data_ptr()
        else:
            cs.dropout_p, cs.dropout_seed = float(dropout_p), int(seed) & 0xFFFFFFFF
    if entry == "zeroed":
        assert cs is None
        cs = AttentionOptions()
    opt = () if entry == "plain" else (None if cs is None else ctypes.byref(cs),)
    ex = "" if entry == "plain" else "Ex"
    fO, fL = Fenced(B, Tq, D), Fenced(B, H, Tq, 2)
    call_hip_function("nnhipAttentionForward" + ex, StridedView(qd), StridedView(kd), StridedView(vd), kvd, fO.view, fL.view, B, H, Tq, Tk, dh,
                      ldv, 1.0 / p["scale"], int(causal), *opt, st)
    torch.cuda.synchronize()
    out = dict(O=fO.host(), LSE=fL.host())
    fences = [fO, fL]
    if backward:
        gd = dev(g)
        if ld3:
            fG = Fenced(B, Tq, 3 * D)
            dq, dk, dv = fG.view[..., 0:D], fG.view[..., D:2 * D], fG.view[..., 2 * D:]
            fences.append(fG)
        else:
            fq, fk, fv = Fenced(B, Tq, D), Fenced(B, Tk, D), Fenced(B, Tk, D)
            dq, dk, dv = fq.view, fk.view, fv.view
            fences += [fq, fk, fv]
        call_hip_function("nnhipAttentionBackward" + ex, StridedView(qd), StridedView(kd), StridedView(vd), kvd, fO.view, gd, fL.view,
                          StridedView(dq), StridedView(dk), StridedView(dv), B, H, Tq, Tk, dh, ldv, 1.0 / p["scale"], int(causal), *opt, st)
        torch.cuda.synchronize()
        out.update(dQ=dq.cpu().numpy(), dK=dk.cpu().numpy(), dV=dv.cpu().numpy())
        np.testing.assert_array_equal(fO.host(), out["O"], err_msg="O changed by the backward")
        np.testing.assert_array_equal(fL.host(), out["LSE"], err_msg="LSE changed by the backward")
    for f in fences:
        assert f.guards_intact(), "a kernel wrote outside an output buffer"
    call_hip_function("nnhipDeviceError")
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


# ----------------------------------------------------------------------------------------------------- against the restatement
def rms_of(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a ** 2))) if a.size else 0.0


def project_bound(ref, zero_scale=0.0):
    """assert_close_scaled(tol = 1e-4): TOL * max(|ref|, rms(ref)[, the un-cancelled magnitude of a tensor that is identically zero])."""
    ref = np.asarray(ref, np.float64)
    return TOL * np.maximum(np.maximum(np.abs(ref), rms_of(ref)), zero_scale) + 1e-30


def share(got, ref, zero_scale=0.0):
    """Worst element's |got - ref| as a fraction of the project bound."""
    ref = np.asarray(ref, np.float64)
    if not ref.size:
        return 0.0
    r = np.abs(np.asarray(got, np.float64) - ref) / project_bound(ref, zero_scale)
    return float(np.max(np.where(np.isfinite(r), r, np.inf)))


def bound_for(ref64, ref32, what, zero_scale=0.0):
    """The rule of tests/test_lstm_tiers_gpu.py: the project bound -- unless the float32 RESTATEMENT alone is further than a quarter of
    it from float64: then max(that, 4 x max|ref32 - ref64|), under the asserted condition that this stays below 1 % of the tensor's
    rms.  Computed from the two references only, never from the kernel."""
    ref64 = np.asarray(ref64, np.float64)
    bound = project_bound(ref64, zero_scale)
    if share(ref32, ref64, zero_scale) > 0.25:
        wide = 4.0 * float(np.max(np.abs(np.asarray(ref32, np.float64) - ref64)))
        assert wide < 0.01 * rms_of(ref64), f"{what}: the float32 restatement is {wide / 4:.2e} off float64, rms {rms_of(ref64):.2e}: change the inputs"
        print(f"\n[bound widened from the restatement's own float32 error] {what}: 4 x {wide / 4:.2e} = {100 * wide / rms_of(ref64):.3f} % of the rms")
        bound = np.maximum(bound, wide)
    return bound


def select_heads(p, n_random=4, seed=0, limit=None):
    """(batch, head) slices to compare with float64: the first, the last, every head of a batch row with padding, one per residue of
    bh % 8 (the XCD lane of map_block) and a few random ones -- all of them when there are few."""
    BH = p["B"] * p["H"]
    if BH <= 16:
        return np.arange(BH)
    rng = np.random.default_rng(seed)
    sel = {0, BH - 1}
    if p["kv"] is not None:
        for b in np.nonzero((p["kv"] == 0).any(1))[0]:
            sel.update(range(b * p["H"], (b + 1) * p["H"]))
    for r in range(8):
        sel.add(int(rng.choice(np.arange(r, BH, 8))))
    sel.update(int(i) for i in rng.choice(BH, n_random, replace=False))
    sel = np.array(sorted(sel))
    assert len(sel) >= 16
    return sel if limit is None else sel[:limit]


def reference(p, sel, causal, dtype, drop=None, dense=None, backward=True, dO=None):
    """attention_ref.attention on the selected (batch, head) slices, eight at a time; LSE as ONE tensor [n, Tq]: max + log2 sum, and
    log2 sum alone on fully masked rows (`full`), whose max is compared exactly."""
    B, H, Tq, Tk, dh = p["B"], p["H"], p["Tq"], p["Tk"], p["dh"]
    qh, kh, vh, gh = (heads(a, H).reshape(B * H, -1, dh) for a in (p["q"], p["k"], p["v"], p["dO"] if dO is None else dO))
    res = {k: [] for k in ("O", "mx", "ls", "dQ", "dK", "dV")}
    for i in range(0, len(sel), 8):
        s = sel[i:i + 8]
        r = attention(qh[s], kh[s], vh[s], None if p["kv"] is None else p["kv"][s // H], causal, p["scale"], gh[s] if backward else None, dtype,
                      drop=None if drop is None else drop.reshape(B * H, Tq, Tk)[s], dense=None if dense is None else dense[s // H])
        for k, a in zip(res, r):
            res[k].append(a)
    ref = {k: np.concatenate(a) for k, a in res.items() if a[0] is not None}
    ref["full"] = ref["mx"].astype(np.float64) == MASKED * LOG2E if dtype is np.float64 else None
    return ref


def lse_tensor(mx, ls, full):
    return np.where(full, np.asarray(ls, np.float64), np.asarray(mx, np.float64) + np.asarray(ls, np.float64))


def compare(out, p, sel, causal, drop=None, dense=None, tag="", backward=True, dO=None):
    """The selected heads of `out` against float64.  Returns {tensor: dict(kernel, ref32: shares of the project bound, over: worst
    error / bound_for ratio)}, prints the shares; the caller asserts with require()."""
    B, H, Tq, Tk, dh = p["B"], p["H"], p["Tq"], p["Tk"], p["dh"]
    r64 = reference(p, sel, causal, np.float64, drop, dense, backward, dO)
    r32 = reference(p, sel, causal, np.float32, drop, dense, backward, dO)
    full = r64["full"]
    lse = out["LSE"].reshape(B * H, Tq, 2)[sel]
    assert np.all(lse[..., 0][full] == MASKED2), f"{tag}: the max of a fully masked row must be exactly -1e9 log2(e) in float32"
    got = {"O": heads(out["O"], H).reshape(B * H, Tq, dh)[sel], "LSE": lse_tensor(lse[..., 0], lse[..., 1], full)}
    want = {"O": (r64["O"], r32["O"]), "LSE": (lse_tensor(r64["mx"], r64["ls"], full), lse_tensor(r32["mx"], r32["ls"], full))}
    zero = {}
    if backward:
        for n, T in (("dQ", Tq), ("dK", Tk), ("dV", Tk)):
            got[n] = heads(out[n], H).reshape(B * H, T, dh)[sel]
            want[n] = (r64[n], r32[n])
        if Tk == 1:
            # one key: P = 1 whatever the scores are, so dQ and dK are identically zero and the kernels hold the rounding of
            # dS = P (dP - Dsum) / scale with dP = Dsum = dO . v.  Their natural magnitude (assert_close_scaled's `scale` for tensors
            # that are mathematically zero): the terms that cancel, |dP| + |Dsum| = 2 |dO . v|, through the same two products.
            assert not r64["dQ"].any() and not r64["dK"].any()
            sel_h = lambda a: heads(a, H).reshape(B * H, -1, dh)[sel].astype(np.float64)      # noqa: E731
            a = 2.0 * np.abs(np.matmul(sel_h(p["dO"] if dO is None else dO), np.swapaxes(sel_h(p["v"]), -1, -2))) / p["scale"]
            zero = {"dQ": rms_of(np.matmul(a, np.abs(sel_h(p["k"])))), "dK": rms_of(np.matmul(np.swapaxes(a, -1, -2), np.abs(sel_h(p["q"]))))}
    res = {}
    for n, g in got.items():
        w64, w32 = want[n]
        assert g.shape == w64.shape, (n, g.shape, w64.shape)
        z = zero.get(n, 0.0)
        bound = bound_for(w64, w32, f"{tag}: {n}", z)
        err = np.abs(np.asarray(g, np.float64) - w64)
        over = float(np.max(np.where(np.isfinite(err), err, np.inf) / bound))
        res[n] = dict(kernel=share(g, w64, z), ref32=share(w32, w64, z), over=over)
    print(f"\n[share of the 1e-4 bound, kernel (float32 restatement)] {tag}: " +
          "  ".join(f"{n} {100 * r['kernel']:.1f} % ({100 * r['ref32']:.1f} %)" for n, r in res.items()) + f"  [{len(sel)} heads]")
    return res


def require(res, tag):
    bad = {n: r for n, r in res.items() if not r["over"] <= 1.0}
    assert not bad, f"{tag}: outside the bound of float64: " + ", ".join(f"{n} at {r['over']:.2f} x the bound" for n, r in bad.items())


# --------------------------------------------------------------------------------------------------------- the child's case list
CHILD_T = (1, 65, 127, 128, 129, 192, 257, 320, 385, 700)
BH_SHAPES = ((1, 1), (3, 2), (3, 3))                          # B*H = 1, 6, 9: padding blocks of map_block, and a second round of 8


def child_cases():
    """(name, problem arguments, call arguments).  Every T x head dim, causal and not, with B*H rotating through 1, 6, 9 (so that every
    T meets every B*H at some head dim); rectangular shapes; the three ways into the GEN kernels.  With B = 3 the batch rows carry
    trailing padding, holes and leading padding; B = 1 takes them in turn."""
    cases = []
    one = ("trailing", "holes", "leading")
    for it, T in enumerate(CHILD_T):
        for idh, dh in enumerate((32, 64, 128)):
            B, H = BH_SHAPES[(it + idh) % 3]
            for causal in (True, False):
                pads = (one[(it + idh + causal) % 3],) if B == 1 else one
                cases.append((f"T{T} dh{dh} B{B}H{H} {'causal' if causal else 'full'}", dict(B=B, H=H, Tq=T, Tk=T, dh=dh, pads=pads),
                              dict(causal=causal)))
    for idh, dh in enumerate((32, 64, 128)):
        B, H = BH_SHAPES[(idh + 1) % 3]
        for Tq, Tk in ((100, 257), (257, 100), (192, 320)):
            for causal in (True, False):
                cases.append((f"Tq{Tq} Tk{Tk} dh{dh} B{B}H{H} {'causal' if causal else 'full'}",
                              dict(B=B, H=H, Tq=Tq, Tk=Tk, dh=dh, pads=one if B > 1 else ("holes",)), dict(causal=causal)))
    for dh, T in ((64, 192), (64, 257), (32, 257), (128, 320)):
        for gen in ("dense", "injected", "hash"):
            cases.append((f"T{T} dh{dh} B3H2 GEN {gen}", dict(B=3, H=2, Tq=T, Tk=T, dh=dh, pads=one), dict(causal=True, gen=gen)))
    cases.append(("T256 dh64 B3H3 causal mul3 (attention_sb unless switched off)", dict(B=3, H=3, Tq=256, Tk=256, dh=64, pads=one, mul=3.0),
                  dict(causal=True)))
    return cases


def run_case(idx, name, pargs, cargs):
    p = make_problem(7000 + idx, **pargs)
    gen = cargs.get("gen")
    kw, ref_kw = {}, {}
    if gen == "dense":
        ref_kw["dense"] = kw["dense"] = random_dense(idx, p)
    elif gen == "injected":
        ref_kw["drop"] = kw["drop"] = injected_dropout(idx, p)
    elif gen == "hash":
        kw.update(dropout_p=0.1, seed=1234 + idx)
        ref_kw["drop"] = hash_dropout(p, 0.1, 1234 + idx)
        keep = float(np.mean(ref_kw["drop"] != 0))
        kept = np.unique(ref_kw["drop"][ref_kw["drop"] != 0])
        assert 0.85 < keep < 0.95 and len(kept) == 1 and abs(float(kept[0]) - 1.0 / 0.9) < 1e-6, (keep, kept)
    out = run(p, cargs["causal"], **kw)
    res = compare(out, p, np.arange(p["B"] * p["H"]), cargs["causal"], tag=name, **ref_kw)
    return dict(name=name, dh=p["dh"], gen=bool(gen), passes=["forward", "dQ", "dKdV"], O=digest(out["O"]), LSE=digest(out["LSE"]),
                shares={n: round(r["kernel"], 5) for n, r in res.items()}, ref32={n: round(r["ref32"], 5) for n, r in res.items()},
                over=max(r["over"] for r in res.values()))


def main():
    import torch
    import neunet_hip
    neunet_hip.load_library()
    assert torch.cuda.is_available()
    real_stdout = sys.stdout
    sys.stdout = sys.stderr                                     # the per-case share lines go to stderr: stdout carries the JSON alone
    done = [run_case(i, *c) for i, c in enumerate(child_cases())]
    sys.stdout = real_stdout
    print(json.dumps(dict(pair=os.environ.get("NNHIP_ATTN_PAIR", ""), waves=os.environ.get("NNHIP_ATTN_WAVES", ""), cases=done)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
