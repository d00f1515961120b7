"""Every dispatch tier of the fused attention kernels (csrc/attention.hip) through the C ABI, each output in a NaN-filled, NaN-fenced
buffer, every element compared with the float64 restatement (tests/attention_ref.py, pinned to the oracle by
tests/test_attention_ref.py); the entries' ABI edges on a device; properties that need no reference.  tests/attention_child.py holds
the problems, the call and the comparison, and is the fresh process for the switches the library reads once.

Dispatch (nnhipAttentionForwardEx / nnhipAttentionBackwardEx; add a row whenever a tier is added):

    head_dim  GEN  NW  pair  sb   bq   kernels                                         taken when
    64        no   -   -     yes  -    attention_sb.hip (balanced T = 256)             causal, no GEN, Tq = Tk = 256
    64        no   2   0/1   no   64   attn_fwd / attn_bwd_dq / attn_bwd_dkdv <64,0,2> default at head dim 64
    64        yes  2   0/1   no   64   the same <64,1,2>                               dense mask, injected or hash dropout
    64        no   4   0/1   no   128  <64,0,4>                                        NNHIP_ATTN_WAVES=4
    64        yes  4   0/1   no   128  <64,1,4>                                        NNHIP_ATTN_WAVES=4 with GEN
    32        any  4   0/1   no   128  <32,GEN,4>                                      always
    128       any  4   0/1   no   128  <128,GEN,4>                                     always

    GEN: opts names a dense mask, a dropout mask or dropout_p > 0.  bq: query rows per forward / dQ block, keys per dK/dV block.
    pair (forward only): nblk = ceil(Tq / bq); on iff causal (a dense mask clears causal) and 2 <= nblk <= 8 and
    B*H*ceil(nblk/2) >= 512 and the call is not sb's; NNHIP_ATTN_PAIR=0: never, =1: whenever nblk >= 2.  In pair mode a block runs query
    block nblk-1-k and then k (the middle one alone when nblk is odd) through the same LDS.

Bound: assert_close_scaled's 1e-4 of max(|ref|, rms(ref)) per element of O, LSE (max exactly on fully masked rows, max + log2 sum
otherwise), dQ, dK, dV against float64; attention_child.bound_for widens it only from the two restatements (never reached here: the
float32 restatement stays below a quarter of the bound on these inputs).  Every case prints its shares before it asserts (-s).

Worst share of the bound per group, in per cent: the float32 restatement (measured on the CPU; what the reference's own rounding
costs) and the kernels.  STATUS: the kernel column is EMPTY -- no MI355X run of this module has been recorded yet; the first run fills
it from the lines every case prints (pytest -s) and adds the module's run time and slowest items here.

    group                                    float32 restatement  O / LSE / dQ / dK / dV      kernels
    pair 1 (dh 64, BH 512, T 128)                                 1.9 / 0.1 / 2.4 / 2.9 / 1.8     -
    pair 2 (BH 256, T 192 [B,T,3D] and T 180)                     2.6 / 0.1 / 2.5 / 3.3 / 4.2     -
    pair 3 (BH 128, T 512 and T 513)                              3.2 / 0.1 / 3.3 / 6.2 / 4.8     -
    pair 4 (BH 512, Tq 128 x Tk 200)                              1.8 / 0.1 / 2.3 / 5.2 / 4.5     -
    pair 5 (BH 256, T 256, injected and hash dropout)             2.4 / 0.1 / 2.8 / 4.7 / 4.1     -
    pair 6 (dh 32, BH 512, T 200)                                 1.5 / 0.1 / 2.0 / 3.2 / 2.0     -
    pair 6 (dh 128, BH 256, T 300)                                3.9 / 0.1 / 4.6 / 5.3 / 3.9     -
    threshold (BH 511 and 512, T 128)                             2.0 / 0.1 / 2.9 / 2.9 / 2.0     -
    long: T 1100 causal, first valid key 70 (dh 32, 64, 128)      4.5 / 0.1 / 4.8 / 6.9 / 5.4     -
    long: T 2048 non-causal                                       3.5 / 0.1 / 4.3 / 4.6 / 4.3     -
    long: Tq 1 x Tk 1500                                          1.0 / 0.0 / 0.7 / 1.3 / 0.6     -
    long: Tq 1500 x Tk 1, causal and not                          0.0 / 0.5 / 0.0 / 0.0 / 0.6     -
    the 91 cases of a child (any switch)                          5.9 / 0.3 / 5.8 / 12.0 / 6.9    -
    (the child's 12 % on dK is its one q, k ~ 3 N(0,1) case, see tests/test_attention_ref.py)

CPU cost, measured: the float64 + float32 restatements of all in-process cases take 15 s together (T 513 on 35 heads 4 s, the
others under 3 s each); a child's 91 cases take 7 s of restatement besides its start-up.

Mutants of csrc/attention.hip to hold this module against (one line each, never committed; each compiles for gfx950 and stays within
the kernels' own index ranges, read in the source).  STATUS: none has been RUN yet; the test named is the one written to catch it:
    1. attn_pair(): `*Tgrid = (nblk / 2) * bq` (the unpaired middle block is never launched): test_pair_odd_block_count (NaN rows of
       the fenced O), test_pair_other_head_dims[128], the odd block counts of the NNHIP_ATTN_PAIR=1 child.
       (`nmap = qblocks / 2` in attn_fwd_kernel is not a mutant on its own: the host still launches ceil(nblk / 2) block columns and
       the extra column maps to kpair = the middle block.)
    2. `qb_second = kpair + 1`: every test_pair_* that pairs (bit-identity and NaN rows), test_forced_pair_is_bit_identical_to_unpaired.
    3. `shift` dropped from skip_ok / last_key of attn_fwd_kernel: test_pair_causal_shift and the rectangular cases of every child.
    4. `skip_ok = !dense && p.causal` (fv ignored: fully masked rows no longer uniform over all keys): test_pair_smallest_default_on_
       shape, test_pair_causal_shift, test_long_sequence[T1100 causal], the leading-padding rows of every child.
    5. `q0 = qb * BQ + wave * (NW == 4 ? 16 : 32)`: test_forced_switch_within_bound[waves4] at head dim 64 only.
    6. `alpha = t > 8 ? 1 : exp2(m - m_new)`: test_long_sequence[T1100 causal, T2048 full, Tq1 Tk1500], T 700 of every child."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_child as C
from lstm_abi import Fenced, dev

pytestmark = pytest.mark.gpu

EINVAL, EALIGN = -1, -2


@pytest.fixture(scope="module", autouse=True)
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    assert os.environ.get("NNHIP_ATTN_PAIR") is None and os.environ.get("NNHIP_ATTN_WAVES", "2") == "2", \
        "this module needs the default dispatch in the parent process"
    return neunet_hip


def check(p, causal, tag, sel=None, out=None, **kw):
    """One fenced forward + backward, compared with float64 on the heads `sel` (default: all)."""
    ref_kw = {k: kw[k] for k in ("drop", "dense") if k in kw}
    out = C.run(p, causal, **kw) if out is None else out
    C.require(C.compare(out, p, np.arange(p["B"] * p["H"]) if sel is None else sel, causal, tag=tag, **ref_kw), tag)
    return out


# ------------------------------------------------------------------------------------------------ a. pair mode, natural dispatch
def sub_batched(p, causal, gen, **kw):
    """The forward of the same problem as calls of so few batch rows that B*H*pairs < 512: pairing is off in each."""
    B, H, Tq, Tk, dh = (p[k] for k in ("B", "H", "Tq", "Tk", "dh"))
    pairs = (-(-Tq // C.block_rows(dh)) + 1) // 2
    step = min(max(1, 511 // (H * pairs)), (B + 1) // 2)
    O, L = [], []
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        assert not C.pair_mode((b1 - b0) * H, Tq, Tk, dh, causal, gen)
        o = C.run(p, causal, backward=False, batch=(b0, b1), **kw)
        O.append(o["O"])
        L.append(o["LSE"])
    return np.concatenate(O), np.concatenate(L)


def pair_case(tag, seed, B, H, Tq, Tk, dh, expect_pair=True, lead=None, ld3=False, drop=None, hash_seed=None):
    p = C.make_problem(seed, B, H, Tq, Tk, dh, lead=lead)
    kw, sub_kw, ref_kw = dict(ld3=ld3), dict(ld3=ld3), {}
    if drop == "injected":
        ref_kw["drop"] = kw["drop"] = sub_kw["drop"] = C.injected_dropout(seed, p)
    elif drop == "hash":
        # the sub-batched calls cannot use the hash (its row key counts rows from the call's own batch 0): they get the multipliers
        # nnhipAttentionDropoutMask reports for the whole call, injected -- the same products P * multiplier, so the same bits
        kw.update(dropout_p=0.1, seed=hash_seed)
        ref_kw["drop"] = sub_kw["drop"] = C.hash_dropout(p, 0.1, hash_seed)
        keep = float(np.mean(ref_kw["drop"] != 0))
        kept = np.unique(ref_kw["drop"][ref_kw["drop"] != 0])
        assert 0.88 < keep < 0.92 and len(kept) == 1 and abs(float(kept[0]) - 1.0 / 0.9) < 1e-6, (keep, kept)
    gen = drop is not None
    assert C.pair_mode(B * H, Tq, Tk, dh, True, gen) == expect_pair, tag
    out = C.run(p, True, **kw)
    O, L = sub_batched(p, True, gen, **sub_kw)
    np.testing.assert_array_equal(out["O"], O, err_msg=f"{tag}: O differs from the sub-batched calls")
    np.testing.assert_array_equal(out["LSE"], L, err_msg=f"{tag}: LSE differs from the sub-batched calls")
    sel = C.select_heads(p, seed=seed)
    lse = out["LSE"].reshape(B * H, Tq, 2)[sel]
    check(p, True, tag, sel=sel, out=out, **ref_kw)
    return p, out, lse


def test_pair_smallest_default_on_shape():
    """Case 1: B 64 x H 8 at T 128, head dim 64: two query blocks, one pair per head, 512 blocks."""
    p, out, lse = pair_case("pair 1: dh 64 BH 512 T 128", 101, 64, 8, 128, 128, 64)
    assert (lse[..., 0] == C.MASKED2).any(), "the leading padding must leave fully masked rows in one item of a pair"


@pytest.mark.parametrize("T,ld3", [(192, True), (180, False)])
def test_pair_odd_block_count(T, ld3):
    """Case 2: three query blocks: the middle one has no partner; T 180 has a ragged last block; T 192 in the [B, T, 3D] layout."""
    pair_case(f"pair 2: dh 64 BH 256 T {T}{' [B,T,3D]' if ld3 else ''}", 102 + T, 32, 8, T, T, 64, ld3=ld3)


@pytest.mark.parametrize("T,on", [(512, True), (513, False)])
def test_pair_upper_limit(T, on):
    """Case 3: eight query blocks is the most that pairs; nine (T 513) is off and the grid is not rewritten."""
    pair_case(f"pair 3: dh 64 BH 128 T {T}", 103 + T, 16, 8, T, T, 64, expect_pair=on)


def test_pair_causal_shift():
    """Case 4: Tq 128 against Tk 200: shift = 72 under pairing; leading padding of 100 keys leaves the first 28 rows fully masked."""
    p, out, lse = pair_case("pair 4: dh 64 BH 512 Tq 128 Tk 200", 104, 64, 8, 128, 200, 64, lead=100)
    assert (lse[..., 0] == C.MASKED2).any()


@pytest.mark.parametrize("drop", ["injected", "hash"])
def test_pair_with_dropout(drop):
    """Case 5: GEN plus pair at T 256 (without dropout this shape is attention_sb's), injected multipliers and the hash RNG."""
    pair_case(f"pair 5: dh 64 BH 256 T 256 {drop} dropout", 105, 32, 8, 256, 256, 64, drop=drop, hash_seed=4242)


@pytest.mark.parametrize("dh,B,T", [(32, 64, 200), (128, 32, 300)])
def test_pair_other_head_dims(dh, B, T):
    """Case 6: 128-row blocks: head dim 32 with two blocks, head dim 128 with three."""
    pair_case(f"pair 6: dh {dh} BH {B * 8} T {T}", 106 + dh, B, 8, T, T, dh)


@pytest.mark.parametrize("B,H,on", [(73, 7, False), (64, 8, True)])
def test_pair_threshold(B, H, on):
    """511 heads at T 128 do not pair, 512 do; both equal the sub-batched calls bit for bit."""
    pair_case(f"pair threshold: BH {B * H} T 128", 107 + B, B, H, 128, 128, 64, expect_pair=on)


# --------------------------------------------------------------------------------------- b. forced switches, one child each
SETTINGS = {"pair1": {"NNHIP_ATTN_PAIR": "1"}, "pair0": {"NNHIP_ATTN_PAIR": "0"}, "waves4": {"NNHIP_ATTN_WAVES": "4"}}
_children = {}


def child(setting):
    """tests/attention_child.py in a fresh interpreter under `setting`, once per module run; children never overlap."""
    if setting not in _children:
        env = {k: v for k, v in os.environ.items() if k not in ("NNHIP_ATTN_PAIR", "NNHIP_ATTN_WAVES")}
        env.update(SETTINGS[setting])
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "attention_child.py")], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _children[setting] = json.loads(r.stdout.strip().splitlines()[-1])
        print(r.stderr[-200000:])
    return _children[setting]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_forced_switch_within_bound(setting):
    """Every tensor of every case of attention_child.child_cases() is within the bound of float64 under the switch."""
    res = child(setting)
    assert res["pair"] == SETTINGS[setting].get("NNHIP_ATTN_PAIR", "") and res["waves"] == SETTINGS[setting].get("NNHIP_ATTN_WAVES", "")
    assert [c["name"] for c in res["cases"]] == [c[0] for c in C.child_cases()]
    worst = {n: max(c["shares"][n] for c in res["cases"]) for n in C.TENSORS}
    print(f"\n[worst share of the 1e-4 bound over {len(res['cases'])} cases] {setting}: " + "  ".join(f"{n} {100 * v:.1f} %" for n, v in worst.items()))
    bad = [(c["name"], c["over"]) for c in res["cases"] if not c["over"] <= 1.0]
    assert not bad, f"{setting}: outside the bound of float64: {bad}"


def test_forced_pair_is_bit_identical_to_unpaired():
    """Pairing changes which block runs a query block, not its arithmetic: O and LSE digests agree case by case; and the forced
    setting did pair something the natural dispatch would not (B*H <= 9)."""
    on, off = child("pair1"), child("pair0")
    diff = [a["name"] for a, b in zip(on["cases"], off["cases"]) if (a["O"], a["LSE"]) != (b["O"], b["LSE"])]
    assert not diff, diff
    paired = [n for n, pa, ca in C.child_cases()
              if C.pair_mode(pa["B"] * pa["H"], pa["Tq"], pa["Tk"], pa["dh"], ca["causal"], bool(ca.get("gen")), forced=1)]
    assert len(paired) > 40, len(paired)


def test_four_wave_child_ran_head_dim_64():
    """NNHIP_ATTN_WAVES=4 ran head-dim-64 cases through forward, dQ and dK/dV, with and without GEN, at more than one 128-row block."""
    res = child("waves4")
    d64 = [c for c in res["cases"] if c["dh"] == 64]
    for gen in (False, True):
        ran = [c for c in d64 if c["gen"] == gen]
        assert len(ran) >= 3 and all(c["passes"] == ["forward", "dQ", "dKdV"] and set(c["shares"]) == set(C.TENSORS) for c in ran)
    assert any("T700" in c["name"] for c in d64)


# ---------------------------------------------------------------------------------------------------------- c. long sequences
LONG = {"T1100 causal": dict(Tq=1100, Tk=1100, causal=True, B=1, H=2, pads=("leading",), lead=70),
        "T2048 full": dict(Tq=2048, Tk=2048, causal=False, B=1, H=2, pads=("holes",)),
        "Tq1 Tk1500": dict(Tq=1, Tk=1500, causal=True, B=3, H=1, pads=("trailing", "holes", "leading")),
        "Tq1500 Tk1 causal": dict(Tq=1500, Tk=1, causal=True, B=1, H=2, pads=None),
        "Tq1500 Tk1 full": dict(Tq=1500, Tk=1, causal=False, B=1, H=2, pads=None)}


@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("shape", list(LONG))
def test_long_sequence(shape, dh):
    """18 and 32 key tiles (the online-softmax rescale, the first valid key beyond tile 0: key 70), one query against 24 key tiles,
    1500 queries against one key (causal: all rows but the last fully masked)."""
    s = dict(LONG[shape])
    causal = s.pop("causal")
    p = C.make_problem(300 + dh, dh=dh, **s)
    if shape == "T1100 causal":
        assert not p["kv"][0, :70].any() and p["kv"][0, 70]
    check(p, causal, f"long: {shape} dh {dh}")


# ------------------------------------------------------------------------------------------------------------ d. C ABI edges
def test_abi_ragged_and_column_blocks():
    """Ragged T (77, 50) with q, k, v as column blocks of [B, T, 3D] buffers and dQ, dK, dV each in ITS column block of a fenced
    [B, T, 3D] buffer of its own: the other two blocks of each stay NaN, the guards too, and the values are those of the contiguous
    layout bit for bit."""
    import torch
    from neunet_hip._lib import StridedView, call_hip_function, get_current_stream_ptr
    for dh, Tq, Tk in ((64, 77, 77), (32, 50, 77), (128, 77, 50)):
        p = C.make_problem(400 + dh, 2, 3, Tq, Tk, dh)
        B, H, D = 2, 3, 3 * dh
        want = C.run(p, True)
        nan = lambda T: np.full((B, T, D), np.nan, np.float32)                                 # noqa: E731
        qb = dev(np.concatenate([p["q"], nan(Tq), nan(Tq)], -1))
        kb = dev(np.concatenate([nan(Tk), p["k"], nan(Tk)], -1))
        vb = dev(np.concatenate([nan(Tk), nan(Tk), p["v"]], -1))
        kvd, gd, st = torch.from_numpy(p["kv"]).cuda(), dev(p["dO"]), get_current_stream_ptr()
        fO, fL = Fenced(B, Tq, D), Fenced(B, H, Tq, 2)
        fq, fk, fv = Fenced(B, Tq, 3 * D), Fenced(B, Tk, 3 * D), Fenced(B, Tk, 3 * D)
        col = lambda t, i: StridedView(t[..., i * D:(i + 1) * D])                              # noqa: E731
        call_hip_function("nnhipAttentionForwardEx", col(qb, 0), col(kb, 1), col(vb, 2), kvd, fO.view, fL.view, B, H, Tq, Tk, dh, 3 * D,
                          1.0 / p["scale"], 1, None, st)
        call_hip_function("nnhipAttentionBackwardEx", col(qb, 0), col(kb, 1), col(vb, 2), kvd, fO.view, gd, fL.view, col(fq.view, 0),
                          col(fk.view, 1), col(fv.view, 2), B, H, Tq, Tk, dh, 3 * D, 1.0 / p["scale"], 1, None, st)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(fO.host(), want["O"])
        np.testing.assert_array_equal(fL.host(), want["LSE"])
        for n, f, i in (("dQ", fq, 0), ("dK", fk, 1), ("dV", fv, 2)):
            got = f.host()
            np.testing.assert_array_equal(got[..., i * D:(i + 1) * D], want[n], err_msg=n)
            others = np.delete(got, np.s_[i * D:(i + 1) * D], -1)
            assert np.isnan(others).all(), f"dh {dh}: {n} wrote into another column block"
        assert all(f.guards_intact() for f in (fO, fL, fq, fk, fv))
        call_hip_function("nnhipDeviceError")


def test_abi_equivalent_calls_are_bit_identical():
    """opts = NULL, a zeroed opts and the non-Ex entries; key_valid = NULL and all-ones; ld_qkv = 0 and H * head_dim."""
    for dh, T, causal in ((64, 150, True), (128, 140, False), (64, 256, True)):            # the last one is attention_sb's shape
        p = C.make_problem(500 + dh, 2, 2, T, T, dh, pads=None)
        base = C.run(p, causal)
        ones = dict(p, kv=np.ones((2, T), np.int32))
        for what, other in (("zeroed opts", C.run(p, causal, entry="zeroed")), ("non-Ex entry", C.run(p, causal, entry="plain")),
                            ("key_valid all ones", C.run(ones, causal)), ("ld_qkv 0", C.run(p, causal, ld=0))):
            for n in C.TENSORS:
                np.testing.assert_array_equal(other[n], base[n], err_msg=f"dh {dh} T {T}: {what}: {n}")


class AbiCall:
    """Real device buffers for one small problem and the two Ex entries called with any argument replaced."""

    def __init__(self, B=2, H=2, Tq=40, Tk=40, dh=64):
        import torch
        from neunet_hip import _lib
        self.lib, self.shape = _lib, dict(B=B, H=H, Tq=Tq, Tk=Tk, dh=dh, ld=0, opts=None)
        p = C.make_problem(600, B, H, Tq, Tk, dh)
        D = H * dh
        self.keep = dict(Q=dev(p["q"]), K=dev(p["k"]), V=dev(p["v"]), kv=torch.from_numpy(p["kv"]).cuda(), dO=dev(p["dO"]))
        self.out = dict(O=Fenced(B, Tq, D), LSE=Fenced(B, H, Tq, 2), dQ=Fenced(B, Tq, D), dK=Fenced(B, Tk, D), dV=Fenced(B, Tk, D))
        self.saved = dict(O=Fenced(B, Tq, D), LSE=Fenced(B, H, Tq, 2))                       # a real forward, for the backward's calls
        self.fwd, self.bwd = _lib.load_hip_function("nnhipAttentionForwardEx"), _lib.load_hip_function("nnhipAttentionBackwardEx")
        self.st = _lib.get_current_stream_ptr()
        self.scale = 1.0 / p["scale"]
        assert self.forward(outs=self.saved) == 0
        torch.cuda.synchronize()
        self.saved_before = {n: f.host() for n, f in self.saved.items()}

    def ptr(self, name, off, outs=None):
        if off.get(name) is None and name in off:
            return None
        t = self.keep[name] if name in self.keep else (outs or self.out)[name].view
        return t.data_ptr() + off.get(name, 0)

    def forward(self, off={}, outs=None, **kw):
        s = dict(self.shape, **kw)
        return self.fwd(*[self.ptr(n, off, outs) for n in ("Q", "K", "V", "kv", "O", "LSE")], s["B"], s["H"], s["Tq"], s["Tk"], s["dh"], s["ld"],
                        self.scale, 1, None if s["opts"] is None else ctypes.byref(s["opts"]), self.st)

    def backward(self, off={}, **kw):
        s = dict(self.shape, **kw)
        args = [self.ptr(n, off) for n in ("Q", "K", "V", "kv")] + [self.ptr("O", off, self.saved), self.ptr("dO", off), self.ptr("LSE", off, self.saved)]
        args += [self.ptr(n, off) for n in ("dQ", "dK", "dV")]
        return self.bwd(*args, s["B"], s["H"], s["Tq"], s["Tk"], s["dh"], s["ld"], self.scale, 1,
                        None if s["opts"] is None else ctypes.byref(s["opts"]), self.st)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        for n, f in self.out.items():
            assert f.untouched(), f"a call that must not launch wrote to {n}"
        for n, f in self.saved.items():
            np.testing.assert_array_equal(f.host(), self.saved_before[n])
        self.lib.call_hip_function("nnhipDeviceError")


def test_abi_empty_problems():
    """B = 0 and Tq = 0 return 0 and touch nothing; so does the backward at Tk = 0."""
    a = AbiCall()
    assert a.forward(B=0) == 0 and a.forward(Tq=0) == 0
    assert a.backward(B=0) == 0 and a.backward(Tq=0) == 0 and a.backward(Tk=0) == 0
    a.untouched()


def test_abi_refusals():
    """Every argument error is refused on the host before any launch (read in attn_check, fill_extra and the head of the two
    entries): the documented status, an error string, every output still NaN, the device error word clear.  The backward looks at
    its options after it has its workspace and before its first launch."""
    a = AbiCall()
    half, p_one = a.lib.AttentionOptions(), a.lib.AttentionOptions()
    half.mask_bits = a.keep["Q"].data_ptr()
    p_one.dropout_p = 1.0
    D = 2 * 64
    cases = [("forward Tk 0", lambda: a.forward(Tk=0), EINVAL, "Tk")]
    for name, entry, names in (("forward", a.forward, ("Q", "K", "V", "O", "LSE")),
                               ("backward", a.backward, ("Q", "K", "V", "O", "dO", "LSE", "dQ", "dK", "dV"))):
        cases += [(f"{name} head dim 48", lambda e=entry: e(dh=48), EINVAL, "head_dim"),
                  (f"{name} ld_qkv < H * dh", lambda e=entry: e(ld=D - 4), EINVAL, "ld_qkv"),
                  (f"{name} ld_qkv % 4", lambda e=entry: e(ld=D + 2), EINVAL, "ld_qkv"),
                  (f"{name} mask_bits without mask_bitsT", lambda e=entry: e(opts=half), EINVAL, "mask_bitsT"),
                  (f"{name} dropout_p 1", lambda e=entry: e(opts=p_one), EINVAL, "dropout_p")]
        cases += [(f"{name} NULL {n}", lambda e=entry, n=n: e({n: None}), EINVAL, "null") for n in names]
        cases += [(f"{name} {n} + 4 bytes", lambda e=entry, n=n: e({n: 4}), EALIGN, "aligned") for n in names]
    for name, call, status, word in cases:
        rc = call()
        assert rc == status, f"{name}: status {rc}, expected {status} ({a.lib.last_error()})"
        assert word in a.lib.last_error(), f"{name}: {a.lib.last_error()!r}"
    a.untouched()


# ---------------------------------------------------------------------------------------- e. properties without a reference
@pytest.mark.parametrize("dh,T,drop", [(64, 200, False), (128, 150, True), (64, 256, False)])
def test_backward_is_linear_in_dO(dh, T, drop):
    """bwd(a dO1 + b dO2) = a bwd(dO1) + b bwd(dO2) with a = 0.5, b = -2 (exact scalings).  Each of the three runs is held to
    1e-4 of max(|g|, rms(g)) of the exact, exactly linear gradient elsewhere in this module, so the two sides differ by at most the
    sum of the three runs' bounds, the second and third scaled by |a| and |b|: that sum is the tolerance."""
    a, b = 0.5, -2.0
    p = C.make_problem(700 + dh, 2, 3, T, T, dh)
    kw = dict(drop=C.injected_dropout(7, p)) if drop else {}
    d1, d2 = p["dO"], np.random.default_rng(701).standard_normal(p["dO"].shape).astype(np.float32)
    mix = (np.float32(a) * d1 + np.float32(b) * d2).astype(np.float32)
    g0, g1, g2 = (C.run(p, True, dO=d, **kw) for d in (mix, d1, d2))
    for n in ("dQ", "dK", "dV"):
        x0, x1, x2 = (g[n].astype(np.float64) for g in (g0, g1, g2))
        tol = sum(abs(c) * C.project_bound(x) for c, x in ((1.0, x0), (a, x1), (b, x2)))
        err = np.abs(x0 - (a * x1 + b * x2)) / tol
        print(f"\n[linearity in dO] dh {dh} T {T} {n}: worst {100 * err.max():.1f} % of the summed bounds")
        assert err.max() <= 1.0, (n, float(err.max()))


@pytest.mark.parametrize("B,H,T,dh", [(64, 8, 128, 64), (5, 3, 200, 64), (5, 2, 300, 128)])
def test_batch_permutation_and_determinism(B, H, T, dh):
    """Permuting the batch entries permutes every output bit for bit (in pair mode: B 64 x H 8 at T 128, and out of it), and a
    second run of the same call gives the same bits."""
    p = C.make_problem(800 + B, B, H, T, T, dh)
    assert C.pair_mode(B * H, T, T, dh, True, False) == (B == 64)
    perm = np.random.default_rng(801).permutation(B)
    q = dict(p, **{k: np.ascontiguousarray(p[k][perm]) for k in ("q", "k", "v", "dO", "kv")})
    one, two, shuffled = C.run(p, True), C.run(p, True), C.run(q, True)
    for n in C.TENSORS:
        np.testing.assert_array_equal(two[n], one[n], err_msg=f"{n}: two runs differ")
        np.testing.assert_array_equal(shuffled[n], one[n][perm], err_msg=f"{n}: not permuted with the batch")
