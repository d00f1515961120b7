"""GPU: every kernel and dispatch branch of csrc/rowops.hip outside LayerNorm -- Softmax (six register tiers x float4 / scalar, looped,
strided), the masked attention-score Softmax (the same tiers, in place and out of place, every mask source), RMSNorm (forward, backward
with and without bias / dX_addend / X_norm) and CrossEntropy (the persistent kernel's tiers, the two-block exchange, the multi-round
loop, the separate denominator launch) -- through the C ABI (include/neunet_hip.h), against the float64 restatements of
tests/rowops_ref.py, at the widths on either side of each dispatch condition.  tests/test_hip_parity.py keeps the reference's fixtures
and the module-level cases; tests/test_gpt2_gpu.py walks LayerNorm.

Which width reaches which kernel (row_tier() in rowops.hip; restated as test_rowops_ref.row_tier / row_variant / ce_kernel, which name
every case id below):

    columns          threads per row x float4 per thread      rows per block
    <= 256           64 x 1                                   4 (a wave per row, no block barrier)
    <= 512           64 x 2                                   4
    <= 1024          64 x 4                                   4
    <= 4096          256 x 4                                  1
    <= 8192          256 x 8                                  1
    <= 16384         1024 x 4                                 1
    above            the looped kernels (no register tile)    1

Each tile exists twice: float4 accesses (`vec`) when cols % 4 == 0 and every operand is 16-byte aligned (CrossEntropy: and the row
pitch % 4 == 0), else one float per access (`scalar`), with a different element -> thread map and therefore a different summation
order.  `off1` cases start every float operand four bytes into its allocation, which forces `scalar` at a width that is a multiple of 4.
CrossEntropy sends rows * cols <= 65536 with cols <= 4096 to ce_small_kernel (covered by test_hip_parity.py), so its table holds the
smallest shapes that do not fit; `2blocks` marks the grids of two blocks, which meet through one atomic exchange, not the arrival ticket.

Every output lives in an allocation with NaN on both sides of it, and every test asserts that nothing outside the output was written.
Bounds, all the project's existing ones: Softmax forward rtol 1e-5, atol 1e-6; gradients and RMSNorm outputs 1e-4 of max(|ref|,
rms(ref)) per element (assert_close_scaled); CrossEntropy loss_rows, lse and loss rtol = atol = 1e-5; counts exact.  Each test prints
its largest error / bound ratios before it asserts (run with -s); one run's figures are in EXPERIMENTS.md 5.21."""
import numpy as np
import pytest

from rowops_ref import (cross_entropy, masked_softmax_backward, masked_softmax_forward, rmsnorm_backward, rmsnorm_forward, softmax_backward,
                        softmax_forward)
from test_hip_parity import assert_close_scaled, rms_of
from test_rowops_ref import (CE_IGNORE, CE_MULTI_ROUND, CE_SHAPES, EPS, MASK_MODES, MASKED_OFF1, MASKED_TK, MASKED_TQ_NE_TK, RMS_CASES, RMS_ROWS,
                             SOFTMAX_CASES, SOFTMAX_ROWS, SOFTMAX_STRIDED, case_id, ce_id, ce_inputs, ce_kernel, masked_inputs, rms_inputs,
                             row_variant, softmax_inputs)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN = float("nan")
PAD = 4                                # floats of NaN in front of an operand (16 bytes: the operand itself stays 16-byte aligned)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import neunet_hip
    neunet_hip.load_library()
    return neunet_hip


def call(name, *args):
    from neunet_hip._lib import call_hip_function, get_current_stream_ptr
    return call_hip_function(name, *args, get_current_stream_ptr())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


class Buf:
    """A float operand inside its own allocation: PAD NaN floats, `off` more (off = 1: the operand starts 4 bytes past a 16-byte
    boundary), the operand (`value`, or NaN when only a shape is given), and NaN to the end."""

    def __init__(self, value, off=0):
        shape = tuple(value) if isinstance(value, (tuple, list)) else np.shape(value)
        n = int(np.prod(shape))
        self.whole = torch.full((PAD + off + n + PAD + 3,), NAN, device="cuda", dtype=torch.float32)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.whole[self.lo:self.hi].view(shape)
        if not isinstance(value, (tuple, list)):
            self.t.copy_(dev(value))
        assert self.t.data_ptr() % 16 == 4 * off and self.t.is_contiguous()

    def intact(self):
        """Nothing outside the operand was written."""
        return bool(torch.isnan(self.whole[:self.lo]).all()) and bool(torch.isnan(self.whole[self.hi:]).all())

    def host(self):
        return host(self.t)


def ratio(got, ref, bound):
    """Largest |got - ref| / bound: what EXPERIMENTS.md quotes."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(np.max(err / np.maximum(np.broadcast_to(bound, err.shape), 1e-300))) if err.size else 0.0


def scaled_bound(ref, tol=1e-4):
    ref = np.asarray(ref, np.float64)
    return tol * np.maximum(np.abs(ref), rms_of(ref)) + 1e-30


def close_bound(ref, rtol, atol):
    return atol + rtol * np.abs(np.asarray(ref, np.float64))


# ===================================================================================================== Softmax
def check_softmax(tag, y, Yr, dx, dXr):
    r_y, r_dx = ratio(y, Yr, close_bound(Yr, 1e-5, 1e-6)), ratio(dx, dXr, scaled_bound(dXr))
    print(f"\n[{tag}] error / bound: Y {r_y:.3f}, dX {r_dx:.3f}")
    np.testing.assert_allclose(y, Yr, rtol=1e-5, atol=1e-6, err_msg=tag + " Y")
    assert_close_scaled(dx, dXr, err_msg=tag + " dX")


@pytest.mark.parametrize("cols,off", SOFTMAX_CASES, ids=[case_id(c, o) for c, o in SOFTMAX_CASES])
def test_softmax_tiers(hip, cols, off):
    """Forward, then backward at the kernel's own output: nine rows (three blocks of four with a ragged last one below 1025 columns)."""
    rows = SOFTMAX_ROWS
    X, dY = softmax_inputs(rows, cols, cols + off)
    x, dy, y, dx = Buf(X, off), Buf(dY, off), Buf((rows, cols), off), Buf((rows, cols), off)
    call("nnhipSoftmaxForward", y.t, x.t, rows, cols, 1)
    call("nnhipSoftmaxBackward", dx.t, dy.t, y.t, rows, cols, 1)
    assert y.intact() and dx.intact() and np.array_equal(x.host(), X) and np.array_equal(dy.host(), dY)
    Yr = softmax_forward(X)
    check_softmax(f"softmax {case_id(cols, off)}", y.host(), Yr, dx.host(), softmax_backward(Yr, dY))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("outer,n,stride", SOFTMAX_STRIDED, ids=[f"strided-slice{n}-stride{s}" for _, n, s in SOFTMAX_STRIDED])
def test_softmax_strided(hip, outer, n, stride, off):
    """stride != 1: one thread per slice; slice s = outer * stride + inner walks `n` elements `stride` apart (softmax over the middle
    axis of [outer, n, stride]).  900 slices: four blocks, the last with 132 threads at work.  n = 1: every output is 1, dX is 0."""
    X, dY = softmax_inputs(outer * n, stride, n + off)
    X, dY = X.reshape(outer, n, stride), dY.reshape(outer, n, stride)
    x, dy, y, dx = Buf(X, off), Buf(dY, off), Buf(X.shape, off), Buf(X.shape, off)
    call("nnhipSoftmaxForward", y.t, x.t, outer * stride, n, stride)
    call("nnhipSoftmaxBackward", dx.t, dy.t, y.t, outer * stride, n, stride)
    assert y.intact() and dx.intact()
    Yr = softmax_forward(X, 1)
    check_softmax(f"softmax strided n = {n}", y.host(), Yr, dx.host(), softmax_backward(Yr, dY, 1))
    if n == 1:
        assert np.all(y.host() == 1) and np.all(dx.host() == 0)


# ===================================================================================================== masked Softmax
def run_masked(c, off, tag):
    """Out of place and in place (out == in, dX == dY: the calls neunet_hip/nn/experimental/attention.py makes), bit-identical;
    against float64; the inputs of the out-of-place calls unchanged."""
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    kv = None if c["key_valid"] is None else dev(c["key_valid"], np.int32)
    dm = None if c["dense"] is None else dev(c["dense"], np.int32)
    geo = (B, H, Tq, Tk, c["scale"], int(c["causal"]))
    s, y = Buf(c["S"], off), Buf(c["S"].shape, off)
    call("nnhipMaskedSoftmaxForwardEx", y.t, s.t, kv, dm, *geo)
    s2 = Buf(c["S"], off)
    call("nnhipMaskedSoftmaxForwardEx", s2.t, s2.t, kv, dm, *geo)
    assert y.intact() and s2.intact() and np.array_equal(s.host(), c["S"])
    assert torch.equal(s2.t, y.t), tag + ": in place differs from out of place (forward)"
    dy, dx = Buf(c["dY"], off), Buf(c["S"].shape, off)
    call("nnhipMaskedSoftmaxBackwardEx", dx.t, dy.t, y.t, kv, dm, *geo)
    dy2 = Buf(c["dY"], off)
    call("nnhipMaskedSoftmaxBackwardEx", dy2.t, dy2.t, y.t, kv, dm, *geo)
    assert dx.intact() and dy2.intact() and np.array_equal(dy.host(), c["dY"])
    assert torch.equal(dy2.t, dx.t), tag + ": in place differs from out of place (backward)"
    Yr = masked_softmax_forward(c["S"], c["key_valid"], c["dense"], c["scale"], c["causal"])
    dXr = masked_softmax_backward(Yr, c["dY"], c["key_valid"], c["dense"], c["scale"], c["causal"])
    check_softmax(tag, y.host(), Yr, dx.host(), dXr)
    assert np.all(dx.host()[dXr == 0] == 0), tag + ": a masked position received a gradient"


@pytest.mark.parametrize("mode", MASK_MODES)
@pytest.mark.parametrize("Tk", MASKED_TK, ids=[case_id(t) for t in MASKED_TK])
def test_masked_softmax_tiers(hip, Tk, mode):
    """B = 2, H = 3, Tq = 5: 30 rows.  Row r is (b, h, i) = (r / 15, (r / 5) % 3, r % 5): with H > 1 a kernel that took i = r % (H Tq)
    or b = r / Tq would read another row of the dense mask or another batch's key_valid."""
    run_masked(masked_inputs(Tk, mode), 0, f"masked softmax {case_id(Tk)} {mode}")


@pytest.mark.parametrize("Tq,Tk", MASKED_TQ_NE_TK, ids=[f"Tq{q}-Tk{k}-{row_variant(k)}" for q, k in MASKED_TQ_NE_TK])
def test_masked_softmax_causal_tq_ne_tk(hip, Tq, Tk):
    """The causal limit is j > i + (Tk - Tq).  Tq = 9 > Tk = 7: queries 0 and 1 see no key at all (uniform rows, zero gradient)."""
    for mode in ("causal", "all"):
        run_masked(masked_inputs(Tk, mode, Tq), 0, f"masked softmax Tq {Tq} Tk {Tk} {mode}")


@pytest.mark.parametrize("Tk", MASKED_OFF1, ids=[case_id(t, 1) for t in MASKED_OFF1])
def test_masked_softmax_offset_operands(hip, Tk):
    """Every float operand four bytes into its allocation: the scalar variant at a width that is a multiple of 4, one per block size."""
    run_masked(masked_inputs(Tk, "all"), 1, f"masked softmax {case_id(Tk, 1)} all")


# ===================================================================================================== RMSNorm
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("cols,off", RMS_CASES, ids=[case_id(c, o) for c, o in RMS_CASES])
def test_rmsnorm_tiers(hip, cols, off, bias):
    """nnhipRMSNormForward with X_norm NULL and non-NULL (the same Y and X_std bits), nnhipRMSNormBackwardEx with and without
    dX_addend, at the kernel's own X_std.  Nine rows: the backward's persistent grid holds three blocks of four row slots below 1025
    columns (the last with one), nine one-row blocks above."""
    rows = RMS_ROWS
    X, w, b, dY, addend = rms_inputs(rows, cols, cols + off + 2 * bias)
    x, wd, dy, ad = Buf(X, off), Buf(w, off), Buf(dY, off), Buf(addend, off)
    bd = Buf(b, off) if bias else None
    Yr, Xnr, stdr = rmsnorm_forward(X, w, b if bias else None, EPS)
    tag = f"rmsnorm {case_id(cols, off)} {'bias' if bias else 'nobias'}"
    kept = None
    for want_norm in (False, True):
        y, std = Buf((rows, cols), off), Buf((rows,), off)
        xn = Buf((rows, cols), off) if want_norm else None
        call("nnhipRMSNormForward", x.t, wd.t, bd.t if bias else None, y.t, std.t, xn.t if want_norm else None, rows, cols, EPS)
        assert y.intact() and std.intact() and (xn is None or xn.intact())
        if kept is None:
            kept = (y, std)
        else:
            assert torch.equal(y.t, kept[0].t) and torch.equal(std.t, kept[1].t), tag + ": X_norm changed Y or X_std"
            r = ratio(xn.host(), Xnr, scaled_bound(Xnr))
            print(f"\n[{tag}] error / bound: X_norm {r:.3f}")
            assert_close_scaled(xn.host(), Xnr, err_msg=tag + " X_norm")
    y, std = kept
    print(f"[{tag}] error / bound: Y {ratio(y.host(), Yr, scaled_bound(Yr)):.3f}, X_std {ratio(std.host(), stdr, scaled_bound(stdr)):.3f}")
    assert_close_scaled(y.host(), Yr, err_msg=tag + " Y")
    assert_close_scaled(std.host(), stdr, err_msg=tag + " X_std")
    for with_addend in (False, True):
        dx, dw = Buf((rows, cols), off), Buf((cols,), off)
        db = Buf((cols,), off) if bias else None
        call("nnhipRMSNormBackwardEx", dy.t, x.t, wd.t, std.t, None, ad.t if with_addend else None, dx.t, dw.t, db.t if bias else None, rows, cols)
        assert dx.intact() and dw.intact() and (db is None or db.intact())
        dXr, dwr, dbr = rmsnorm_backward(X, w, dY, EPS, addend if with_addend else None)
        shares = dict(dX=ratio(dx.host(), dXr, scaled_bound(dXr)), dW=ratio(dw.host(), dwr, scaled_bound(dwr)))
        if bias:
            shares["db"] = ratio(db.host(), dbr, scaled_bound(dbr))
        print(f"[{tag}{' + addend' if with_addend else ''}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
        assert_close_scaled(dx.host(), dXr, err_msg=tag + " dX")
        assert_close_scaled(dw.host(), dwr, err_msg=tag + " dW")
        if bias:
            assert_close_scaled(db.host(), dbr, err_msg=tag + " db")
    assert np.array_equal(x.host(), X) and np.array_equal(dy.host(), dY) and np.array_equal(ad.host(), addend)


# ===================================================================================================== CrossEntropy
RED = {"n": "none", "m": "mean", "s": "sum"}
LABEL_TYPES = {2: np.int16, 4: np.int32, 8: np.int64}
SENTINEL = -7


class CeRun:
    """One nnhipCrossEntropyLossEx call.  logits [rows, ld] with NaN in the pad columns ld - cols; dlogits NULL (in place) or a second
    buffer of the same pitch; loss_rows, lse, loss_out in NaN-fenced buffers; count_out between two sentinels; the labels as int16 /
    int32 / int64, optionally one element into their buffer (`label_off`: a 4-byte-aligned int32 vector, count_labels' scalar path)."""

    def __init__(self, logits, labels, weight, red, lbytes=4, ld=None, inplace=False, off=0, label_off=0, calls=1):
        rows, cols = logits.shape
        ld = cols if ld is None else ld
        padded = np.full((rows, ld), np.nan, np.float32)
        padded[:, :cols] = logits
        self.x = Buf(padded, off)
        self.dl = None if inplace else Buf((rows, ld), off)
        self.loss_rows, self.lse, self.loss = Buf((rows,), off), Buf((rows,), off), Buf((1,), off)
        self.count = torch.full((3,), SENTINEL, device="cuda", dtype=torch.int32)
        lab = torch.zeros(rows + label_off, device="cuda", dtype={2: torch.int16, 4: torch.int32, 8: torch.int64}[lbytes])
        lab[label_off:] = dev(labels, LABEL_TYPES[lbytes])
        lab = lab[label_off:]
        assert lab.data_ptr() % 16 == (lbytes * label_off) % 16
        wd = None if weight is None else Buf(weight, off)
        for i in range(calls):
            if i:
                self.x.t.copy_(dev(padded))                   # (an in-place call overwrote them)
            call("nnhipCrossEntropyLossEx", self.x.t, None if inplace else self.dl.t, self.loss_rows.t, self.lse.t, lab, lbytes,
                 None if wd is None else wd.t, ld, CE_IGNORE, rows, cols, red.encode(), self.loss.t, self.count[1:2])
        out = self.x if inplace else self.dl
        full = out.host()
        self.dlogits, self.pad = full[:, :cols], full[:, cols:]
        self.red, self.cols = red, cols
        self.fenced = all(b.intact() for b in (self.x, self.loss_rows, self.lse, self.loss) + (() if inplace else (self.dl,)))
        self.logits_kept = inplace or np.array_equal(self.x.host()[:, :cols], logits)

    def bits(self):
        return [self.dlogits, self.loss_rows.host(), self.lse.host(), self.loss.host(), host(self.count)]

    def check(self, tag, ref):
        """Against rowops_ref.cross_entropy's (loss_rows, lse, loss, dlogits, count)."""
        loss_rows, lse, loss, dlogits, count = ref
        assert self.fenced, tag + ": wrote outside an output"
        assert self.logits_kept, tag + ": an out-of-place call changed the logits"
        assert np.all(np.isnan(self.pad)), tag + ": the pad columns were written"
        cnt = host(self.count)
        assert cnt[0] == SENTINEL and cnt[2] == SENTINEL
        shares = dict(loss_rows=ratio(self.loss_rows.host(), loss_rows, close_bound(loss_rows, 1e-5, 1e-5)),
                      lse=ratio(self.lse.host(), lse, close_bound(lse, 1e-5, 1e-5)), dlogits=ratio(self.dlogits, dlogits, scaled_bound(dlogits)))
        if self.red != "n":
            shares["loss"] = ratio(self.loss.host()[0], loss, close_bound(loss, 1e-5, 1e-5))
        print(f"\n[{tag}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
        np.testing.assert_allclose(self.loss_rows.host(), loss_rows, rtol=1e-5, atol=1e-5, err_msg=tag + " loss_rows")
        np.testing.assert_allclose(self.lse.host(), lse, rtol=1e-5, atol=1e-5, err_msg=tag + " lse")
        assert_close_scaled(self.dlogits, dlogits, err_msg=tag + " dlogits")
        if self.red == "n":
            assert np.isnan(self.loss.host()[0]), tag + ": 'n' wrote loss_out"
        else:
            np.testing.assert_allclose(self.loss.host()[0], loss, rtol=1e-5, atol=1e-5, err_msg=tag + " loss")
        if self.red == "m":
            assert cnt[1] == count, tag + f": count_out {cnt[1]} != {count}"           # ('m' is the reduction that documents a count)
        inert = np.all(dlogits == 0, axis=1)
        assert np.all(self.dlogits[inert] == 0) and np.all(self.loss_rows.host()[inert] == 0), tag + ": an inert row is not zero"


def same_bits(a, b, what):
    for u, v, name in zip(a.bits(), b.bits(), ("dlogits", "loss_rows", "lse", "loss", "count")):
        assert np.array_equal(u, v, equal_nan=True), f"{what}: {name} differs"


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("red", ["n", "m", "s"])
@pytest.mark.parametrize("shape", CE_SHAPES, ids=[ce_id(s) for s in CE_SHAPES])
def test_cross_entropy_tiers(hip, shape, red, weighted):
    """Every register tier of ce_rows_kernel in both variants and ce_looped_kernel, every reduction, with and without class weights;
    ignore_index 0 on every fifth row, one label == C and one negative label that is not ignore_index."""
    logits, labels, weight = ce_inputs(*shape)
    w = weight if weighted else None
    run = CeRun(logits, labels, w, red)
    run.check(f"ce {ce_id(shape)} {red} {'weighted' if weighted else 'plain'}", cross_entropy(logits, labels, w, CE_IGNORE, RED[red]))


@pytest.mark.parametrize("shape", CE_SHAPES, ids=[ce_id(s) for s in CE_SHAPES])
def test_cross_entropy_call_variants(hip, shape):
    """Around the plain 'm' call of each shape: in place (dlogits NULL), a padded row pitch, the three label types, a label vector that
    is not 16-byte aligned, and the same call twice (the kernel resets its own sync words).  The same arithmetic gives the same bits;
    where the kernel variant changes (pitch cols + 1 takes the scalar tile at any width) the results are held to the bounds."""
    rows, cols = shape
    logits, labels, weight = ce_inputs(*shape)
    ref = cross_entropy(logits, labels, None, CE_IGNORE, "mean")
    base = CeRun(logits, labels, None, "m")
    base.check(f"ce {ce_id(shape)} base", ref)
    same_bits(CeRun(logits, labels, None, "m", inplace=True), base, "in place")
    same_bits(CeRun(logits, labels, None, "m", calls=2), base, "called twice")
    same_bits(CeRun(logits, labels, None, "m", inplace=True, calls=2), base, "in place, called twice")
    for lbytes in (2, 8):
        same_bits(CeRun(logits, labels, None, "m", lbytes=lbytes), base, f"int{8 * lbytes} labels")
    same_bits(CeRun(logits, labels, None, "m", label_off=1), base, "int32 labels, 4-byte aligned")
    for ld in (cols + 4, cols + 1):
        for inplace in (False, True):
            run = CeRun(logits, labels, None, "m", ld=ld, inplace=inplace)
            tag = f"ce {rows}x{cols} pitch {ld} ({ce_kernel(rows, cols, ld)}){' in place' if inplace else ''}"
            run.check(tag, ref)
            if ce_kernel(rows, cols, ld) == ce_kernel(rows, cols):
                same_bits(run, base, tag)
    # class weights: the denominator is a float sum whose order depends on the label path (int4 loads / one label per load), so the
    # label types agree to the bounds, not to the bit
    refw = cross_entropy(logits, labels, weight, CE_IGNORE, "mean")
    for lbytes, label_off in ((2, 0), (4, 0), (4, 1), (8, 0)):
        CeRun(logits, labels, weight, "m", lbytes=lbytes, label_off=label_off, inplace=True).check(
            f"ce {rows}x{cols} weighted int{8 * lbytes}{' + 4 bytes' if label_off else ''}", refw)


def test_cross_entropy_offset_operands(hip):
    """Every float operand four bytes into its allocation: the scalar tile at widths that are multiples of 4."""
    for shape in ((66, 1024), (17, 4096), (2, 16384)):
        logits, labels, weight = ce_inputs(*shape)
        CeRun(logits, labels, weight, "m", off=1).check(f"ce {shape[0]}x{shape[1]} off1 ({ce_kernel(*shape, off=1)})",
                                                         cross_entropy(logits, labels, weight, CE_IGNORE, "mean"))


@pytest.mark.parametrize("shape", CE_MULTI_ROUND, ids=[ce_id(s) for s in CE_MULTI_ROUND])
def test_cross_entropy_multi_round(hip, shape):
    """'m' derives its denominator from the labels in every block, so ce_launch() caps the grid at 1024 blocks: 12293 rows of <= 1024
    columns are three rounds of 4096 rows and one of five -- the prefetch of the row after next runs, and ends raggedly (block 0 has
    four rounds, block 2 three); 2053 rows of 4100 columns are two rounds and five rows of the tier that does not prefetch."""
    logits, labels, _ = ce_inputs(*shape)
    ref = cross_entropy(logits, labels, None, CE_IGNORE, "mean")
    run = CeRun(logits, labels, None, "m")
    run.check(f"ce {ce_id(shape)} multi-round", ref)
    same_bits(CeRun(logits, labels, None, "m", inplace=True), run, "in place")


def test_cross_entropy_separate_denominator_launch(hip):
    """int64 labels at 12293 rows: 1024 blocks x 12293 x 8 B is over the 64 MB a per-block count may re-read, so the denominator comes
    from ce_denominator_kernel and the grid is not capped.  Same numbers as the int32 run (a different grid: to the bounds), and the
    count is written by the denominator launch."""
    shape = (12293, 260)
    logits, labels, weight = ce_inputs(*shape)
    for w in (None, weight):
        ref = cross_entropy(logits, labels, w, CE_IGNORE, "mean")
        wide, narrow = CeRun(logits, labels, w, "m", lbytes=8), CeRun(logits, labels, w, "m", lbytes=4)
        wide.check("ce 12293x260 int64 (separate denominator)", ref)
        narrow.check("ce 12293x260 int32 (counted in the kernel)", ref)
        np.testing.assert_allclose(wide.loss.host(), narrow.loss.host(), rtol=1e-5, atol=1e-5)
        assert host(wide.count)[1] == host(narrow.count)[1] == ref[4]
        assert np.array_equal(wide.lse.host(), narrow.lse.host())            # a row's lse does not depend on the grid


def test_cross_entropy_more_blocks_than_slots(hip):
    """'s' at 20000 x 130: 5000 blocks of four rows, more than any device holds at once (256 compute units x 8 blocks), so the
    persistent loop runs at least two rounds whatever the occupancy."""
    shape = (20000, 130)
    logits, labels, weight = ce_inputs(*shape)
    for w in (None, weight):
        CeRun(logits, labels, w, "s").check("ce 20000x130 s", cross_entropy(logits, labels, w, CE_IGNORE, "sum"))
