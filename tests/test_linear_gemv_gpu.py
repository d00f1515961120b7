"""GPU: the weight-streaming Linear forward for 1..8 rows (csrc/linear_gemv.hip; nnhipLinearGemvForward, the nnhipSetLinearGemv
switch, neunet_hip.linear_gemv, examples/gpt2_infer.py --linear gemv).

Accuracy is asserted against float64 with assert_dot_close(c=4): 4 units of 2^-24 sum|x||w| per output.  The float32 emulation of
the kernel's summation order in tests/test_linear_gemv.py stays within 1 unit; a dropped or doubled k element costs a whole term.
Everything the header promises bit for bit (row independence, the epilogue order, reruns, the dispatch) is compared as uint32."""
import numpy as np
import pytest

from lstm_abi import Fenced, dev
from test_gpt2_gpu import hip, tiny  # noqa: F401  (fixtures: the loaded library; the reference's tiny GPT-2 with its fixtures)
from test_hip_parity import assert_close_scaled, assert_dot_close

pytestmark = pytest.mark.gpu


def call(name, *args):
    from neunet_hip._lib import call_hip_function
    return call_hip_function(name, *args)


def stream():
    from neunet_hip._lib import get_current_stream_ptr
    return get_current_stream_ptr()


def counts():
    return [int(call("nnhipGemmLaunchCount", k)) for k in range(5)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture
def switch(hip):  # noqa: F811
    """The switch is what it was when the test ends, whatever the test did to it; no device error is left behind."""
    before = hip.get_linear_gemv()
    yield hip
    hip.set_linear_gemv(before)
    call("nnhipDeviceError")


def shifted(a, shift):
    """`a` on the device, `shift` floats into a fresh allocation (torch allocations are 256-byte aligned): shift 1 = 4-byte aligned only."""
    import torch
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
    view = buf[shift:shift + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * shift
    return view


def gemv(X, W, b=None, add=None, shift=(0, 0, 0)):
    """One nnhipLinearGemvForward call on host arrays; O is a NaN-filled, NaN-fenced buffer.  shift: floats by which X, W, O are moved
    off their 16-byte alignment.  Returns the host result after checking the fences and that every element was written."""
    import torch
    rows, n_in = X.shape
    n_out = W.shape[0]
    out = Fenced(rows * n_out + 4)
    o = out.view[shift[2]:shift[2] + rows * n_out].view(rows, n_out)
    call("nnhipLinearGemvForward", shifted(X, shift[0]), shifted(W, shift[1]), None if b is None else dev(b),
         None if add is None else dev(add), o, rows, n_in, n_out, stream())
    torch.cuda.synchronize()
    assert out.guards_intact(), "the kernel wrote outside O"
    flat = out.host()
    assert np.isnan(flat[:shift[2]]).all() and np.isnan(flat[shift[2] + rows * n_out:]).all(), "the kernel wrote next to O"
    return o.cpu().numpy()


def operands(seed, rows, n_in, n_out):
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return u(rows, n_in), u(n_out, n_in), u(n_out), u(rows, n_out)


def check(got, X, W, b, add, msg):
    assert not np.isnan(got).any(), f"{msg}: an output was not written"
    plus = None
    if b is not None:
        plus = b.astype(np.float64)[None, :]
    if add is not None:
        plus = add.astype(np.float64) if plus is None else plus + add
    assert_dot_close(got, X, W.T, c=4, plus=plus, err_msg=msg)


# ------------------------------------------------------------------------------------------- 1. against float64
ROWS_AX, IN_AX, OUT_AX = (1, 2, 3, 5, 8), (1, 3, 4, 128, 255, 256, 260, 1028, 3072), (1, 7, 64, 257, 1001)


def sampled_cases():
    """45 of the 225 combinations, seeded: every value of every axis appears (9 / 5 / 9 times), and bias / addend are each present
    and absent next to every rows value."""
    rng = np.random.default_rng(214)
    r, i, o = list(ROWS_AX) * 9, list(IN_AX) * 5, list(OUT_AX) * 9
    rng.shuffle(i)
    rng.shuffle(o)
    return [(r[k], i[k], o[k], bool((k // 5) & 1), bool((k // 10) & 1)) for k in range(45)]


def test_sample_covers_every_axis_value():
    cases = sampled_cases()
    assert {c[0] for c in cases} == set(ROWS_AX) and {c[1] for c in cases} == set(IN_AX) and {c[2] for c in cases} == set(OUT_AX)
    assert {(c[3], c[4]) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("rows,n_in,n_out,with_b,with_add", sampled_cases())
def test_direct_entry_vs_float64(switch, rows, n_in, n_out, with_b, with_add):
    X, W, b, add = operands(rows * 100003 + n_in * 101 + n_out, rows, n_in, n_out)
    b, add = (b if with_b else None), (add if with_add else None)
    before = counts()
    got = gemv(X, W, b, add)
    check(got, X, W, b, add, f"rows={rows} in={n_in} out={n_out}")
    after = counts()
    assert after[4] == before[4] + 1 and after[:4] == before[:4]            # the direct entry: the kernel, once, and nothing else


# ------------------------------------------------------------------------------------------- 2. GPT-2 shapes
_gpt2_operands = {}


@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("n_in,n_out", [(768, 2304), (3072, 768), (768, 50257)])
def test_gpt2_shapes_vs_float64(switch, n_in, n_out, rows):
    if (n_in, n_out) not in _gpt2_operands:                                 # drawn once per shape, shared by both row counts, never changed
        _gpt2_operands.clear()
        _gpt2_operands[(n_in, n_out)] = operands(n_in + n_out, 8, n_in, n_out)
    X, W, b, add = _gpt2_operands[(n_in, n_out)]
    got = gemv(X[:rows], W, b, add[:rows])
    check(got, X[:rows], W, b, add[:rows], f"rows={rows} {n_in}->{n_out}")


# ------------------------------------------------------------------------------------------- 3. the scalar path
@pytest.mark.parametrize("rows", [1, 5, 8])
@pytest.mark.parametrize("n_in", [255, 1028])
def test_four_byte_aligned_operands(switch, n_in, rows):
    """X, W and O one float into 16-byte-aligned buffers.  in = 255: no W row but the first is 16-byte aligned anyway; in = 1028 (a
    multiple of 4) takes 16-byte loads only when X and W are both aligned: aligned and misaligned X (and W) must each pass."""
    n_out = 257
    X, W, b, add = operands(n_in + rows, rows, n_in, n_out)
    for shift in ((1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        got = gemv(X, W, b, add, shift=shift)
        check(got, X, W, b, add, f"rows={rows} in={n_in} shift={shift}")


# ------------------------------------------------------------------------------------------- 4. row independence
@pytest.mark.parametrize("n_in,n_out", [(128, 512), (3072, 257)])
def test_rows_do_not_see_each_other(switch, n_in, n_out):
    X, W, b, add = operands(n_in * 7 + n_out, 8, n_in, n_out)
    full = gemv(X, W, b, add)
    check(full, X, W, b, add, "8 rows")
    for r in range(8):
        one = gemv(X[r:r + 1], W, b, add[r:r + 1])
        np.testing.assert_array_equal(bits(one[0]), bits(full[r]), err_msg=f"row {r}: the 1-row call differs from the 8-row call")
    three = gemv(X[2:5], W, b, add[2:5])
    np.testing.assert_array_equal(bits(three), bits(full[2:5]), err_msg="a 3-row call differs from rows 2..4 of the 8-row call")
    # a NaN row stays in its row
    Xn = X.copy()
    Xn[5] = np.nan
    got = gemv(Xn, W, b, add)
    assert np.isnan(got[5]).all()
    keep = [r for r in range(8) if r != 5]
    np.testing.assert_array_equal(bits(got[keep]), bits(full[keep]))
    # a NaN weight stays in its column
    Wn = W.copy()
    Wn[11, 40] = np.nan
    got = gemv(X, Wn, b, add)
    assert np.isnan(got[:, 11]).all()
    cols = [n for n in range(n_out) if n != 11]
    np.testing.assert_array_equal(bits(got[:, cols]), bits(full[:, cols]))


# ------------------------------------------------------------------------------------------- 5. / 6. epilogue order, reruns
@pytest.mark.parametrize("rows,n_in,n_out", [(1, 768, 257), (8, 260, 1001), (3, 3, 7)])
def test_epilogue_is_plain_plus_addend_bit_for_bit(switch, rows, n_in, n_out):
    X, W, b, add = operands(rows + n_in + n_out, rows, n_in, n_out)
    for bias in (b, None):
        plain, with_add = gemv(X, W, bias, None), gemv(X, W, bias, add)
        np.testing.assert_array_equal(bits(plain + add), bits(with_add))    # one float32 add of the two arrays
    nobias, biased = gemv(X, W, None, None), gemv(X, W, b, None)
    np.testing.assert_array_equal(bits(nobias + b[None, :]), bits(biased))


def test_reruns_are_bit_identical(switch):
    import torch
    rows, n_in, n_out = 8, 3072, 1001
    X, W, b, add = (dev(a) for a in operands(6, rows, n_in, n_out))
    outs = []
    for _ in range(3):
        o = torch.full((rows, n_out), float("nan"), device="cuda")
        call("nnhipLinearGemvForward", X, W, b, add, o, rows, n_in, n_out, stream())
        outs.append(o.cpu().numpy())
    np.testing.assert_array_equal(bits(outs[0]), bits(outs[1]))
    np.testing.assert_array_equal(bits(outs[0]), bits(outs[2]))
    assert not np.isnan(outs[0]).any()


# ------------------------------------------------------------------------------------------- 7. dispatch
def test_switch_routes_the_module_entry(switch):
    import torch
    hip_ = switch
    n_in, n_out = 768, 2304                                                 # c_attn: a shape the dispatch rule sends to the kernel
    X9, W, b, add9 = (dev(a) for a in operands(7, 9, n_in, n_out))

    def module(rows):
        o = torch.full((rows, n_out), float("nan"), device="cuda")
        call("nnhipLinearModuleForwardEx", X9[:rows].contiguous(), W, b, add9[:rows].contiguous(), o, rows, n_in, n_out, stream())
        return o.cpu().numpy()

    def direct(rows):
        o = torch.full((rows, n_out), float("nan"), device="cuda")
        call("nnhipLinearGemvForward", X9[:rows].contiguous(), W, b, add9[:rows].contiguous(), o, rows, n_in, n_out, stream())
        return o.cpu().numpy()

    hip_.set_linear_gemv(False)
    off_before = {rows: module(rows) for rows in (1, 8, 9)}
    ref = {rows: direct(rows) for rows in (1, 8)}
    hip_.set_linear_gemv(True)
    for rows in (1, 8):
        c0 = counts()
        got = module(rows)
        c1 = counts()
        assert c1[4] == c0[4] + 1 and c1[:4] == c0[:4], (rows, c0, c1)
        np.testing.assert_array_equal(bits(got), bits(ref[rows]))
    c0 = counts()
    nine = module(9)
    c1 = counts()
    assert c1[4] == c0[4] and c1[:4] != c0[:4]                              # 9 rows: the GEMM, as ever
    np.testing.assert_array_equal(bits(nine), bits(off_before[9]))
    # the plain entry (no addend) is routed too
    c0 = counts()
    o = torch.empty((1, n_out), device="cuda")
    call("nnhipLinearModuleForward", X9[:1].contiguous(), W, b, o, 1, n_in, n_out, stream())
    assert counts()[4] == c0[4] + 1
    hip_.set_linear_gemv(False)
    c0 = counts()
    for rows in (1, 8):
        np.testing.assert_array_equal(bits(module(rows)), bits(off_before[rows]))
    assert counts()[4] == c0[4]


# ------------------------------------------------------------------------------------------- 8. nn.Linear
@pytest.mark.parametrize("shape", [(1, 128), (8, 128), (2, 3, 128)])
def test_nn_linear_under_the_switch(switch, shape):
    import neunet_hip.nn as nn
    hip_ = switch
    rng = np.random.default_rng(sum(shape))
    X = rng.uniform(-1, 1, shape).astype(np.float32)
    R = rng.uniform(-1, 1, shape[:-1] + (512,)).astype(np.float32)
    dY = rng.uniform(-1, 1, shape[:-1] + (512,)).astype(np.float32)
    np.random.seed(3)
    lin = nn.Linear(128, 512)
    W, b = lin.weight.data.cpu().numpy(), lin.bias.data.cpu().numpy().reshape(-1)

    def run(residual, gemv_on):
        for p in lin.parameters():
            p.grad = None
        x = hip_.Tensor(X, device="cuda")
        r = hip_.Tensor(R, device="cuda") if residual else None
        c0 = counts()
        with hip_.linear_gemv(gemv_on):
            y = lin(x, residual=r) if residual else lin(x)
            out = y.data.cpu().numpy()                                      # (the lazy path launches when .data is first read)
        assert counts()[4] - c0[4] == (1 if gemv_on else 0)
        y.backward(dev(dY))
        return out, [x.grad.cpu().numpy(), lin.weight.grad.cpu().numpy(), lin.bias.grad.cpu().numpy()]

    for residual in (False, True):
        out_off, grads_off = run(residual, False)
        out_on, grads_on = run(residual, True)
        plus = b[None, :] + (R.reshape(-1, 512).astype(np.float64) if residual else 0.0)
        assert_dot_close(out_on.reshape(-1, 512), X.reshape(-1, 128), W.T, c=4, plus=plus, err_msg=f"residual={residual}")
        for name, a, g in zip(("x.grad", "weight.grad", "bias.grad"), grads_off, grads_on):
            np.testing.assert_array_equal(bits(a), bits(g), err_msg=f"{name}: the backward must not see the switch")


# ------------------------------------------------------------------------------------------- 9. GPT-2 tiny
def test_gpt2_tiny_teacher_forced_cached_decode_under_the_switch(switch, tiny):  # noqa: F811
    hip_ = switch
    f, model = tiny["f"], tiny["model"]
    model.eval()
    tokens = f["tokens"]
    c0 = counts()
    with hip_.linear_gemv():
        cache = model.new_cache(1, 40)
        for t in range(40):
            logits = model(tokens[None, t:t + 1], cache=cache).data.cpu().numpy()
            assert_close_scaled(logits[0, 0], f["logits64"][t], tol=1e-4, err_msg=f"step {t}")
        cache = model.new_cache(1, 40)
        logits = model(tokens[None, :8], cache=cache).data.cpu().numpy()
        assert_close_scaled(logits[0], f["logits64"][:8], tol=1e-4, err_msg="prefill")
        for t in range(8, 40):
            logits = model(tokens[None, t:t + 1], cache=cache).data.cpu().numpy()
            assert_close_scaled(logits[0, 0], f["logits64"][t], tol=1e-4, err_msg=f"step {t} after prefill")
    assert counts()[4] > c0[4]
    assert hip_.get_linear_gemv() is False


@pytest.mark.parametrize("mode", ["cached", "graph"])
def test_gpt2_tiny_generate_gemv_returns_the_fixture_tokens(switch, tiny, mode):  # noqa: F811
    hip_ = switch
    f, G, model = tiny["f"], tiny["G"], tiny["model"]
    for before in (False, True):                                            # generate hands the switch back as it found it
        hip_.set_linear_gemv(before)
        c0, stats = counts(), {}
        out = G.generate(model, f["prompt"], 32, mode=mode, stats=stats, linear="gemv")
        assert hip_.get_linear_gemv() is before
        assert out.shape == (1, 40) and out.dtype == np.int32
        np.testing.assert_array_equal(out[0], f["tokens"])
        assert stats["linear"] == "gemv"
        assert counts()[4] > c0[4]
    hip_.set_linear_gemv(False)
    if mode == "graph":
        gemm_stats = {}
        G.generate(model, f["prompt"], 32, mode="graph", stats=gemm_stats)
        assert gemm_stats["linear"] == "gemm"
        assert stats["graph_nodes"] == stats["kernel_nodes"], stats
        assert gemm_stats["graph_nodes"] == gemm_stats["kernel_nodes"], gemm_stats
        assert 0 < stats["kernel_nodes"] <= gemm_stats["kernel_nodes"], (stats, gemm_stats)
    # recompute ignores the flag
    c0 = counts()
    out = G.generate(model, f["prompt"], 4, mode="recompute", linear="gemv")
    np.testing.assert_array_equal(out[0], f["tokens"][:12])
    assert counts()[4] == c0[4] and hip_.get_linear_gemv() is False


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("mode", ["cached", "graph"])
def test_gpt2_tiny_generate_gemv_batches(switch, tiny, mode, B):  # noqa: F811
    f, G, model = tiny["f"], tiny["G"], tiny["model"]
    out = G.generate(model, np.tile(f["prompt"], (B, 1)), 32, mode=mode, linear="gemv")
    for row in range(B):
        np.testing.assert_array_equal(out[row], f["tokens"], err_msg=f"row {row} of {B}")
    assert switch.get_linear_gemv() is False
