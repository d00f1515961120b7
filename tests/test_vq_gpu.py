"""GPU: the vector-quantisation entries (csrc/vector_quantize.hip) through the C ABI against the float64 restatements of
tests/vq_ref.py; neunet_hip.quantize / vq_loss on the tape; and one whole training step of examples/vqvae.py against the step the
reference ran (tests/golden/vqvae_tiny_{frozen,trained}.npz).

Bounds.  The search: near-optimality in exact arithmetic, d(n, idx[n]) - min_k d(n, k) <= bound_n with bound_n derived per tier in
vq_ref's docstring, on EVERY row; equality with the float64 argmin wherever the gap between the two nearest codes exceeds bound_n; z_q
bit-equal to the chosen code.  The loss and its gradients: vq_ref.vq_loss_bounds.  Whole steps: the bounds of
test_mlp_generative_gpu.test_vae_step_vs_reference.  Each test prints its largest error / bound ratio before it asserts (run with -s)."""
import os
import sys

import numpy as np
import pytest

import vq_ref
from test_hip_parity import assert_within, grad_list_scale
from test_mlp_generative_gpu import check_first_adam_step, check_grads, load_params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
NAN = float("nan")
SENTINEL = -7777
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


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


def dev(a, dtype=np.float32, offset=0):
    """A device copy; offset = 1: one float into its buffer (data_ptr() % 16 == 4)."""
    a = np.ascontiguousarray(np.asarray(a).astype(dtype))
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    out = buf[offset:].view(a.shape)
    out.copy_(torch.from_numpy(a))
    assert offset == 0 or out.data_ptr() % 16 == 4
    return out


def host(t):
    return t.detach().cpu().numpy()


def run_nearest(z, e, with_zq=True, offset=0):
    """nnhipVQNearest into sentinel / NaN-filled buffers one element longer than needed; returns (idx, z_q) on the host after checking
    that the extra element is untouched."""
    N, D = z.shape
    K = e.shape[0]
    ibuf = torch.full((N + 1 + offset,), SENTINEL, dtype=torch.int32, device="cuda")
    qbuf = torch.full((N * D + 1 + offset,), NAN, dtype=torch.float32, device="cuda")
    idx, zq = ibuf[offset:offset + N], qbuf[offset:offset + N * D]
    call("nnhipVQNearest", dev(z, offset=offset), dev(e, offset=offset), idx, zq if with_zq else None, N, D, K)
    ih, qh = host(ibuf), host(qbuf)
    assert ih[offset + N] == SENTINEL and np.all(ih[:offset] == SENTINEL), "idx: written past the end"
    assert np.isnan(qh[offset + N * D]) and np.all(np.isnan(qh[:offset])), "zq: written past the end"
    if not with_zq:
        assert np.all(np.isnan(qh)), "zq = NULL: something was written"
    return ih[offset:offset + N].copy(), qh[offset:offset + N * D].reshape(N, D).copy()


def check_search(tag, z, e, idx, zq):
    """The four properties of the module docstring, on every row."""
    K = e.shape[0]
    assert idx.dtype == np.int32 and np.all((idx >= 0) & (idx < K)), f"{tag}: index out of range"
    d = vq_ref.distances(z, e)
    bound = vq_ref.nearest_bound(z, e, d)
    ex = vq_ref.excess(z, e, idx, d)
    clear = vq_ref.second_gap(d) > bound
    print(f"{tag}: worst (d(idx) - d_min) / bound = {float(np.max(ex / bound)):.4f}; {int(clear.sum())} of {len(idx)} rows have a gap above their "
          f"bound, {int(np.sum(idx != d.argmin(1)))} rows differ from the float64 argmin")
    assert np.all(ex <= bound), f"{tag}: {int(np.sum(ex > bound))} rows farther from optimal than their bound"
    assert np.array_equal(idx[clear], d.argmin(1).astype(np.int32)[clear]), f"{tag}: a clear row misses the float64 argmin"
    if zq is not None:
        assert np.array_equal(zq.view(np.int32), np.asarray(e, np.float32)[idx].view(np.int32)), f"{tag}: z_q is not a bit copy of the chosen code"
    return d, bound


def operands(rng, N, D, K, amp):
    return rng.standard_normal((N, D)).astype(np.float32), rng.uniform(-amp, amp, (K, D)).astype(np.float32)


# ===================================================================================================== the kernel against float64
SHAPES = [(1, 1, 1), (5, 3, 7), (100, 2, 100), (130, 8, 33), (130, 9, 33), (257, 64, 512), (67, 20, 1000), (33, 40, 50), (21, 100, 45),
          (18, 256, 70), (37, 260, 70), (19, 261, 40), (4099, 4, 1024)]


@pytest.mark.parametrize("amp", [0.01, 1.0], ids=["codes0.01", "codes1"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nearest_vs_float64(hip, shape, amp):
    """Degenerate sizes, a small ragged case, the notebook, the last narrow D, the first wide D (k tail of 1), a row tile + 1, K no
    multiple of 16, three and seven k-groups, the last register-resident D, D just past it (16-byte loads and scalar loads), many narrow
    blocks over two LDS tiles."""
    N, D, K = shape
    rng = np.random.default_rng(N * 1000003 + D * 1009 + K)
    z, e = operands(rng, N, D, K, amp)
    idx, zq = run_nearest(z, e)
    check_search(f"\n{shape} +-{amp}", z, e, idx, zq)


TIERS = {"narrow": (37, 4, 600), "wide": (37, 20, 100), "wide-looped": (21, 264, 100)}


def last_partial_tile(tier, K):
    return (K - 1) // vq_ref.VQ_NARROW_CODES * vq_ref.VQ_NARROW_CODES if tier == "narrow" else (K - 1) // 16 * 16


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_planted_answers(hip, tier):
    """The nearest code at index K - 1, at the first index of the last partial code tile, one for row N - 1, and a row EQUAL to a code."""
    N, D, K = TIERS[tier]
    rng = np.random.default_rng(11)
    z, e = operands(rng, N, D, K, 1.0)
    first = last_partial_tile(tier, K)
    assert 0 < first < K - 1 and (K - first) % 16 != 0
    plant = {0: K - 1, 1: first, N - 1: 7, 2: 3}
    for row, code in plant.items():
        e[code] = z[row] + (np.float32(0) if row == 2 else np.float32(1e-3))
    idx, zq = run_nearest(z, e)
    check_search(f"\nplanted {tier}", z, e, idx, zq)
    for row, code in plant.items():
        assert idx[row] == code, (row, code, idx[row])
    assert np.array_equal(zq[2].view(np.int32), z[2].view(np.int32))


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_duplicated_codebook_resolves_to_the_lower_half(hip, tier):
    """codebook[K/2:] = codebook[:K/2]: every code ties with its copy bit for bit (the norm is computed by the same instruction
    sequence wherever a code sits), so every index is below K/2 -- whichever lane, tile, wave or LDS tile the copy lands in."""
    N, D, K = TIERS[tier]
    rng = np.random.default_rng(12)
    z, e = operands(rng, N, D, K, 1.0)
    e[K // 2:] = e[:K // 2]
    idx, zq = run_nearest(z, e)
    check_search(f"\nduplicated {tier}", z, e, idx, zq)
    assert np.all(idx < K // 2)


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_close_pair_three_bounds_apart(hip, tier):
    """For ten rows, two codes near the row whose float64 distances differ by 3 bound_n: the nearer one must be chosen, whether it has
    the lower or the higher index."""
    N, D, K = TIERS[tier]
    rng = np.random.default_rng(13)
    z, e = operands(rng, N, D, K, 1.0)
    # The narrow bound is ~7e-7 of the distance itself, so the pair must be resolvable in float32: the ten rows sit near ten corners of
    # a cube of half-side 0.4 (0.8 apart), each pair r = 0.2 from its row (components below 1: one float32 spacing of the second code
    # moves the gap by less than half a bound), and every other code is moved 3 away along component 0, so the pair stays the row's
    # two nearest.
    r = 0.2
    corners = np.array([[0.4 if (i >> j) & 1 else -0.4 for j in range(4)] + [0.0] * (D - 4) for i in range(10)])
    z[:10] = (corners + rng.uniform(-0.05, 0.05, (10, D))).astype(np.float32)
    e[:, 0] += np.float32(3.0)
    v = rng.standard_normal((10, D))
    v = (r * v / np.linalg.norm(v, axis=1, keepdims=True))
    for i in range(10):
        e[20 + 2 * i + (i & 1)] = (z[i] + v[i]).astype(np.float32)                       # odd i: the nearer code has the HIGHER index
        e[20 + 2 * i + 1 - (i & 1)] = e[20 + 2 * i + (i & 1)]                            # (placeholder until the bound is known)
    bound = vq_ref.nearest_bound(z, e)
    for i in range(10):
        a, b = 20 + 2 * i + (i & 1), 20 + 2 * i + 1 - (i & 1)
        delta = np.sqrt(1.0 + 3.0 * bound[i] / r ** 2) - 1.0
        e[b] = (z[i] + v[i] * (1.0 + delta)).astype(np.float32)
        # both codes were rounded to float32, which moves a narrow-tier gap by about a bound: walk the second code's largest component
        # outward or inward one float32 at a time until the float64 gap is 3 bounds to within a half
        j = int(np.argmax(np.abs(v[i])))
        gap = lambda: (vq_ref.distances(z[i:i + 1], e[b:b + 1]) - vq_ref.distances(z[i:i + 1], e[a:a + 1]))[0, 0] / bound[i]      # noqa: E731
        for _ in range(400):
            if abs(gap() - 3.0) <= 0.5:
                break
            away = np.float32(np.inf) * np.sign(np.float32(v[i, j]))
            e[b, j] = np.nextafter(e[b, j], away if gap() < 3.0 else -away)
    d = vq_ref.distances(z, e)
    bound = vq_ref.nearest_bound(z, e, d)
    near = np.array([20 + 2 * i + (i & 1) for i in range(10)])
    ratio = vq_ref.second_gap(d)[:10] / bound[:10]
    print(f"\nclose pair {tier}: gap / bound of the ten rows: {np.round(ratio, 2)}")
    assert np.array_equal(d[:10].argmin(1), near) and np.all((ratio > 2.0) & (ratio < 4.0))      # the construction is what it says
    idx, zq = run_nearest(z, e)
    check_search(f"close pair {tier}", z, e, idx, zq)
    assert np.array_equal(idx[:10], near)


@pytest.mark.parametrize("tier", sorted(TIERS))
def test_nan_rule(hip, tier):
    """np.argmin's: a NaN in one row gives index 0 for that row only; a NaN in code 5 gives 5 for every NaN-free row; NaNs in codes 5
    and 2 give 2."""
    N, D, K = TIERS[tier]
    rng = np.random.default_rng(14)
    z, e = operands(rng, N, D, K, 1.0)
    clean, _ = run_nearest(z, e)
    zn = z.copy()
    zn[3, D - 1] = NAN
    idx, zq = run_nearest(zn, e)
    assert idx[3] == 0 and np.array_equal(np.delete(idx, 3), np.delete(clean, 3))
    assert np.array_equal(zq.view(np.int32), e[idx].view(np.int32))
    e5 = e.copy()
    e5[5, 0] = NAN
    idx, zq = run_nearest(z, e5)
    assert np.all(idx == 5) and np.array_equal(zq.view(np.int32), e5[idx].view(np.int32))
    idx, _ = run_nearest(zn, e5)                                                         # the NaN row scores NaN everywhere: the first
    assert idx[3] == 0 and np.all(np.delete(idx, 3) == 5)
    eL = e.copy()
    eL[K - 2, 1] = NAN                                                                   # in the last code tile, another wave's share
    idx, _ = run_nearest(z, eL)
    assert np.all(idx == K - 2)
    e52 = e5.copy()
    e52[2, D - 1] = NAN
    idx, _ = run_nearest(z, e52)
    assert np.all(idx == 2)
    np.testing.assert_array_equal(idx, vq_ref.nearest(z, e52)[0])


@pytest.mark.parametrize("shape", [(100, 2, 100), (67, 20, 1000), (257, 64, 512), (37, 260, 70)], ids=lambda s: "x".join(map(str, s)))
def test_null_zq_offset_operands_and_reruns(hip, shape):
    """zq = NULL writes nothing but idx; operands one float into their buffers (no 16-byte loads) give the same indices; two runs are
    bit-identical."""
    N, D, K = shape
    rng = np.random.default_rng(15)
    z, e = operands(rng, N, D, K, 1.0)
    idx, zq = run_nearest(z, e)
    idx_only, _ = run_nearest(z, e, with_zq=False)
    np.testing.assert_array_equal(idx_only, idx)
    idx_off, zq_off = run_nearest(z, e, offset=1)
    check_search(f"\n{shape} offset operands", z, e, idx_off, zq_off)
    np.testing.assert_array_equal(idx_off, idx)                                          # the same arithmetic, whatever the load width
    idx2, zq2 = run_nearest(z, e)
    assert np.array_equal(idx2, idx) and np.array_equal(zq2.view(np.int32), zq.view(np.int32))


@pytest.mark.parametrize("shape", [(100, 2, 100), (67, 20, 1000)], ids=lambda s: "x".join(map(str, s)))
def test_nearest_in_a_captured_graph(hip, shape):
    """One launch, no workspace, no host synchronisation: capture the call, change the inputs in place, replay -- equal to the eager call."""
    N, D, K = shape
    rng = np.random.default_rng(16)
    z, e = operands(rng, N, D, K, 1.0)
    zd, ed = dev(z), dev(e)
    idx, zq = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((N, D), NAN, device="cuda")
    call("nnhipVQNearest", zd, ed, idx, zq, N, D, K)                                     # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call("nnhipVQNearest", zd, ed, idx, zq, N, D, K)
    z2, e2 = operands(rng, N, D, K, 1.0)
    zd.copy_(torch.from_numpy(z2))
    ed.copy_(torch.from_numpy(e2))
    idx.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    ref_idx, ref_zq = run_nearest(z2, e2)
    np.testing.assert_array_equal(host(idx), ref_idx)
    assert np.array_equal(host(zq).view(np.int32), ref_zq.view(np.int32))


def test_einval_returns_without_a_launch(hip):
    from neunet_hip import _lib
    f = _lib.load_hip_function("nnhipVQNearest")
    z, e = dev(np.zeros((4, 3))), dev(np.zeros((5, 3)))
    idx, zq = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((4, 3), NAN, device="cuda")
    st = _lib.get_current_stream_ptr()
    P = lambda t: None if t is None else t.data_ptr()                                    # noqa: E731
    for N, D, K in ((0, 3, 5), (4, 0, 5), (4, 3, 0), (-1, 3, 5), (2 ** 31, 3, 5), (4, 2 ** 31, 5), (4, 3, 2 ** 31)):
        assert f(P(z), P(e), P(idx), P(zq), N, D, K, st) == -1 and "bad sizes" in _lib.last_error()
    for args in ((None, e, idx, zq), (z, None, idx, zq), (z, e, None, zq)):
        assert f(*[P(t) for t in args], 4, 3, 5, st) == -1 and "null pointer" in _lib.last_error()
    torch.cuda.synchronize()
    assert np.all(host(idx) == SENTINEL) and np.all(np.isnan(host(zq)))
    lf = _lib.load_hip_function("nnhipVQLossForwardBackward")
    loss = torch.full((1,), NAN, device="cuda")
    assert lf(P(z), P(z), 0.25, P(loss), None, None, 0, st) == -1 and lf(None, P(z), 0.25, P(loss), None, None, 12, st) == -1
    torch.cuda.synchronize()
    assert np.isnan(host(loss)[0])


# ===================================================================================================== the loss
@pytest.mark.parametrize("beta", [0.0, 0.25])
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_vq_loss_kernel(hip, n, beta):
    """Value and both gradients within vq_ref's bounds; either gradient pointer NULL; nothing past the end."""
    rng = np.random.default_rng(n)
    ze, zq = rng.standard_normal(n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    ref_loss, ref_e, ref_q = vq_ref.vq_loss(ze, zq, beta)
    lb, eb, qb = vq_ref.vq_loss_bounds(ze, zq, beta)
    worst = 0.0
    for want_e, want_q in ((True, True), (True, False), (False, True), (False, False)):
        loss = torch.full((2,), NAN, device="cuda")
        de, dq = torch.full((n + 1,), NAN, device="cuda"), torch.full((n + 1,), NAN, device="cuda")
        call("nnhipVQLossForwardBackward", dev(ze), dev(zq), beta, loss, de[:n] if want_e else None, dq[:n] if want_q else None, n)
        lh, eh, qh = host(loss), host(de), host(dq)
        assert np.isnan(lh[1]) and np.isnan(eh[n]) and np.isnan(qh[n])
        worst = max(worst, abs(lh[0] - ref_loss) / lb)
        assert abs(lh[0] - ref_loss) <= lb, (lh[0], ref_loss, lb)
        if want_e:
            worst = max(worst, float(np.max(np.abs(eh[:n] - ref_e) / eb)))
            assert_within(eh[:n], ref_e, eb, "dz_e")
        else:
            assert np.all(np.isnan(eh))
        if want_q:
            worst = max(worst, float(np.max(np.abs(qh[:n] - ref_q) / qb)))
            assert_within(qh[:n], ref_q, qb, "dz_q")
        else:
            assert np.all(np.isnan(qh))
    if beta == 0.0:
        assert np.all(ref_e == 0)
    print(f"\nvq_loss n={n} beta={beta}: worst error / bound = {worst:.3f}")


# ===================================================================================================== quantize / vq_loss on the tape
def tape_case(hip, codebook, straight_through, shape=(12, 3), K=5, seed=21):
    from neunet_hip import Tensor
    from neunet_hip.nn import Parameter
    rng = np.random.default_rng(seed)
    zh, eh = rng.standard_normal(shape).astype(np.float32), rng.uniform(-1, 1, (K, shape[-1])).astype(np.float32)
    z = Tensor(zh, device="cuda", requires_grad=True)
    cb = Tensor(eh, device="cuda", requires_grad=False)
    if codebook == "trained":
        cb = Parameter(cb)
    z_q, indices = hip.quantize(z, cb, straight_through=straight_through)
    return rng, zh, eh, z, cb, z_q, indices


@pytest.mark.parametrize("straight_through", [False, True], ids=["", "straight-through"])
@pytest.mark.parametrize("codebook", ["frozen", "trained"])
def test_quantize_on_the_tape(hip, codebook, straight_through):
    """z_q.backward(G) and (vq_loss + a second consumer).backward(): the codebook's gradient is the last-wins assignment of z_q's
    accumulated gradient, z receives dz_e and -- with straight_through -- z_q's gradient unchanged; neither on: z_q is off the tape."""
    rng, zh, eh, z, cb, z_q, indices = tape_case(hip, codebook, straight_through)
    ref_idx, ref_zq = vq_ref.nearest(zh, eh)
    idx = host(indices.data)
    assert indices.requires_grad is False and indices.shape == (12,) and idx.dtype == np.int32
    np.testing.assert_array_equal(idx, ref_idx)
    assert np.array_equal(host(z_q.data).view(np.int32), ref_zq.view(np.int32))
    assert np.bincount(idx).max() >= 2                                                   # repeated indices: last-wins shows
    on_tape = codebook == "trained" or straight_through
    assert z_q.requires_grad is on_tape
    G = rng.standard_normal(zh.shape).astype(np.float32)
    z_q.backward(torch.from_numpy(G).cuda())
    if codebook == "trained":
        np.testing.assert_array_equal(host(cb.grad), vq_ref.last_wins_codebook_grad(G, idx, 5).astype(np.float32))      # a copy: exact
    else:
        assert cb.grad is None
    if straight_through:
        np.testing.assert_array_equal(host(z.grad), vq_ref.straight_through_grad(G).astype(np.float32))
    else:
        assert z.grad is None
    # through the loss
    rng, zh, eh, z, cb, z_q, indices = tape_case(hip, codebook, straight_through)
    loss = hip.vq_loss(z, z_q, beta=0.25)
    assert loss.shape == () and loss.requires_grad
    loss.backward()
    ref_loss, dze, dzq = vq_ref.vq_loss(zh, ref_zq, 0.25)
    lb, eb, qb = vq_ref.vq_loss_bounds(zh, ref_zq, 0.25)
    assert abs(loss.item() - ref_loss) <= lb
    ref_z = dze + (vq_ref.straight_through_grad(dzq) if straight_through else 0.0)
    zb = eb + (qb + 2.0 ** -24 * np.abs(ref_z) if straight_through else 0.0)             # two gradients added: one more rounding
    print(f"\n{codebook} {'straight-through' if straight_through else ''}: z.grad worst error / bound = "
          f"{float(np.max(np.abs(host(z.grad) - ref_z) / zb)):.3f}")
    assert_within(host(z.grad), ref_z, zb, "z.grad")
    if codebook == "trained":
        assert_within(host(cb.grad), vq_ref.last_wins_codebook_grad(dzq, idx, 5), vq_ref.last_wins_codebook_grad(qb, idx, 5), "codebook.grad")
        assert np.all(host(cb.grad)[np.bincount(idx, minlength=5) == 0] == 0)
    else:
        assert cb.grad is None and (straight_through or z_q.grad is None)


def test_quantize_3d_and_fixture(hip, golden):
    from neunet_hip import Tensor
    rng, zh, eh, z, cb, z_q, indices = tape_case(hip, "trained", True, shape=(2, 6, 3))
    ref_idx, ref_zq = vq_ref.nearest(zh, eh)
    assert indices.shape == (2, 6) and z_q.shape == (2, 6, 3)
    np.testing.assert_array_equal(host(indices.data).reshape(-1), ref_idx)
    assert np.array_equal(host(z_q.data).reshape(-1, 3).view(np.int32), ref_zq.view(np.int32))
    G = rng.standard_normal(zh.shape).astype(np.float32)
    z_q.backward(torch.from_numpy(G).cuda())
    np.testing.assert_array_equal(host(cb.grad), vq_ref.last_wins_codebook_grad(G, ref_idx, 5).astype(np.float32))
    np.testing.assert_array_equal(host(z.grad), G)
    g = golden("vq_quantize")
    for tag in "abc":
        zq, ind = hip.quantize(Tensor(g[f"z_{tag}"], device="cuda"), Tensor(g[f"codebook_{tag}"], device="cuda", requires_grad=False))
        np.testing.assert_array_equal(host(ind.data), g[f"min_indices_{tag}"])
        np.testing.assert_array_equal(host(zq.data), g[f"z_q_{tag}"])
        assert zq.requires_grad is False


def test_vq_loss_under_a_non_unit_upstream_gradient(hip):
    rng, zh, eh, z, cb, z_q, indices = tape_case(hip, "trained", False)
    idx = host(indices.data)
    loss = hip.vq_loss(z, z_q, beta=0.25)
    loss.backward(np.float32(3.0))
    _, dze, dzq = vq_ref.vq_loss(zh, eh[idx], 0.25)
    _, eb, qb = vq_ref.vq_loss_bounds(zh, eh[idx], 0.25)
    assert_within(host(z.grad), 3.0 * dze, 3.0 * eb + 2.0 ** -24 * np.abs(3.0 * dze), "z.grad")
    assert_within(host(cb.grad), vq_ref.last_wins_codebook_grad(3.0 * dzq, idx, 5),
                  vq_ref.last_wins_codebook_grad(3.0 * qb + 2.0 ** -24 * np.abs(3.0 * dzq), idx, 5), "codebook.grad")


# ===================================================================================================== whole steps
@pytest.mark.parametrize("tag", ["frozen", "trained"])
def test_vqvae_step_vs_reference(hip, golden, tag):
    """One training step of the notebook's VQVAE class as the reference ran it (64 pixels, hidden 48 / 32, latent 2, 10 codes, batch 12)
    through examples/vqvae.py at --config tiny, from the fixture's initial state.  The fixture's seed keeps every row's two nearest
    codes 1e-3 (|z|^2 + max|e|^2) apart, so the indices must EQUAL the reference's; everything else is held to the bounds of
    test_vae_step_vs_reference (the loss, an O(1) mean here, to 1e-6 relative)."""
    import vqvae as example
    from neunet_hip import Tensor
    from neunet_hip.optim import Adam
    f = golden(f"vqvae_tiny_{tag}")
    cfg = [int(v) for v in f["cfg"]]
    tiny = example.CONFIGS["tiny"]
    assert cfg == [tiny["input_size"], *tiny["hidden"], tiny["latent_size"], tiny["num_embeddings"], tiny["batch"]]
    model = example.VQVAE(cfg[0], cfg[3], cfg[4], (cfg[1], cfg[2]), codebook=tag).to("cuda")
    params = model.parameters()
    n = int(f["n_params"])
    assert len(params) == n
    load_params(params, f, "p")
    if tag == "frozen":
        model.codebook.weight.data.copy_(torch.from_numpy(f["codebook"]).cuda())
        assert all(p is not model.codebook.weight for p in params) and model.codebook.weight.requires_grad is False
    else:
        assert params[12] is model.codebook.weight and np.array_equal(host(params[12].data), f["codebook"])
    lr = 0.0005
    opt = Adam(params, lr=lr)
    model.train()
    x = Tensor(f["x"], device="cuda", requires_grad=False)
    z_e = model.encoder(x)
    z_q, indices = model.quantize(z_e)
    x_recon = model.decoder(z_q)
    loss = model.loss_function(x, x_recon, z_e, z_q)
    opt.zero_grad()
    loss.backward()
    np.testing.assert_array_equal(host(indices.data), f["indices"])
    np.testing.assert_array_equal(host(z_q.data), f["z_q"])
    assert z_q.requires_grad is (tag == "trained")
    ref_loss = float(f["loss"])
    print(f"\nvqvae {tag}: loss {loss.item():.7f} vs {ref_loss:.7f}: |difference| / (1e-6 |loss|) = "
          f"{abs(loss.item() - ref_loss) / (1e-6 * abs(ref_loss)):.3f}")
    assert loss.shape == ()
    assert abs(loss.item() - ref_loss) < 1e-6 * abs(ref_loss)
    np.testing.assert_allclose(host(z_e.data), f["z_e"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(host(x_recon.data), f["x_recon"], rtol=1e-4, atol=1e-5)
    grads = [f[f"g{i}"] for i in range(n)]
    gscale = grad_list_scale(grads)
    check_grads(f"vqvae {tag}", params, grads, gscale)
    opt.step()
    check_first_adam_step(f"vqvae {tag}", params, grads, [f[f"p_after{i}"] for i in range(n)], lr, gscale)
    bns = [m for seq in (model.encoder, model.decoder) for m in seq.modules if isinstance(m, hip.nn.BatchNorm1d)]
    np.testing.assert_allclose(np.concatenate([host(m.running_mean.data).reshape(-1) for m in bns]), f["bn_running_mean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(np.concatenate([host(m.running_var.data).reshape(-1) for m in bns]), f["bn_running_var"], rtol=1e-5, atol=1e-6)
    if tag == "frozen":
        assert np.array_equal(host(model.codebook.weight.data).view(np.int32), f["codebook"].view(np.int32))      # unchanged bit for bit
        assert model.codebook.weight.grad is None
        assert all(p is not model.codebook.weight for p in model.parameters())
