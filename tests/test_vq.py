"""CPU-only: the float64 restatements of tests/vq_ref.py against the reference's fixtures (tests/golden/vq_quantize.npz,
vqvae_tiny_{frozen,trained}.npz); the tier constant and the bound's constants against the kernel source they restate; ABI 219's two
entries (declarations, status codes without a device); every error of neunet_hip.quantize / vq_loss that needs no device; the kbench
section and the example's exports."""
import importlib.util
import os
import re

import numpy as np
import pytest

import vq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "numpy-nn-model_amd", "csrc")


# ------------------------------------------------------------------------------------------- restatements vs the reference's fixtures
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_nearest_restatement_matches_reference_fixture(golden, tag):
    g = golden("vq_quantize")
    idx, zq = vq_ref.nearest(g[f"z_{tag}"], g[f"codebook_{tag}"])
    np.testing.assert_array_equal(idx, g[f"min_indices_{tag}"])
    np.testing.assert_array_equal(zq, g[f"z_q_{tag}"])                                  # a gather: exact
    assert idx.dtype == np.int32
    if tag == "c":                                                                       # the duplicated code: the lower index
        assert np.array_equal(g["codebook_c"][1], g["codebook_c"][6]) and np.all(idx[:3] == 1)


@pytest.mark.parametrize("tag", ["frozen", "trained"])
def test_loss_restatement_matches_step_fixture(golden, tag):
    """The step fixtures hold what the notebook's own expressions gave.  loss - MSE(x_recon, x) is vq_loss + beta commit_loss; the
    encoder's output receives nothing but dz_e (no straight-through in the notebook), the codebook -- when it trains -- the last-wins
    rows of dz_q plus the reconstruction gradient, of which only the sum is in the fixture: checked here on the rows no code chose."""
    g = golden(f"vqvae_tiny_{tag}")
    idx, zq = vq_ref.nearest(g["z_e"], g["codebook"])
    np.testing.assert_array_equal(idx, g["indices"])
    np.testing.assert_array_equal(zq, g["z_q"])
    d = vq_ref.distances(g["z_e"], g["codebook"])
    scale = (g["z_e"].astype(np.float64) ** 2).sum(1) + (g["codebook"].astype(np.float64) ** 2).sum(1).max()
    assert np.all(vq_ref.second_gap(d) >= 1e-3 * scale)                                  # the seed search's condition
    counts = np.bincount(idx, minlength=g["codebook"].shape[0])
    assert (counts > 0).sum() >= 3 and counts.max() >= 2
    loss, dze, dzq = vq_ref.vq_loss(g["z_e"], g["z_q"], 0.25)
    recon = np.mean((g["x_recon"].astype(np.float64) - g["x"]) ** 2)
    np.testing.assert_allclose(recon + loss, float(g["loss"]), rtol=2e-6)
    lb, eb, qb = vq_ref.vq_loss_bounds(g["z_e"], g["z_q"], 0.25)
    assert 0 < lb < 1e-5 * loss and np.all(eb <= 1e-6 * np.abs(dze) + 1e-44) and np.all(qb <= 1e-6 * np.abs(dzq) + 1e-44)
    n = int(g["n_params"])
    assert n == (23 if tag == "trained" else 22)
    if tag == "trained":
        cb = [i for i in range(n) if g[f"p{i}"].shape == g["codebook"].shape and np.array_equal(g[f"p{i}"], g["codebook"])]
        assert cb == [12]                                                                # parameters() order: encoder, codebook, decoder
        unused = counts == 0
        assert unused.any() and np.all(g["g12"][unused] == 0) and np.all(np.abs(g["g12"][~unused]).sum(1) > 0)
        lw = vq_ref.last_wins_codebook_grad(dzq, idx, g["codebook"].shape[0])
        assert np.all(lw[unused] == 0) and np.all(np.abs(lw[~unused]).sum(1) > 0)


def test_gradient_restatements():
    rng = np.random.default_rng(5)
    ze, zq = rng.standard_normal((6, 3)), rng.standard_normal((6, 3))
    f = lambda a, b: vq_ref.vq_loss(a, b, 0.25)[0]                                       # noqa: E731
    _, dze, dzq = vq_ref.vq_loss(ze, zq, 0.25)
    h = 1e-6
    for i in np.ndindex(ze.shape):
        e = np.zeros_like(ze)
        e[i] = h
        # d/dz_e of the commit term only (beta MSE(z_q.detach(), z_e)), d/dz_q of the vq term only (MSE(z_q, z_e.detach()))
        assert abs((f(ze + e, zq) - f(ze - e, zq)) / (2 * h) * 0.25 / 1.25 - dze[i]) < 1e-8
        assert abs((f(ze, zq + e) - f(ze, zq - e)) / (2 * h) / 1.25 - dzq[i]) < 1e-8
    g = rng.standard_normal((5, 2))
    lw = vq_ref.last_wins_codebook_grad(g, [3, 1, 3, 0, 1], 5)
    np.testing.assert_array_equal(lw, np.stack([g[3], g[4], np.zeros(2), g[2], np.zeros(2)]))
    np.testing.assert_array_equal(vq_ref.straight_through_grad(g), g)


def test_numpy_rule_of_the_restatement():
    e = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [5.0, 5.0]], np.float32)
    z = np.array([[0.9, 0.0], [np.nan, 0.0], [4.0, 4.0]], np.float32)
    np.testing.assert_array_equal(vq_ref.nearest(z, e)[0], [1, 0, 3])                    # tie -> lower index; NaN row -> 0
    e[2, 1] = np.nan
    np.testing.assert_array_equal(vq_ref.nearest(z, e)[0], [2, 0, 2])                    # a NaN code wins every NaN-free row


# ------------------------------------------------------------------------------------------- constants vs the kernel source
def test_constants_restate_the_kernel_source():
    src = open(os.path.join(CSRC, "vector_quantize.hip")).read()
    header = open(os.path.join(ROOT, "include", "neunet_hip.h")).read()
    import neunet_hip
    assert int(re.search(r"#define NNHIP_VQ_NARROW_MAX_D (\d+)", header).group(1)) == vq_ref.VQ_NARROW_MAX_D == neunet_hip.VQ_NARROW_MAX_D == 8
    assert "constexpr int VQ_NARROW_MAX_D = NNHIP_VQ_NARROW_MAX_D;" in src and "if (D <= VQ_NARROW_MAX_D) {" in src
    for name in ("VQ_NARROW_CODES", "VQ_ROWS", "VQ_WIDE_RESIDENT_D", "VQ_LOSS_THREADS"):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == getattr(vq_ref, name), name
    tiles = int(re.search(r"constexpr int VQ_TILES = (\d+);", src).group(1))
    assert 16 * tiles == vq_ref.VQ_SUPER
    assert "switch (D <= VQ_WIDE_RESIDENT_D ? (int)((D + 15) / 16) : 0)" in src and "VQ_WIDE_CASE(16);" in src and "VQ_WIDE_CASE(17)" not in src
    assert 16 * 16 == vq_ref.VQ_WIDE_RESIDENT_D
    # the operations the bounds count: the narrow tier's subtraction + fma per component, the wide tier's one fma per loaded component
    # for the norm, its two cross-lane adds, and the single fmaf(-2, acc, norm) of the score
    assert "const float t = r[j] - tile[c * D + j];" in src and "s = fmaf(t, t, s);" in src
    assert src.count("n += __shfl_xor(n, ") == 2 and "fmaf(-2.f, acc[t][v], n)" in src
    assert "nrm[t] = fmaf(c.q[t].w, c.q[t].w, fmaf(c.q[t].z, c.q[t].z, fmaf(c.q[t].y, c.q[t].y, fmaf(c.q[t].x, c.q[t].x, nrm[t]))));" in src
    assert vq_ref.VQ_WIDE_C == 2.0
    # the loss: one block, block_sum over its 16 waves, the three host-side factors
    assert "block_sum<VQ_LOSS_THREADS / 64>(s, red)" in src and "dim3(1), dim3(VQ_LOSS_THREADS)" in src
    assert "const float cq = 2.0f / (float)n;" in src and "beta * cq" in src and "(1.0f + beta) / (float)n" in src
    assert [vq_ref.vq_loss_sum_c(n) for n in (1, 1024, 1025, 4099)] == [29, 29, 30, 33]
    # one comparator, shared: embedding.hip no longer defines it, both files include the header, the min order is the max order mirrored
    order = open(os.path.join(CSRC, "arg_order.h")).read()
    emb = open(os.path.join(CSRC, "embedding.hip")).read()
    assert order.count("bool arg_better(") == 1 and "return arg_better(-v, i, -bv, bi);" in order
    assert "bool arg_better(" not in emb and "bool arg_better(" not in src
    assert '#include "arg_order.h"' in emb and '#include "arg_order.h"' in src
    build = open(os.path.join(ROOT, "numpy-nn-model_amd", "build.py")).read()
    assert '"vector_quantize.hip"' in build and '"vector_quantize.hip": (r"vq_",)' in build and '"arg_order.h"' in build


def test_bounds_are_what_the_docstring_derives():
    rng = np.random.default_rng(6)
    for D in (2, 8):
        z, e = rng.standard_normal((9, D)), rng.uniform(-1, 1, (5, D))
        d = vq_ref.distances(z, e)
        G = (D + 2) * 2.0 ** -24 / (1 - (D + 2) * 2.0 ** -24)
        np.testing.assert_allclose(vq_ref.nearest_bound(z, e), 2 * G * d.min(1) / (1 - G) + 2 * D * 2.0 ** -149, rtol=1e-12)
    for D in (9, 64, 300):
        z, e = rng.standard_normal((9, D)), rng.uniform(-1, 1, (5, D))
        G = (D + 3) * 2.0 ** -24 / (1 - (D + 3) * 2.0 ** -24)
        ref = 2 * G * (np.linalg.norm(z, axis=1) + np.linalg.norm(e, axis=1).max()) ** 2 + (2 * D + 4) * 2.0 ** -149
        np.testing.assert_allclose(vq_ref.nearest_bound(z, e), ref, rtol=1e-12)
    assert vq_ref.is_narrow(8) and not vq_ref.is_narrow(9)
    # a sequential float32 expansion stays inside the wide bound (and mostly at the float64 argmin) in both of the issue's regimes
    for amp in (0.01, 1.0):
        z, e = rng.standard_normal((130, 20)).astype(np.float32), rng.uniform(-amp, amp, (33, 20)).astype(np.float32)
        acc, nrm = np.zeros((130, 33), np.float32), np.zeros(33, np.float32)
        for j in range(20):
            acc += z[:, j:j + 1] * e[None, :, j]
            nrm += e[:, j] * e[:, j]
        idx = np.argmin(nrm[None, :] - np.float32(2) * acc, axis=1)
        assert np.all(vq_ref.excess(z, e, idx) <= vq_ref.wide_bound(z, e))


# ------------------------------------------------------------------------------------------- ABI 219 without a device
@pytest.fixture(scope="module")
def lib():
    import neunet_hip
    return neunet_hip.load_library()


C_TYPES = {"const float*": "P", "float*": "P", "int32_t*": "P", "int64_t": "c_int64", "float": "c_float", "nnhipStream_t": "c_void_p"}


def test_abi_219_declares_the_new_entries(lib):
    import ctypes

    from neunet_hip import _lib
    assert _lib.load_hip_function("nnhipVersion")() >= 219
    header = open(os.path.join(ROOT, "include", "neunet_hip.h")).read()
    names = {"P": ctypes.c_void_p, "c_int64": ctypes.c_int64, "c_float": ctypes.c_float, "c_void_p": ctypes.c_void_p}
    for name in ("nnhipVQNearest", "nnhipVQLossForwardBackward"):
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header)
        assert m, name
        params = [re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1)[0] for p in m.group(1).split(",")]
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes == [names[C_TYPES[p]] for p in params], (name, params)
    assert "VQVAE.quantize" in header and "min_indices = argmin(distances, axis=1)" in header          # the notebook expressions cited
    assert "loss_fn(z_q, z_e.detach()) + beta * loss_fn(z_q.detach(), z_e)" in header
    assert "NEVER split across" in header and "NNHIP_VQ_NARROW_MAX_D" in header


def test_new_entries_return_status_codes_without_a_device(lib):
    """Every argument check precedes the first device call: the pointers here are never dereferenced."""
    from neunet_hip import _lib
    EINVAL, D = -1, 0x1000
    near, loss = _lib.load_hip_function("nnhipVQNearest"), _lib.load_hip_function("nnhipVQLossForwardBackward")
    for bad in (dict(N=0), dict(D_=0), dict(K=0), dict(N=-1), dict(N=2 ** 31), dict(D_=2 ** 31), dict(K=2 ** 31)):
        a = dict(N=4, D_=3, K=5)
        a.update(bad)
        assert near(D, D, D, D, a["N"], a["D_"], a["K"], None) == EINVAL and "bad sizes" in _lib.last_error(), bad
    for k in range(3):
        ptrs = [D, D, D, D]
        ptrs[k] = None
        assert near(*ptrs, 4, 3, 5, None) == EINVAL and "null pointer" in _lib.last_error(), k
    assert loss(D, D, 0.25, D, D, D, 0, None) == EINVAL and "n must be > 0" in _lib.last_error()
    assert loss(D, D, 0.25, D, D, D, -3, None) == EINVAL
    for k in (0, 1, 3):
        args = [D, D, 0.25, D, D, D]
        args[k] = None
        assert loss(*args, 8, None) == EINVAL and "null pointer" in _lib.last_error(), k


# ------------------------------------------------------------------------------------------- host behaviour of the public functions
def test_quantize_and_vq_loss_errors_on_the_host():
    import neunet_hip
    from neunet_hip import Tensor
    z, cb = Tensor(np.zeros((4, 3), np.float32)), Tensor(np.zeros((5, 3), np.float32))
    for args in ((z.data, cb), (z, cb.data), (None, cb)):
        with pytest.raises(TypeError, match="quantize takes Tensors"):
            neunet_hip.quantize(*args)
    with pytest.raises(NotImplementedError, match="float32"):
        neunet_hip.quantize(Tensor(np.zeros((4, 3)), dtype=np.float64), cb)
    with pytest.raises(NotImplementedError, match="float32"):
        neunet_hip.quantize(z, Tensor(np.zeros((5, 3)), dtype=np.int32))
    for bad in (np.zeros((5,)), np.zeros((2, 5, 3))):
        with pytest.raises(ValueError, match="2-D codebook"):
            neunet_hip.quantize(z, Tensor(bad.astype(np.float32)))
    with pytest.raises(ValueError, match="one D"):
        neunet_hip.quantize(z, Tensor(np.zeros((5, 4), np.float32)))
    with pytest.raises(ValueError, match="one D"):
        neunet_hip.quantize(Tensor(np.float32(1.0)), cb)
    for zz, cc in ((np.zeros((0, 3)), np.zeros((5, 3))), (np.zeros((2, 0, 3)), np.zeros((5, 3))), (np.zeros((4, 3)), np.zeros((0, 3))),
                   (np.zeros((4, 0)), np.zeros((5, 0)))):
        with pytest.raises(ValueError, match="at least one row"):
            neunet_hip.quantize(Tensor(zz.astype(np.float32)), Tensor(cc.astype(np.float32)))
    with pytest.raises(ValueError, match="HIP device"):                                  # well-formed host tensors: no CPU fallback
        neunet_hip.quantize(z, cb)
    with pytest.raises(TypeError, match="vq_loss takes Tensors"):
        neunet_hip.vq_loss(z, z.data)
    with pytest.raises(NotImplementedError, match="float32"):
        neunet_hip.vq_loss(z, Tensor(np.zeros((4, 3)), dtype=np.float64))
    with pytest.raises(ValueError, match="equal shapes"):
        neunet_hip.vq_loss(z, cb)
    with pytest.raises(ValueError, match="at least one element"):
        neunet_hip.vq_loss(Tensor(np.zeros((0, 3), np.float32)), Tensor(np.zeros((0, 3), np.float32)))
    with pytest.raises(ValueError, match="HIP device"):
        neunet_hip.vq_loss(z, z)


# ------------------------------------------------------------------------------------------- tools and the example
def test_kbench_registers_the_vq_section():
    src = open(os.path.join(ROOT, "tools", "kbench.py")).read()
    assert 'if "vq" in only:' in src and '"nnhipVQNearest"' in src
    assert "[(100, 2, 100), (8192, 64, 512), (32768, 64, 1024), (4096, 256, 8192)]" in src


def test_vqvae_example_exports():
    spec = importlib.util.spec_from_file_location("example_vqvae", os.path.join(ROOT, "examples", "vqvae.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CONFIGS["notebook"] == dict(input_size=784, latent_size=2, num_embeddings=100, hidden=(512, 256), batch=100)
    assert mod.CONFIGS["tiny"] == dict(input_size=64, latent_size=2, num_embeddings=10, hidden=(48, 32), batch=12)
    for name in ("forward", "quantize", "loss_function", "train_step", "encode", "decode", "reconstruct"):
        assert callable(getattr(mod.VQVAE, name)), name
    assert callable(mod.main) and callable(mod.synthetic_images)
    assert "requires_grad=False" in mod.__doc__ and "frozen" in mod.__doc__
    with pytest.raises(ValueError, match="frozen"):
        mod.VQVAE(8, 2, 4, codebook="ema")
