"""CPU-only: nnhipSampleTopK's argument checks (status codes, before any launch), the host contracts of neunet_hip.sample_top_k and
generate(sampler=...), and the NumPy restatement of the sampler (tests/sample_ref.py) the GPU tests judge the kernel by."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from sample_ref import candidates, cdf64, check_draw, draw64, ks_distance, uniform
from test_abi import lib  # noqa: F401  (fixture: builds the library if it is missing, loads it)

FAKE = 256      # a non-null, 4-byte aligned "device pointer": every case below is refused before anything is launched


def call(*args):
    from neunet_hip import _lib
    return _lib.call_hip_function("nnhipSampleTopK", *args)


def test_abi_213(lib):  # noqa: F811
    from neunet_hip import _lib
    assert _lib.load_hip_function("nnhipVersion")() >= 213
    assert "nnhipSampleTopK" in _lib.exported_symbols()


@pytest.mark.parametrize("args,match", [
    # out_ids, u_out, logits, rows, n, ld, top_k, temperature, seed, seed_dev, stream
    ((None, None, FAKE, 2, 8, 8, 4, 1.0, 0, None, None), "null pointer"),
    ((FAKE, None, None, 2, 8, 8, 4, 1.0, 0, None, None), "null pointer"),
    ((FAKE, None, FAKE, -1, 8, 8, 4, 1.0, 0, None, None), "negative size"),
    ((FAKE, None, FAKE, 2, 0, 8, 4, 1.0, 0, None, None), "empty row"),
    ((FAKE, None, FAKE, 2, 8, 7, 4, 1.0, 0, None, None), "row stride"),
    ((FAKE, None, FAKE, 1, 1 << 31, 1 << 31, 4, 1.0, 0, None, None), "int32 indices"),
    ((FAKE, None, FAKE, 2, 8, 8, 0, 1.0, 0, None, None), "top_k must be at least 1"),
    ((FAKE, None, FAKE, 2, 8, 8, -3, 1.0, 0, None, None), "top_k must be at least 1"),
    ((FAKE, None, FAKE, 2, 8, 8, 1025, 1.0, 0, None, None), "NNHIP_SAMPLE_MAX_K = 1024"),
    ((FAKE, None, FAKE, 2, 8, 8, 4, float("nan"), 0, None, None), "temperature"),
    ((FAKE, None, FAKE, 2, 8, 8, 4, -0.5, 0, None, None), "temperature"),
])
def test_argument_errors_are_status_codes(lib, args, match):  # noqa: F811
    from neunet_hip import _lib
    with pytest.raises(_lib.NeunetHipError, match=match):
        call(*args)


def test_zero_rows_is_a_no_op(lib):  # noqa: F811
    assert call(None, None, None, 0, 8, 8, 4, 1.0, 0, None, None) == 0
    assert call(None, None, None, 0, 0, 0, 1, 0.0, 7, None, None) == 0


def test_header_states_the_cap():
    text = open(os.path.join(ROOT, "include", "neunet_hip.h")).read()
    import neunet_hip
    assert f"#define NNHIP_SAMPLE_MAX_K {neunet_hip.SAMPLE_MAX_K}" in text


def test_sample_top_k_host_contract():
    """Everything sample_top_k can refuse, it refuses before it touches the device (this machine has none)."""
    import torch
    import neunet_hip
    x = torch.zeros((2, 8))
    for k in (0, -1):
        with pytest.raises(ValueError, match="top_k >= 1"):
            neunet_hip.sample_top_k(x, k)
    with pytest.raises(ValueError, match="top_k <= 1024"):
        neunet_hip.sample_top_k(x, 1025)
    for t in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            neunet_hip.sample_top_k(x, 4, temperature=t)
    with pytest.raises(ValueError, match="on the device"):
        neunet_hip.sample_top_k(x, 4)


def test_generate_sampler_contract():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import gpt2_infer as G
    import inspect
    sig = inspect.signature(G.generate)
    assert sig.parameters["sampler"].default == "host"
    with pytest.raises(ValueError, match="unknown sampler"):
        G.generate(None, [[1, 2, 3]], 4, top_k=5, sampler="gpu")
    with pytest.raises(ValueError, match="unknown sampler"):
        G.generate(None, [[1, 2, 3]], 4, sampler=None)
    assert "sampler" in inspect.signature(G.GraphedDecodeStep.__init__).parameters


# ------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("seed", [0, 1, 4, 12345])
def test_uniform_over_rows_is_uniform(seed):
    u = uniform(seed, 0, 8192)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    d = ks_distance(u)
    print(f"seed {seed}: KS distance {d:.4f} (bound {1.95 / np.sqrt(8192):.4f})")
    assert d < 1.95 / np.sqrt(8192)


@pytest.mark.parametrize("row", [0, 1, 2, 3])
def test_uniform_over_words_is_uniform(row):
    u = uniform(0, np.arange(100, 4196), np.full(4096, row))
    d = ks_distance(u)
    print(f"row {row}: KS distance {d:.4f} (bound {1.95 / np.sqrt(4096):.4f})")
    assert d < 1.95 / np.sqrt(4096)


def test_uniform_adds_seed_and_word_mod_2_32():
    np.testing.assert_array_equal(uniform(7, 5, 64), uniform(12, 0, 64))
    np.testing.assert_array_equal(uniform(0xFFFFFFFE, 5, 64), uniform(3, 0, 64))
    assert not np.array_equal(uniform(7, 5, 64), uniform(7, 6, 64))


def test_candidates_order():
    rng = np.random.default_rng(0)
    for n, k in ((5000, 40), (100, 100), (17, 40), (1, 3)):
        x = rng.choice(np.array([-1.0, 0.0, 0.5, 2.0], np.float32), n)
        np.testing.assert_array_equal(candidates(x, k), np.argsort(-x, kind="stable")[:k])
    x = rng.standard_normal(300).astype(np.float32).round(1)          # many repeated values
    np.testing.assert_array_equal(candidates(x, 64), np.argsort(-x, kind="stable")[:64])
    # what argsort does not say: NaNs first (lowest index first), -0 == +0, -inf last
    x = np.array([0.0, -np.inf, np.nan, 3.0, -0.0, np.nan, 3.0], np.float32)
    np.testing.assert_array_equal(candidates(x, 7), [2, 5, 3, 6, 0, 4, 1])


def test_check_draw_accepts_float64_draws_and_rejects_shifted_ones():
    rng = np.random.default_rng(1)
    for n, k, t in ((1000, 5, 1.3), (4096, 256, 0.7), (64, 8, 1.0), (17, 40, 1.0)):
        x = (rng.standard_normal(n) * 3).astype(np.float32)
        idx = candidates(x, k)
        cdf = cdf64(x, idx, t)
        rejected = 0
        for u in uniform(3, 0, 200):
            tok = draw64(x, k, t, u)
            assert check_draw(x, k, t, u, tok) == 0.0
            j = int(np.nonzero(idx == tok)[0][0])
            other = int(idx[(j + 1) % len(idx)])                      # the next candidate: off by one in the CDF
            width = min(cdf[j] - u, u - (cdf[j - 1] if j else 0.0))   # how far inside its own interval u lies
            if width > (len(idx) + 32) * 2.0 ** -22:
                with pytest.raises(AssertionError):
                    check_draw(x, k, t, u, other)
                rejected += 1
        assert rejected > 150
        with pytest.raises(AssertionError, match="not among"):
            check_draw(x, min(k, n - 1), t, 0.5, int(np.argmin(x)))
    # masked vocabulary and degenerate rows
    x = np.full(50, -np.inf, np.float32)
    x[[7, 20, 33]] = [0.0, 1.0, 0.5]
    assert draw64(x, 40, 1.0, 0.999999) in (7, 20, 33)
    with pytest.raises(AssertionError):
        check_draw(x, 40, 1.0, 0.999999, 0)
    check_draw(np.full(9, -np.inf, np.float32), 4, 1.0, 0.3, 0)
    with pytest.raises(AssertionError, match="degenerate"):
        check_draw(np.array([1.0, np.nan, 2.0], np.float32), 2, 1.0, 0.3, 2)
    check_draw(np.array([1.0, np.nan, 2.0], np.float32), 2, 1.0, 0.3, 1)
