"""CPU-only: the C-ABI library loads and exports every symbol include/neunet_hip.h declares, and the ctypes
signature table of the host package covers exactly that set.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "neunet_hip.h")


def header_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nnhip[A-Za-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    import neunet_hip
    from neunet_hip import _lib
    path = _lib.lib_path()
    if not os.path.exists(path):
        import importlib.util
        spec = importlib.util.spec_from_file_location("nnhip_build", os.path.join(ROOT, "numpy-nn-model_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return neunet_hip.load_library()


def test_header_declares_expected_surface():
    syms = header_symbols()
    for must in ["nnhipLinearModuleForward", "nnhipLinearModuleBackward", "nnhipLinearSwishForward",
                 "nnhipLinearSwishBackward", "nnhipSwishForward", "nnhipSwishBackward", "nnhipFusedSwishAndMul",
                 "nnhipFusedSwishAndMulBackward", "nnhipSoftmaxForward", "nnhipSoftmaxBackward",
                 "nnhipCrossEntropyForwardBackward", "nnhipRMSNormForward", "nnhipRMSNormBackward",
                 "nnhipFusedAdamWStep", "nnhipCreateFusedOptimizer", "nnhipDestroyFusedOptimizer",
                 "nnhipFusedAdamWMultiTensorStep", "nnhipConv2dForward", "nnhipConv2dBackward", "nnhipCleanup"]:
        assert must in syms


def test_library_exports_every_declared_symbol(lib):
    missing = [s for s in header_symbols() if not hasattr(lib, s)]
    assert not missing, f"declared in include/neunet_hip.h but not exported: {missing}"


def test_ctypes_table_matches_header(lib):
    from neunet_hip import _lib
    assert sorted(_lib.exported_symbols()) == header_symbols()
    for name in _lib.exported_symbols():
        _lib.load_hip_function(name)  # argtypes bind


def header_struct_fields(name):
    """[(member, array length)] of `typedef struct <name> { ... } <name>;` in the header, in declaration order; every member must be
    a (const) float* array."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S)
    assert m, f"struct {name} not found in include/neunet_hip.h"
    fields = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        f = re.fullmatch(r"(?:const\s+)?float\s*\*\s*(\w+)\s*\[\s*(\d+)\s*\]", decl)
        assert f, f"struct {name}: member {decl!r} is not a float* array"
        fields.append((f.group(1), int(f.group(2))))
    return fields


@pytest.mark.parametrize("cname,pyname,order", [("nnhipLSTMWeights", "LSTMWeights", ["wx", "wh", "b"]),
                                                ("nnhipLSTMGrads", "LSTMGrads", ["dwx", "dwh", "db"])])
def test_lstm_structs_match_header(cname, pyname, order):
    """The two structs the LSTM entries take by pointer: the ctypes mirror has the header's members, in the header's order, each an
    array of four pointers -- twelve pointers, no padding, each member at the offset the C compiler gives it."""
    from neunet_hip import _lib
    cls = getattr(_lib, pyname)
    fields = header_struct_fields(cname)
    assert [n for n, _ in fields] == order
    assert all(k == 4 for _, k in fields)
    assert [n for n, _ in cls._fields_] == order
    psz = ctypes.sizeof(ctypes.c_void_p)
    for idx, (n, t) in enumerate(cls._fields_):
        assert t._type_ is ctypes.c_void_p and t._length_ == 4, n
        assert getattr(cls, n).offset == idx * 4 * psz and getattr(cls, n).size == 4 * psz, n
    assert ctypes.sizeof(cls) == 12 * psz
    argtypes = {"nnhipLSTMWeights": [("nnhipLSTMForward", 1), ("nnhipLSTMBackward", 1)], "nnhipLSTMGrads": [("nnhipLSTMBackward", 8)]}
    for fn, pos in argtypes[cname]:
        assert _lib._SIGNATURES[fn][1][pos] is ctypes.POINTER(cls), (fn, pos)


def test_version_and_error_string(lib):
    from neunet_hip import _lib
    assert _lib.load_hip_function("nnhipVersion")() >= 100
    assert isinstance(_lib.last_error(), str)


def test_argument_errors_are_status_codes_not_exits(lib):
    """Bad arguments come back as negative status (the reference printf+exit()s)."""
    from neunet_hip import _lib
    with pytest.raises(_lib.NeunetHipError, match="negative size"):
        _lib.call_hip_function("nnhipSwishForward", 16, 16, 1.0, -1, None)
    with pytest.raises(_lib.NeunetHipError, match="null"):
        _lib.call_hip_function("nnhipLinearModuleForward", None, None, None, None, 4, 4, 4, None)
    with pytest.raises(_lib.NeunetHipError, match="reduction"):
        _lib.call_hip_function("nnhipCrossEntropyForwardBackward", 16, 16, 16, 16, 4, -100, 2, 4, b"x", 1, None, None, None)


def test_numpy_arrays_rejected_like_reference():
    """utils.py:75-76 of the reference: to_pointer raises TypeError on NumPy input."""
    import numpy as np
    from neunet_hip import _lib
    with pytest.raises(TypeError):
        _lib.to_pointer(np.zeros(4, np.float32))


def test_missing_library_fails_loudly(monkeypatch):
    from neunet_hip import _lib
    monkeypatch.setattr(_lib, "_dll", None)
    monkeypatch.setattr(_lib, "_funcs", {})
    monkeypatch.setenv(_lib.LIB_ENV, "/nonexistent/libneunet_hip.so")
    with pytest.raises(_lib.NeunetHipError, match="no CPU fallback"):
        _lib.load_hip_function("nnhipVersion")


def test_comm_unique_id_needs_no_gpu(lib):
    """The RCCL entry points bind librccl lazily (dlopen): the id for nnhipCommInitRank can be drawn on a GPU-less host, bad
    arguments are status codes, and the library that got bound is an RCCL."""
    import ctypes
    from neunet_hip import _lib
    buf = ctypes.create_string_buffer(128)
    try:
        _lib.call_hip_function("nnhipCommUniqueId", buf)
    except _lib.NeunetHipError as exc:
        pytest.skip(f"no RCCL on this host: {exc}")
    assert any(buf.raw), "ncclGetUniqueId left the buffer untouched"
    path, ver = ctypes.create_string_buffer(256), ctypes.c_int(0)
    _lib.call_hip_function("nnhipCommLibrary", path, 256, ctypes.byref(ver))
    assert b"rccl" in path.value and ver.value > 0
    with pytest.raises(_lib.NeunetHipError, match="null communicator"):
        _lib.call_hip_function("nnhipAllReduceSumF32", None, 16, 4, None)
    with pytest.raises(_lib.NeunetHipError, match="rank"):
        h = ctypes.c_void_p()
        _lib.call_hip_function("nnhipCommInitRank", ctypes.byref(h), buf.raw, 3, 2)
    assert _lib.call_hip_function("nnhipCommDestroy", None) == 0


def test_attention_status_codes_need_no_device(lib):
    """The fused attention entries' argument checks (attn_check, fill_extra and the head of the two entries in csrc/attention.hip) all
    precede the first device call: the pointers here are never dereferenced.  ABI 215: the forward answers NNHIP_EALIGN (it said
    NNHIP_EINVAL) for an O that is not 16-byte aligned, and both entries require LSE 8-byte aligned (the kernels store and load a
    row's (max, log2 sum) as one float2).  (The backward looks at its options after it has asked for its workspace, a device call:
    its two option refusals need a GPU and are not checked here.)"""
    from neunet_hip import _lib
    EINVAL, EALIGN = -1, -2
    assert _lib.load_hip_function("nnhipVersion")() >= 215
    fwd, bwd = _lib.load_hip_function("nnhipAttentionForwardEx"), _lib.load_hip_function("nnhipAttentionBackwardEx")
    D = 0x1000                                                  # non-null, 16-byte aligned, never dereferenced
    base = dict(B=2, H=2, Tq=8, Tk=8, dh=64, ld=0, opts=None)

    def call(entry, names, off, kw):
        s = dict(base, **kw)
        opts = None if s["opts"] is None else ctypes.byref(s["opts"])
        rc = entry(*[D + off.get(n, 0) for n in names], s["B"], s["H"], s["Tq"], s["Tk"], s["dh"], s["ld"], 0.1, 1, opts, None)
        assert rc == 0 or "nnhipAttention" in _lib.last_error()
        return rc

    def forward(off={}, **kw):
        return call(fwd, ("Q", "K", "V", "kv", "O", "LSE"), off, kw)

    def backward(off={}, **kw):
        return call(bwd, ("Q", "K", "V", "kv", "O", "dO", "LSE", "dQ", "dK", "dV"), off, kw)

    for entry, names in ((forward, ("Q", "K", "V", "O")), (backward, ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV"))):
        for n in names:
            for by in (4, 8):
                assert entry({n: by}) == EALIGN, (entry.__name__, n, by)
                assert "16-byte aligned" in _lib.last_error()
            assert entry({n: -D}) == EINVAL and "null" in _lib.last_error(), (entry.__name__, n)
        assert entry({"LSE": 4}) == EALIGN and "LSE 8-byte aligned" in _lib.last_error()
        assert entry({"LSE": -D}) == EINVAL and "null" in _lib.last_error()      # a NULL LSE stays NNHIP_EINVAL
        assert entry(dh=48) == EINVAL and "head_dim" in _lib.last_error()
        assert entry(ld=2 * 64 - 4) == EINVAL and "ld_qkv" in _lib.last_error()
        assert entry(ld=2 * 64 + 2) == EINVAL and "ld_qkv" in _lib.last_error()
        assert entry(H=0) == EINVAL and entry(B=-1) == EINVAL and entry(Tq=1 << 24) == EINVAL
        assert entry(B=0) == 0 and entry(Tq=0) == 0                              # nothing to do: no launch, whatever the pointers are
    assert forward(Tk=0) == EINVAL and "Tk" in _lib.last_error()
    assert backward(Tk=0) == 0
    half, p_one = _lib.AttentionOptions(), _lib.AttentionOptions()
    half.mask_bits = D
    p_one.dropout_p = 1.0
    assert forward({"LSE": 8}, opts=half) == EINVAL and "mask_bitsT" in _lib.last_error()     # (LSE + 8 bytes is aligned)
    assert forward(opts=p_one) == EINVAL and "dropout_p" in _lib.last_error()
