"""Host side of the rational resampler (gr4hip_resamp_*): symbols, every refusal before any device work, and the C++ host mirror (CPU body against the definition over
chunked calls, carried inputs across settings changes, plugin registration, gr:sample_rate forwarded times L / M).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_rational_resampler")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
SYMBOLS = ["gr4hip_resamp_create", "gr4hip_resamp_set_taps", "gr4hip_resamp_reset", "gr4hip_resamp_process", "gr4hip_resamp_destroy", "gr4hip_resamp_tile", "gr4hip_resamp_design"]


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


def _taps(K):
    return O.design_taps_hamming_lowpass(K, 0.1) if K >= 8 else np.full(K, 1.0 / K, np.float32)


def test_symbols_exist_and_are_declared(L):
    from gnuradio4_amd import capi
    import gnuradio4_amd as G
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gr4hip.h")).read(), flags=re.S)
    raw = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in gr4hip.h"
        assert hasattr(raw, s) and s in capi.SIGNATURES
    assert hasattr(raw, "gr4hip_internal_resamp_last_paths") and not re.search(r"\bgr4hip_internal_resamp_last_paths\b", text)  # test hook: exported, not declared
    for name in ("rational_resampler", "design_resampler_taps"):
        assert hasattr(G, name) and name in G.__all__
    assert L.gr4hip_resamp_tile() >= 1 and G.rational_resampler.tile() == L.gr4hip_resamp_tile()


def test_create_refusals_come_before_any_device_work(L):
    """every one of these returns its status with or without a device: the checks run on the host first"""
    from gnuradio4_amd import capi
    h = C.c_void_p()
    b = _taps(8)
    F32, C32 = capi.F32, capi.C32
    assert L.gr4hip_resamp_create(None, F32, b.ctypes.data, 8, 3, 4) == capi.INVALID_ARGUMENT
    assert L.gr4hip_resamp_create(C.byref(h), F32, None, 8, 3, 4) == capi.INVALID_ARGUMENT and b"null taps" in L.gr4hip_last_error()
    assert L.gr4hip_resamp_create(C.byref(h), F32, b.ctypes.data, 0, 3, 4) == capi.INVALID_ARGUMENT
    assert L.gr4hip_resamp_create(C.byref(h), F32, b.ctypes.data, 8, 0, 4) == capi.INVALID_ARGUMENT and b"interp" in L.gr4hip_last_error()
    assert L.gr4hip_resamp_create(C.byref(h), C32, b.ctypes.data, 8, 3, 0) == capi.INVALID_ARGUMENT and b"decim" in L.gr4hip_last_error()
    for bad in (np.inf, -np.inf, np.nan):
        t = b.copy()
        t[5] = bad
        assert L.gr4hip_resamp_create(C.byref(h), F32, t.ctypes.data, 8, 3, 4) == capi.INVALID_ARGUMENT and b"tap 5 is not finite" in L.gr4hip_last_error()
    big = _taps(65537)
    assert L.gr4hip_resamp_create(C.byref(h), F32, big.ctypes.data, 65537, 3, 4) == capi.UNSUPPORTED
    assert L.gr4hip_resamp_create(C.byref(h), F32, b.ctypes.data, 8, 1025, 4) == capi.UNSUPPORTED
    assert L.gr4hip_resamp_create(C.byref(h), C32, b.ctypes.data, 8, 3, 1025) == capi.UNSUPPORTED
    for dtype in (capi.F64, capi.C64, capi.I32, 99, -1):
        assert L.gr4hip_resamp_create(C.byref(h), dtype, b.ctypes.data, 8, 3, 4) == capi.UNSUPPORTED
    assert not h.value
    # the handle-taking calls refuse a null handle
    assert L.gr4hip_resamp_set_taps(None, b.ctypes.data, 8) == capi.INVALID_ARGUMENT
    assert L.gr4hip_resamp_reset(None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_resamp_process(None, None, 0, None, None, None) == capi.INVALID_ARGUMENT


def test_create_fails_loudly_without_a_gpu(L):
    from gnuradio4_amd import capi
    import gnuradio4_amd as G
    b = _taps(65536)  # the largest supported shape: accepted by the host checks
    h = C.c_void_p()
    rc = L.gr4hip_resamp_create(C.byref(h), capi.C32, b.ctypes.data, len(b), 1024, 1024)
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        assert L.gr4hip_resamp_destroy(h) == 0
        return
    assert rc == capi.NO_DEVICE and not h.value and b"no HIP device" in L.gr4hip_last_error()
    with pytest.raises(capi.Gr4HipError) as e:
        G.rational_resampler(b[:16], 3, 4)  # no silent CPU path in the package
    assert e.value.status == capi.NO_DEVICE
    with pytest.raises(capi.Gr4HipError) as e:
        G.rational_resampler(b[:16], 3, 4, torch.float64)
    assert e.value.status == capi.UNSUPPORTED


def test_host_mirror_cpu_body_settings_plugin_and_sample_rate():
    """gr::filter::rational_resampler<float | complex<float>> of the C++ host mirror on the CPU: the body against the literal definition the program evaluates itself
    over chunked calls, the carried inputs kept across new taps and cleared by another rate, the settings errors, both plugin names, gr:sample_rate times L / M"""
    assert os.path.exists(BIN), "build() compiles host/tests/test_host_rational_resampler.cpp"
    r = subprocess.run([BIN, "host", PLUGIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rational_resampler host: ok" in r.stdout
