"""Host side of the complex-tap FIR (gr4hip_cfir_*): symbols, every create-time rejection before any device work, the tap operand of the matrix-pipe kernel bit for
bit against the oracle's, and the C++ host mirror (CPU body, settings errors, plugin registration, sample_rate forwarding).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import complex_fir_oracle as CO
import oracle_lib as O

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_complex_fir")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
SYMBOLS = ["gr4hip_cfir_create", "gr4hip_cfir_set_taps", "gr4hip_cfir_reset", "gr4hip_cfir_set_guard_mode", "gr4hip_cfir_process", "gr4hip_cfir_destroy", "gr4hip_cfir_tile",
           "gr4hip_cfir_segment", "gr4hip_cfir_band_table"]


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


def _taps(K, seed=0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(K) + 1j * rng.standard_normal(K)) / np.sqrt(2 * K)).astype(np.complex64)


def test_symbols_exist_and_are_declared(L):
    from gnuradio4_amd import capi
    import gnuradio4_amd as G
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gr4hip.h")).read(), flags=re.S)
    raw = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in gr4hip.h"
        assert hasattr(raw, s) and s in capi.SIGNATURES
    for s in ("gr4hip_internal_cfir_last_paths", "gr4hip_internal_cfir_marked"):  # test hooks: exported, not declared
        assert hasattr(raw, s) and not re.search(r"\b%s\b" % s, text)
    assert hasattr(G, "complex_fir_filter") and "complex_fir_filter" in G.__all__
    assert L.gr4hip_cfir_tile() >= 128 and L.gr4hip_cfir_tile() % 128 == 0  # whole 16 x 16 tiles of 128 complex outputs
    assert L.gr4hip_cfir_segment() >= 128


def test_create_rejections_come_before_any_device_work(L):
    """every one of these returns its status with or without a device: the checks run on the host first"""
    from gnuradio4_amd import capi
    h = C.c_void_p()
    b = _taps(8)
    assert L.gr4hip_cfir_create(C.byref(h), None, 8, 1) == capi.INVALID_ARGUMENT and b"null taps" in L.gr4hip_last_error()
    assert L.gr4hip_cfir_create(C.byref(h), b.ctypes.data, 0, 1) == capi.INVALID_ARGUMENT
    assert L.gr4hip_cfir_create(C.byref(h), b.ctypes.data, 8, 0) == capi.INVALID_ARGUMENT and b"decim" in L.gr4hip_last_error()
    assert L.gr4hip_cfir_create(None, b.ctypes.data, 8, 1) == capi.INVALID_ARGUMENT
    for bad in (np.inf, -np.inf, np.nan):
        for part in (0, 1):
            t = b.copy()
            t.view(np.float32)[2 * 5 + part] = bad
            assert L.gr4hip_cfir_create(C.byref(h), t.ctypes.data, 8, 1) == capi.INVALID_ARGUMENT and b"tap 5 is not finite" in L.gr4hip_last_error()
    big = _taps(2049)
    assert L.gr4hip_cfir_create(C.byref(h), big.ctypes.data, 2049, 1) == capi.UNSUPPORTED
    assert L.gr4hip_cfir_create(C.byref(h), b.ctypes.data, 8, 65) == capi.UNSUPPORTED
    assert not h.value
    # the handle-taking calls refuse a null handle
    assert L.gr4hip_cfir_set_taps(None, b.ctypes.data, 8) == capi.INVALID_ARGUMENT
    assert L.gr4hip_cfir_reset(None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_cfir_set_guard_mode(None, 0) == capi.INVALID_ARGUMENT
    assert L.gr4hip_cfir_process(None, None, 0, None, None, None) == capi.INVALID_ARGUMENT


def test_create_fails_loudly_without_a_gpu(L):
    from gnuradio4_amd import capi
    import gnuradio4_amd as G
    b = _taps(2048)  # the largest supported shape: accepted by the host checks
    h = C.c_void_p()
    rc = L.gr4hip_cfir_create(C.byref(h), b.ctypes.data, len(b), 64)
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        assert L.gr4hip_cfir_destroy(h) == 0
        return
    assert rc == capi.NO_DEVICE and not h.value and b"no HIP device" in L.gr4hip_last_error()
    with pytest.raises(capi.Gr4HipError) as e:
        G.complex_fir_filter(b[:16], 2)  # no silent CPU path in the package
    assert e.value.status == capi.NO_DEVICE


@pytest.mark.parametrize("K,D", [(K, D) for K in (1, 2, 5, 33, 64, 100) for D in (1, 2, 3, 4, 8)] + [(2048, 64), (1024, 16)])
def test_band_table_is_the_oracles_bit_for_bit(L, K, D):
    b = _taps(K, 31 * K + D)
    want, r_min = CO.band_table(b, D, np.float32)
    ns, r0 = C.c_size_t(0), C.c_long(0)
    assert L.gr4hip_cfir_band_table(b.ctypes.data, K, D, None, 0, C.byref(ns), C.byref(r0)) == 0  # size query
    assert ns.value == len(want) and r0.value == r_min
    got = np.full(ns.value * 256 + 3, 7.0, np.float32)
    ns2, r1 = C.c_size_t(0), C.c_long(0)
    assert L.gr4hip_cfir_band_table(b.ctypes.data, K, D, got.ctypes.data, ns.value * 256, C.byref(ns2), C.byref(r1)) == 0
    assert (ns2.value, r1.value) == (ns.value, r_min)
    assert np.array_equal(got[:-3].view(np.uint32), want.ravel().view(np.uint32))  # signed zeros included
    assert np.all(got[-3:] == 7.0)


def test_band_table_rejections(L):
    from gnuradio4_amd import capi
    b = _taps(33)
    out = np.zeros(16, np.float32)
    assert L.gr4hip_cfir_band_table(None, 33, 1, None, 0, None, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_cfir_band_table(b.ctypes.data, 0, 1, None, 0, None, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_cfir_band_table(b.ctypes.data, 33, 0, None, 0, None, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_cfir_band_table(b.ctypes.data, 33, 65, None, 0, None, None) == capi.UNSUPPORTED
    assert L.gr4hip_cfir_band_table(b.ctypes.data, 33, 1, out.ctypes.data, out.size, None, None) == capi.INVALID_ARGUMENT and b"room for" in L.gr4hip_last_error()
    assert np.all(out == 0)
    assert L.gr4hip_cfir_band_table(b.ctypes.data, 33, 1, None, 0, None, None) == 0  # every output is optional


def test_host_mirror_cpu_body_settings_plugin_and_sample_rate():
    """gr::filter::complex_fir_filter<std::complex<float>> of the C++ host mirror on the CPU: the body against values the program computes itself, the settings errors,
    registration in the blocks plugin, and gr:sample_rate forwarded divided by `decimate`"""
    assert os.path.exists(BIN), "build() compiles host/tests/test_host_complex_fir.cpp"
    r = subprocess.run([BIN, "host", PLUGIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "complex_fir host: ok" in r.stdout
