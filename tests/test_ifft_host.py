"""Host side of the inverse transform and the polyphase synthesis bank (gr4hip_ifft_* / gr4hip_pfb_synth_*): symbols, every create-time refusal before any
device work, and the C++ host mirror (gr::blocks::fft::InverseFFT / PfbSynthesizer: CPU bodies against the float64 oracle, settings errors, the history across
settings changes, plugin registration).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pfb_oracle as PO
import synthesis_oracle as SO

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_ifft")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
SYMBOLS = ["gr4hip_ifft_create", "gr4hip_ifft_process", "gr4hip_ifft_destroy", "gr4hip_pfb_synth_create", "gr4hip_pfb_synth_set_taps", "gr4hip_pfb_synth_reset",
           "gr4hip_pfb_synth_process", "gr4hip_pfb_synth_destroy"]
NAMES = ("gr::blocks::fft::InverseFFT<complex<float32>>", "gr::blocks::fft::InverseFFT<float32>", "gr::blocks::fft::PfbSynthesizer<complex<float32>>")
TOL = 1e-5  # the parity contract (include/gr4hip.h); the bodies are a float64 transform rounded to float and float32 sums


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    assert os.path.exists(BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_ifft.cpp and the plugin"
    prefix = str(tmp_path_factory.mktemp("ifft") / "host")
    r = subprocess.run([BIN, "host", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r, prefix


def _c(path):
    return np.fromfile(path, np.float32).view(np.complex64)


def test_symbols_exist_and_are_declared(L):
    from gnuradio4_amd import capi
    import gnuradio4_amd as G
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gr4hip.h")).read(), flags=re.S)
    raw = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in gr4hip.h"
        assert hasattr(raw, s) and s in capi.SIGNATURES
    assert re.search(r"#define\s+GR4HIP_IFFT_SCALE\s+1\b", text) and capi.IFFT_SCALE == 1
    assert re.search(r"#define\s+GR4HIP_ABI_VERSION\s+1\b", text)
    for name in ("InverseFFT", "PolyphaseSynthesisBank"):
        assert hasattr(G, name) and name in G.__all__


def test_create_refusals_come_before_any_device_work(L):
    """every one of these returns its status with or without a device, and leaves the handle it was given untouched: the checks run on the host first"""
    from gnuradio4_amd import capi
    N, P = 64, 4
    g = PO.design(N, P)
    SENT = 0x5A5A5A5A

    def ifft(dtype, n, window=0, flags=0):
        hd = C.c_void_p(SENT)
        rc = L.gr4hip_ifft_create(C.byref(hd), dtype, n, window, flags)
        assert (hd.value == SENT) == (rc != capi.OK), "a refused create wrote its handle"
        if rc == capi.OK:
            L.gr4hip_ifft_destroy(hd)
        return rc

    def bank(n, p, taps, flags=0):
        hd = C.c_void_p(SENT)
        rc = L.gr4hip_pfb_synth_create(C.byref(hd), n, p, taps.ctypes.data if taps is not None else None, flags)
        assert (hd.value == SENT) == (rc != capi.OK), "a refused create wrote its handle"
        if rc == capi.OK:
            L.gr4hip_pfb_synth_destroy(hd)
        return rc

    assert L.gr4hip_ifft_create(None, capi.C32, N, 0, 0) == capi.INVALID_ARGUMENT
    assert L.gr4hip_pfb_synth_create(None, N, P, g.ctypes.data, 0) == capi.INVALID_ARGUMENT
    for dtype in (capi.F64, capi.C64, capi.I16):
        assert ifft(dtype, N) == capi.INVALID_ARGUMENT
    for n in (0, 1):
        assert ifft(capi.C32, n) == capi.INVALID_ARGUMENT and ifft(capi.F32, n) == capi.INVALID_ARGUMENT
        assert bank(n, P, g) == capi.INVALID_ARGUMENT
    assert ifft(capi.C32, N, flags=2) == capi.INVALID_ARGUMENT and ifft(capi.C32, N, flags=3) == capi.INVALID_ARGUMENT
    assert ifft(capi.C32, N, window=12) == capi.INVALID_ARGUMENT and ifft(capi.C32, N, window=-1) == capi.INVALID_ARGUMENT
    assert bank(N, 0, g) == capi.INVALID_ARGUMENT
    assert bank(N, P, g, flags=2) == capi.INVALID_ARGUMENT
    for v in (np.inf, np.nan):
        bad = g.copy()
        bad[100] = v
        assert bank(N, P, bad) == capi.INVALID_ARGUMENT
        assert b"tap 100" in L.gr4hip_last_error()
    for n in (1000, 16384, 768):  # gr4hip_fft_plan kinds 2, 1 and 3
        assert ifft(capi.C32, n) == capi.UNSUPPORTED and ifft(capi.F32, n) == capi.UNSUPPORTED
        assert bank(n, 1, np.ones(n, np.float32)) == capi.UNSUPPORTED
    assert bank(N, 33, np.ones(N * 33, np.float32)) == capi.UNSUPPORTED
    # valid handles: only the device can be missing
    assert ifft(capi.C32, N) in (capi.OK, capi.NO_DEVICE) and ifft(capi.F32, N, 3, capi.IFFT_SCALE) in (capi.OK, capi.NO_DEVICE)
    assert bank(N, P, g, capi.IFFT_SCALE) in (capi.OK, capi.NO_DEVICE) and bank(N, P, None) in (capi.OK, capi.NO_DEVICE)
    # a NULL handle in every other entry point
    assert L.gr4hip_ifft_process(None, None, 4, None, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_pfb_synth_process(None, None, 4, None, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_pfb_synth_set_taps(None, g.ctypes.data, g.size) == capi.INVALID_ARGUMENT
    assert L.gr4hip_pfb_synth_reset(None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_ifft_destroy(None) == capi.OK and L.gr4hip_pfb_synth_destroy(None) == capi.OK


def test_host_program_holds(host_run):
    """the settings errors, the history bookkeeping, the reflected members and the plugin registration are EXPECTs of the program"""
    r, _ = host_run
    assert r.returncode == 0 and "ifft host: ok" in r.stdout and "FAIL" not in r.stdout
    for name in NAMES:
        assert f"plugin: {name} available" in r.stdout


@pytest.mark.parametrize("N", [8, 64])
def test_cpu_bodies_against_the_oracle(host_run, N):
    _, prefix = host_run
    tag = f"{prefix}.N{N}"
    X = _c(tag + ".in").reshape(-1, N)
    assert len(X) == 9
    w = PO.window("Hann", N)
    e = {
        "c2c": SO.rel(_c(tag + ".c2c").reshape(-1, N), SO.ifft_c2c(X, N)),
        "c2c Hann 1/N": SO.rel(_c(tag + ".c2c.hann.scaled").reshape(-1, N), SO.ifft_c2c(X, N) * w / N),
        "c2r": SO.rel(np.fromfile(tag + ".c2r", np.float32).reshape(-1, N), SO.ifft_c2r(X, N)),
    }
    for P in (1, 3):
        e[f"bank P {P}"] = SO.rel(_c(f"{tag}.P{P}.synth").reshape(-1, N), SO.synth(PO.design(N, P, "Hamming"), X, N, P))
    print(f"N {N}: host bodies " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= TOL


def test_history_kept_on_new_taps_and_cleared_on_a_new_shape(host_run):
    _, prefix = host_run
    N, P = 32, 4
    a, b, c = (_c(f"{prefix}.hist.{k}.in") for k in "abc")
    g2 = np.fromfile(prefix + ".hist.taps", np.float32)
    got = {k: _c(f"{prefix}.hist.{k}.synth").reshape(-1, N) for k in "abc"}
    assert SO.rel(got["a"], SO.synth(PO.design(N, P), a, N, P)) <= TOL
    kept = SO.synth(g2, b, N, P, history=a)
    assert SO.rel(got["b"], kept) <= TOL  # new taps on the old transformed frames
    assert SO.rel(got["b"][:P - 1], SO.synth(g2, b, N, P)[:P - 1]) > 1e-2  # ... which zeros in front would not give
    assert SO.rel(got["c"], SO.synth(PO.design(N, 2), c, N, 2)) <= TOL  # another taps_per_channel: zeros in front
    assert SO.rel(got["c"][:1], SO.synth(PO.design(N, 2), c, N, 2, history=b)[:1]) > 1e-2
