"""Host side of the polyphase filter bank (gr4hip_pfb_*): symbols, every create-time refusal before any device work, and the C++ host mirror
(gr::blocks::fft::PfbPowerSpectrum / PfbChannelizer: CPU bodies against the float64 oracle, settings errors, the history across settings changes, plugin
registration).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pfb_oracle as PO

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_pfb")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
SYMBOLS = ["gr4hip_pfb_design", "gr4hip_pfb_create", "gr4hip_pfb_set_taps", "gr4hip_pfb_reset", "gr4hip_pfb_process", "gr4hip_pfb_destroy"]
TOL = 1e-5  # the parity contract (include/gr4hip.h); the bodies are float32 sums and a float64 transform: measured 1e-7 .. 3e-7


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    assert os.path.exists(BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_pfb.cpp and the plugin"
    prefix = str(tmp_path_factory.mktemp("pfb") / "host")
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
    for name in ("PolyphaseFilterBank", "design_pfb"):
        assert hasattr(G, name) and name in G.__all__
    h = G.design_pfb(64, 4, "Hann")
    assert h.dtype == np.float32 and np.array_equal(h, PO.design(64, 4, "Hann"))


def test_create_refusals_come_before_any_device_work(L):
    """every one of these returns its status with or without a device: the checks run on the host first"""
    from gnuradio4_amd import capi
    h = PO.design(64, 4)

    def create(dtype, n, p, taps, flags=0):
        hd = C.c_void_p()
        rc = L.gr4hip_pfb_create(C.byref(hd), dtype, n, p, taps.ctypes.data if taps is not None else None, flags)
        if hd.value:
            L.gr4hip_pfb_destroy(hd)
        return rc

    assert L.gr4hip_pfb_create(None, capi.C32, 64, 4, h.ctypes.data, 0) == capi.INVALID_ARGUMENT
    assert create(capi.C32, 1, 4, h) == capi.INVALID_ARGUMENT
    assert create(capi.C32, 64, 0, h) == capi.INVALID_ARGUMENT
    assert create(capi.I16, 64, 4, h) == capi.INVALID_ARGUMENT
    assert create(capi.C32, 64, 4, h, flags=1) == capi.INVALID_ARGUMENT
    bad = h.copy()
    bad[100] = np.inf
    assert create(capi.C32, 64, 4, bad) == capi.INVALID_ARGUMENT
    assert b"tap 100" in L.gr4hip_last_error()
    assert create(capi.F32, 64, 4, h) == capi.UNSUPPORTED
    for n in (16384, 1000, 768):
        assert create(capi.C32, n, 1, np.ones(n, np.float32)) == capi.UNSUPPORTED
    assert create(capi.C32, 64, 33, np.ones(64 * 33, np.float32)) == capi.UNSUPPORTED
    assert create(capi.C32, 64, 4, h) in (capi.OK, capi.NO_DEVICE)  # a valid bank: only the device can be missing
    for f in (L.gr4hip_pfb_reset, L.gr4hip_pfb_destroy):
        assert f(None) in (capi.OK, capi.INVALID_ARGUMENT)
    assert L.gr4hip_pfb_process(None, None, 4, None, None, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_pfb_set_taps(None, h.ctypes.data, h.size) == capi.INVALID_ARGUMENT


def test_host_program_holds(host_run):
    """the settings errors (every bad setting throws, in both blocks), the history bookkeeping, the reflected members and the plugin registration are EXPECTs of the program"""
    r, _ = host_run
    assert r.returncode == 0 and "pfb host: ok" in r.stdout and "FAIL" not in r.stdout
    for name in ("gr::blocks::fft::PfbPowerSpectrum<complex<float32>>", "gr::blocks::fft::PfbChannelizer<complex<float32>>"):
        assert f"plugin: {name} available" in r.stdout


@pytest.mark.parametrize("N,P", [(8, 1), (16, 3), (64, 4), (256, 8)])
def test_cpu_bodies_against_the_oracle(host_run, N, P):
    _, prefix = host_run
    tag = f"{prefix}.N{N}.P{P}"
    x = _c(tag + ".in")
    assert len(x) == N * (P + 6)
    t = PO.pfb(PO.design(N, P, "Hamming"), x, N, P)
    e_s = PO.rel(_c(tag + ".spec").reshape(-1, N), t)
    e_m = PO.rel(np.fromfile(tag + ".mag2", np.float32).reshape(-1, N), np.abs(t) ** 2)
    print(f"N {N} P {P}: host body spectrum {e_s:.2e}, |X|^2 {e_m:.2e}")
    assert e_s <= TOL and e_m <= TOL


def test_history_kept_on_new_taps_and_cleared_on_a_new_shape(host_run):
    _, prefix = host_run
    N, P = 32, 4
    a, b, c = (_c(f"{prefix}.hist.{k}.in") for k in "abc")
    h2 = np.fromfile(prefix + ".hist.taps", np.float32)
    got = {k: _c(f"{prefix}.hist.{k}.spec").reshape(-1, N) for k in "abc"}
    assert PO.rel(got["a"], PO.pfb(PO.design(N, P), a, N, P)) <= TOL
    kept = PO.pfb(h2, b, N, P, history=a)
    assert PO.rel(got["b"], kept) <= TOL  # new taps on the old samples
    assert PO.rel(got["b"][:P - 1], PO.pfb(h2, b, N, P)[:P - 1]) > 1e-2  # ... which zeros in front would not give
    assert PO.rel(got["c"], PO.pfb(PO.design(N, 2), c, N, 2)) <= TOL  # another taps_per_channel: zeros in front
    assert PO.rel(got["c"][:1], PO.pfb(PO.design(N, 2), c, N, 2, history=b)[:1]) > 1e-2
