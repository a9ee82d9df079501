"""Host side of the spectrum integrator (gr4hip_specint_*, gr4hip_fft_mag2_integrate, gr4hip_pfb_power_integrate): symbols, every refusal before any device work,
gr4hip_specint_pending, and the C++ host mirror (gr::blocks::fft::SpectrumIntegrator<float>: its CPU body in a host-domain graph against the oracle's ordered sums
bit for bit, the settings errors, gr:sample_rate, the plugin registration).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import spectrum_integrator_oracle as SO

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_spectrum_integrator")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
SYMBOLS = ["gr4hip_specint_create", "gr4hip_specint_reset", "gr4hip_specint_set_length", "gr4hip_specint_pending", "gr4hip_specint_process", "gr4hip_specint_destroy",
           "gr4hip_specint_leaf", "gr4hip_fft_mag2_integrate", "gr4hip_pfb_power_integrate"]


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    assert os.path.exists(BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_spectrum_integrator.cpp and the plugin"
    prefix = str(tmp_path_factory.mktemp("specint") / "host")
    r = subprocess.run([BIN, "host", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r, prefix


def _create(L, n_bins, n_integrate, flags=0):
    h = C.c_void_p()
    return L.gr4hip_specint_create(C.byref(h), n_bins, n_integrate, flags), h


def test_symbols_exist_and_are_declared(L):
    from gnuradio4_amd import capi
    import gnuradio4_amd as G
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gr4hip.h")).read(), flags=re.S)
    raw = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in gr4hip.h"
        assert hasattr(raw, s) and s in capi.SIGNATURES
    assert hasattr(raw, "gr4hip_internal_specint_last_path") and "gr4hip_internal_specint_last_path" not in text  # the test hook is exported, not declared
    assert hasattr(G, "SpectrumIntegrator") and "SpectrumIntegrator" in G.__all__
    assert hasattr(G.FFT, "power_integrated") and hasattr(G.PolyphaseFilterBank, "power_integrated")
    assert L.gr4hip_specint_leaf() == 32 == SO.LEAF


def test_refusals_come_before_any_device_work(L):
    """every one of these returns its status with or without a device: the checks run on the host first, and a handle is host state until its first call"""
    from gnuradio4_amd import capi
    INV = capi.INVALID_ARGUMENT
    assert L.gr4hip_specint_create(None, 64, 4, 0) == INV
    for args in ((1, 4, 0), (0, 4, 0), (64, 0, 0), (64, 4, 2), (64, 4, -1)):
        rc, h = _create(L, *args)
        assert rc == INV and not h.value, args
    rc, h = _create(L, (1 << 20) + 1, 4)
    assert rc == capi.UNSUPPORTED and not h.value
    rc, big = _create(L, 1 << 20, 4, capi.SPECINT_MEAN)
    assert rc == capi.OK and big.value
    L.gr4hip_specint_destroy(big)
    rc, h = _create(L, 64, 4)
    assert rc == capi.OK
    n = C.c_size_t(777)
    buf = np.zeros(64 * 16 + 4, np.float32)
    p = buf.ctypes.data  # (host memory: no call below gets as far as reading it)
    proc = L.gr4hip_specint_process
    assert proc(None, p, 8, p + 4096, C.byref(n), None) == INV
    assert proc(h, None, 8, p + 4096, C.byref(n), None) == INV
    assert proc(h, p, 8, None, C.byref(n), None) == INV and b"completes 2" in L.gr4hip_last_error()  # 8 frames complete two integrations
    assert proc(h, p, 8, p + 4096, None, None) == INV
    assert proc(h, p + 2, 8, p + 4096, C.byref(n), None) == INV  # not aligned to 4 bytes
    assert proc(h, p, 8, p + 4096 + 2, C.byref(n), None) == INV
    assert proc(h, p, 8, p + 64 * 4, C.byref(n), None) == INV and b"overlaps" in L.gr4hip_last_error()  # the output inside the input
    assert proc(h, p + 256, 8, p, C.byref(n), None) == INV  # the output's end inside the input
    assert proc(h, p, (1 << 40) // 64 + 1, p, C.byref(n), None) == INV
    assert n.value == 777
    assert proc(h, None, 0, None, C.byref(n), None) == capi.OK and n.value == 0  # no frames: a no-op, with or without a device
    for f in (L.gr4hip_specint_reset, L.gr4hip_specint_destroy):
        assert f(None) in (capi.OK, INV)
    assert L.gr4hip_specint_set_length(None, 4) == INV and L.gr4hip_specint_set_length(h, 0) == INV
    assert L.gr4hip_specint_pending(None, 4, C.byref(n)) == INV and L.gr4hip_specint_pending(h, 4, None) == INV
    # the fused entries: NULL handles on either side
    n.value = 777
    for entry in (L.gr4hip_fft_mag2_integrate, L.gr4hip_pfb_power_integrate):
        assert entry(None, h, p, 8, p + 4096, C.byref(n), None) == INV
    assert n.value == 777
    L.gr4hip_specint_destroy(h)


def test_pending_over_a_sequence_of_cuts(L):
    """pending is host arithmetic on the carried frame position: floor((pos + n) / A).  Without a device the position stays where create, reset and set_length
    put it (0); tests/test_gpu_spectrum_integrator.py follows it through real calls."""
    from gnuradio4_amd import capi
    rc, h = _create(L, 16, 33)
    assert rc == capi.OK
    n = C.c_size_t(0)
    for frames, want in ((0, 0), (1, 0), (32, 0), (33, 1), (65, 1), (66, 2), (33 * 1000 + 32, 1000)):
        assert L.gr4hip_specint_pending(h, frames, C.byref(n)) == capi.OK and n.value == want, frames
    assert L.gr4hip_specint_set_length(h, 5) == capi.OK
    for frames, want in ((4, 0), (5, 1), (14, 2)):
        assert L.gr4hip_specint_pending(h, frames, C.byref(n)) == capi.OK and n.value == want, frames
    assert L.gr4hip_specint_reset(h) == capi.OK and L.gr4hip_specint_pending(h, 5, C.byref(n)) == capi.OK and n.value == 1
    L.gr4hip_specint_destroy(h)


def test_host_program_holds(host_run):
    """the settings errors, the chunk sizes, gr:sample_rate divided by n_integrate, the reflected members and the plugin registration are EXPECTs of the program"""
    r, _ = host_run
    assert r.returncode == 0 and "spectrum integrator host: ok" in r.stdout and "FAIL" not in r.stdout
    assert "plugin: gr::blocks::fft::SpectrumIntegrator<float32> available" in r.stdout


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("N,A", [(8, 1), (16, 31), (32, 33), (64, 67), (16, 32)])
def test_cpu_body_is_the_definition_bit_for_bit(host_run, N, A, mean):
    _, prefix = host_run
    tag = f"{prefix}.N{N}.A{A}.{'mean' if mean else 'sum'}"
    m = np.fromfile(tag + ".in", np.float32).reshape(-1, N)
    got = np.fromfile(tag + ".out", np.float32).reshape(-1, N)
    assert len(m) == 2 * A + 3
    want = SO.integrate_ordered(m, A, mean)
    assert got.shape == want.shape == ((2 * A + 3) // A, N) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
