"""Host side of the cross-spectrum correlator (gr4hip_xcorr_*): symbols, every refusal before any device work, gr4hip_xcorr_pending, and the C++ host mirror
(gr::blocks::fft::CrossSpectrum<float>: its CPU body in a host-domain graph against the oracle's ordered definition bit for bit, the settings errors, the chunk
sizes, gr:sample_rate, the plugin registration).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cross_spectrum_oracle as XO
import oracle_lib as O

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_cross_spectrum")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
SYMBOLS = ["gr4hip_xcorr_create", "gr4hip_xcorr_reset", "gr4hip_xcorr_set_length", "gr4hip_xcorr_pending", "gr4hip_xcorr_process", "gr4hip_xcorr_destroy",
           "gr4hip_xcorr_leaf", "gr4hip_xcorr_coherence"]
HOOKS = ["gr4hip_internal_xcorr_set_path", "gr4hip_internal_xcorr_last_path"]


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    assert os.path.exists(BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_cross_spectrum.cpp and the plugin"
    prefix = str(tmp_path_factory.mktemp("xcorr") / "host")
    r = subprocess.run([BIN, "host", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r, prefix


def _create(L, n_streams, n_bins, n_integrate, flags=0):
    h = C.c_void_p()
    return L.gr4hip_xcorr_create(C.byref(h), n_streams, n_bins, n_integrate, flags), h


def test_symbols_exist_and_are_declared(L):
    from gnuradio4_amd import capi
    import gnuradio4_amd as G
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gr4hip.h")).read(), flags=re.S)
    raw = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in gr4hip.h"
        assert hasattr(raw, s) and s in capi.SIGNATURES
    for s in HOOKS:  # the test hooks are exported, not declared
        assert hasattr(raw, s) and s not in text and s not in capi.SIGNATURES
    assert hasattr(G, "CrossSpectrum") and "CrossSpectrum" in G.__all__
    for m in ("process_bulk", "reset", "set_length", "pending", "coherence", "baseline"):
        assert hasattr(G.CrossSpectrum, m)
    assert L.gr4hip_xcorr_leaf() == 64 == XO.LEAF
    assert L.gr4hip_abi_version() == 1


def test_create_refusals(L):
    from gnuradio4_amd import capi
    INV, UNS = capi.INVALID_ARGUMENT, capi.UNSUPPORTED
    assert L.gr4hip_xcorr_create(None, 2, 64, 4, 0) == INV
    for args in ((1, 64, 4, 0), (0, 64, 4, 0), (2, 1, 4, 0), (2, 0, 4, 0), (2, 64, 0, 0), (2, 64, 4, 2), (2, 64, 4, -1)):
        rc, h = _create(L, *args)
        assert rc == INV and not h.value, args
    # more than 32 streams, more than 2^20 bins, P n_bins above 2^24 (S = 32: P = 528, 2^24 / 528 = 31775.03)
    for args in ((33, 64, 4), (2, (1 << 20) + 1, 4), (32, 31776, 4), (6, 1 << 20, 4)):
        rc, h = _create(L, *args)
        assert rc == UNS and not h.value, args
    for args in ((32, 31775, 4, capi.XCORR_MEAN), (5, 1 << 20, 1, 0), (2, 2, 1 << 40, 0)):
        rc, h = _create(L, *args)
        assert rc == capi.OK and h.value, args
        L.gr4hip_xcorr_destroy(h)


def test_refusals_come_before_any_device_work(L):
    """every one of these returns its status with or without a device: the checks run on the host first, and a handle is host state until its first call"""
    from gnuradio4_amd import capi
    INV = capi.INVALID_ARGUMENT
    S, N, A = 3, 64, 4
    P = S * (S + 1) // 2
    rc, h = _create(L, S, N, A)
    assert rc == capi.OK
    n = C.c_size_t(777)
    frames = 8
    buf = np.zeros(2 * (S * frames * N + 2 * P * N) + 8, np.float32)  # (host memory: no call below gets as far as reading it)
    p = buf.ctypes.data + (-buf.ctypes.data) % 8
    stream_bytes = frames * N * 8
    ins = [p + s * stream_bytes for s in range(S)]
    out = p + S * stream_bytes
    arr = lambda v: (C.c_void_p * S)(*v)
    proc = L.gr4hip_xcorr_process
    assert proc(None, arr(ins), frames, out, C.byref(n), None) == INV
    assert proc(h, None, frames, out, C.byref(n), None) == INV
    assert proc(h, arr([ins[0], None, ins[2]]), frames, out, C.byref(n), None) == INV
    assert proc(h, arr(ins), frames, None, C.byref(n), None) == INV and b"completes 2" in L.gr4hip_last_error()  # 8 frames complete two integrations
    assert proc(h, arr(ins), frames, out, None, None) == INV
    assert proc(h, arr([ins[0], ins[1] + 4, ins[2]]), frames, out, C.byref(n), None) == INV  # not aligned to 8 bytes
    assert proc(h, arr(ins), frames, out + 4, C.byref(n), None) == INV
    assert proc(h, arr(ins), frames, ins[2] + 64, C.byref(n), None) == INV and b"overlaps" in L.gr4hip_last_error()  # the output inside an input
    assert proc(h, arr([ins[0], ins[1], out + 8]), frames, out, C.byref(n), None) == INV  # an input inside the output
    assert proc(h, arr(ins), (1 << 40) // N + 1, out, C.byref(n), None) == INV
    assert n.value == 777 and not buf.any()
    assert proc(h, arr([ins[0], ins[0], ins[0]]), 0, None, C.byref(n), None) == capi.OK and n.value == 0  # no frames: a no-op, with or without a device
    n.value = 777
    assert proc(h, None, 0, None, C.byref(n), None) == capi.OK and n.value == 0
    for f in (L.gr4hip_xcorr_reset, L.gr4hip_xcorr_destroy):
        assert f(None) in (capi.OK, INV)
    assert L.gr4hip_xcorr_set_length(None, 4) == INV and L.gr4hip_xcorr_set_length(h, 0) == INV
    assert L.gr4hip_xcorr_pending(None, 4, C.byref(n)) == INV and L.gr4hip_xcorr_pending(h, 4, None) == INV
    L.gr4hip_xcorr_destroy(h)
    # the stateless coherence call
    coh = L.gr4hip_xcorr_coherence
    vis, msc, h1 = p, out, out + N * 4 + 8 - (N * 4) % 8
    assert coh(None, S, N, 1, 1, 0, msc, h1, None) == INV
    assert coh(vis, S, N, 1, 1, 0, None, None, None) == INV
    assert coh(vis, 1, N, 1, 0, 0, msc, h1, None) == INV and coh(vis, S, 1, 1, 1, 0, msc, h1, None) == INV
    assert coh(vis, S, N, 1, S, 0, msc, h1, None) == INV and coh(vis, S, N, 1, 0, S, msc, h1, None) == INV
    assert coh(vis + 4, S, N, 1, 1, 0, msc, h1, None) == INV and coh(vis, S, N, 1, 1, 0, msc + 2, h1, None) == INV and coh(vis, S, N, 1, 1, 0, msc, h1 + 4, None) == INV
    assert coh(vis, S, N, 1, 1, 0, vis + 16, None, None) == INV and coh(vis, S, N, 1, 1, 0, None, vis + 16, None) == INV  # an output inside the input
    assert coh(vis, 33, N, 1, 1, 0, msc, h1, None) == capi.UNSUPPORTED
    assert coh(vis, S, N, 0, 1, 0, msc, h1, None) == capi.OK  # no matrices: a no-op
    assert not buf.any()


def test_pending_over_a_sequence_of_cuts(L):
    """pending is host arithmetic on the carried frame position: floor((pos + n) / A).  Without a device the position stays where create, reset and set_length
    put it (0); tests/test_gpu_cross_spectrum.py follows it through real calls."""
    from gnuradio4_amd import capi
    rc, h = _create(L, 4, 16, 65)
    assert rc == capi.OK
    n = C.c_size_t(0)
    for frames, want in ((0, 0), (1, 0), (64, 0), (65, 1), (129, 1), (130, 2), (65 * 1000 + 64, 1000)):
        assert L.gr4hip_xcorr_pending(h, frames, C.byref(n)) == capi.OK and n.value == want, frames
    assert L.gr4hip_xcorr_set_length(h, 5) == capi.OK
    for frames, want in ((4, 0), (5, 1), (14, 2)):
        assert L.gr4hip_xcorr_pending(h, frames, C.byref(n)) == capi.OK and n.value == want, frames
    assert L.gr4hip_xcorr_reset(h) == capi.OK and L.gr4hip_xcorr_pending(h, 5, C.byref(n)) == capi.OK and n.value == 1
    L.gr4hip_xcorr_destroy(h)


def test_host_program_holds(host_run):
    """the settings errors, the chunk sizes, gr:sample_rate scaled by P / n_integrate, the reflected members and the plugin registration are EXPECTs of the program"""
    r, _ = host_run
    assert r.returncode == 0 and "cross spectrum host: ok" in r.stdout and "FAIL" not in r.stdout
    assert "plugin: gr::blocks::fft::CrossSpectrum<float32> available" in r.stdout


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("S,N,A", [(2, 8, 1), (3, 16, 63), (5, 8, 65), (4, 8, 130)])
def test_cpu_body_is_the_definition_bit_for_bit(host_run, S, N, A, mean):
    _, prefix = host_run
    tag = f"{prefix}.S{S}.N{N}.A{A}.{'mean' if mean else 'sum'}"
    X = np.fromfile(tag + ".in", np.complex64).reshape(S, -1, N)
    got = np.fromfile(tag + ".out", np.complex64).reshape(-1, S * (S + 1) // 2, N)
    assert X.shape[1] == 2 * A + 3
    want = XO.cross_ordered(X, A, mean)
    assert got.shape == want.shape == ((2 * A + 3) // A, S * (S + 1) // 2, N) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
