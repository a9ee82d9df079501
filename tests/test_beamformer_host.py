"""Host side of the beamformer (gr4hip_beamform_*): symbols, every refusal that needs no device, and the C++ host mirror (gr::blocks::fft::Beamformer<float>: its
CPU body in a host-domain graph against the oracle's ordered definition bit for bit, with per-bin weights and with the [B, S] short form, the settings errors,
the chunk sizes, gr:sample_rate, the plugin registration).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beamformer_oracle as BO
import oracle_lib as O

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_beamformer")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
SYMBOLS = ["gr4hip_beamform_create", "gr4hip_beamform_set_weights", "gr4hip_beamform_process", "gr4hip_beamform_power_integrate", "gr4hip_beamform_destroy"]
HOOKS = ["gr4hip_internal_beamform_set_path", "gr4hip_internal_beamform_last_path"]
FRAMES = 7


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    assert os.path.exists(BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_beamformer.cpp and the plugin"
    prefix = str(tmp_path_factory.mktemp("beamform") / "host")
    r = subprocess.run([BIN, "host", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r, prefix


def _create(L, S, B, N):
    h = C.c_void_p()
    return L.gr4hip_beamform_create(C.byref(h), S, B, N), h


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
    assert hasattr(G, "Beamformer") and "Beamformer" in G.__all__
    for m in ("set_weights", "process_bulk", "power_integrated", "delay_weights"):
        assert hasattr(G.Beamformer, m)
    assert L.gr4hip_abi_version() == 1


def test_the_definition_reads_the_same_everywhere():
    """the four fmaf lines of the definition, in the header, the document, the oracle and the host block"""
    squash = lambda s: re.sub(r"[\s*/]+", "", s)
    lines = ["re = fmaf( wr_s, xr_s, re);   re = fmaf(-wi_s, xi_s, re);", "im = fmaf( wi_s, xr_s, im);   im = fmaf( wr_s, xi_s, im);"]
    for path in ("include/gr4hip.h", "BEAMFORMER.md", "tests/beamformer_oracle.py", "gnuradio4_amd/host/include/gr4/blocks.hpp", "gnuradio4_amd/csrc/beamformer.hip"):
        text = squash(open(os.path.join(ROOT, path)).read())
        for line in lines:
            assert squash(line) in text, (path, line)


def test_create_refusals(L):
    from gnuradio4_amd import capi
    INV, UNS = capi.INVALID_ARGUMENT, capi.UNSUPPORTED
    assert L.gr4hip_beamform_create(None, 2, 1, 64) == INV
    for args in ((0, 1, 64), (2, 0, 64), (2, 1, 1), (2, 1, 0)):
        rc, h = _create(L, *args)
        assert rc == INV and not h.value, args
    # more than 32 streams or beams, more than 2^20 bins, B S n_bins above 2^24
    for args in ((33, 1, 64), (1, 33, 64), (2, 1, (1 << 20) + 1), (32, 32, (1 << 14) + 1), (17, 1, 1 << 20)):
        rc, h = _create(L, *args)
        assert rc == UNS and not h.value, args
    for args in ((32, 32, 1 << 14), (16, 1, 1 << 20), (1, 1, 2)):
        rc, h = _create(L, *args)
        assert rc == capi.OK and h.value, args
        L.gr4hip_beamform_destroy(h)


def test_refusals_come_before_any_device_work(L):
    """every one of these returns its status with or without a device: the checks run on the host first, and a handle is host state until its first set_weights"""
    from gnuradio4_amd import capi
    INV = capi.INVALID_ARGUMENT
    S, B, N, frames = 3, 2, 64, 4
    rc, h = _create(L, S, B, N)
    assert rc == capi.OK
    rc, si = C.c_int(0), C.c_void_p()
    assert L.gr4hip_specint_create(C.byref(si), B * N, 2, 0) == capi.OK
    buf = np.zeros(2 * (S + B) * frames * N + 8, np.float32)  # (host memory: no call below gets as far as reading it)
    p = buf.ctypes.data + (-buf.ctypes.data) % 8
    ins = (C.c_void_p * S)(*[p + s * frames * N * 8 for s in range(S)])
    outs = (C.c_void_p * B)(*[p + (S + b) * frames * N * 8 for b in range(B)])
    n = C.c_size_t(777)
    proc, integ = L.gr4hip_beamform_process, L.gr4hip_beamform_power_integrate
    assert proc(None, ins, frames, outs, N, None) == INV
    assert proc(h, ins, frames, outs, N, None) == INV and b"no weights" in L.gr4hip_last_error()  # process before any set_weights
    assert integ(None, si, ins, frames, outs[0], C.byref(n), None) == INV
    assert integ(h, None, ins, frames, outs[0], C.byref(n), None) == INV
    assert integ(h, si, ins, frames, outs[0], None, None) == INV
    assert integ(h, si, ins, frames, outs[0], C.byref(n), None) == INV and b"no weights" in L.gr4hip_last_error()
    assert L.gr4hip_beamform_set_weights(None, p, None) == INV and L.gr4hip_beamform_set_weights(h, None, None) == INV
    assert L.gr4hip_beamform_set_weights(h, p + 4, None) == INV  # not aligned to 8 bytes
    assert n.value == 777 and not buf.any()
    assert proc(h, ins, 0, outs, N, None) == capi.OK and proc(h, None, 0, None, N, None) == capi.OK  # no frames: a no-op, with or without a device
    assert integ(h, si, ins, 0, None, C.byref(n), None) == capi.OK and n.value == 0
    other = C.c_void_p()
    assert L.gr4hip_specint_create(C.byref(other), B * N + 1, 2, 0) == capi.OK
    n.value = 777
    assert integ(h, other, ins, 0, None, C.byref(n), None) == INV and n.value == 777  # an integrator of another width
    for handle in (si, other):
        L.gr4hip_specint_destroy(handle)
    assert L.gr4hip_beamform_destroy(h) == capi.OK and L.gr4hip_beamform_destroy(None) in (capi.OK, INV)


def test_delay_weights_are_the_float64_formula_rounded_once():
    import gnuradio4_amd as G
    tau = np.array([[0.0, 1e-6, 2.5e-6], [0.0, -1e-6, -2.5e-6]])
    f = np.arange(8) * 125e3
    w = G.Beamformer.delay_weights(tau, f)
    want = (np.exp(-2j * np.pi * f[None, None, :] * tau[:, :, None]) / 3).astype(np.complex64)
    assert w.dtype == np.complex64 and w.shape == (2, 3, 8) and np.array_equal(w.view(np.uint32), want.view(np.uint32))
    plain = np.exp(-2j * np.pi * f[None, None, :] * tau[:, :, None]).astype(np.complex64)
    assert np.array_equal(G.Beamformer.delay_weights(tau, f, normalise=False).view(np.uint32), plain.view(np.uint32))
    assert np.all(w[:, 0] == np.complex64(1 / 3))  # zero delay: a real weight in every bin


def test_host_program_holds(host_run):
    """the settings errors, the chunk sizes, gr:sample_rate scaled by n_beams, the reflected members, the C-ABI's refusals and the plugin registration are EXPECTs of
    the program"""
    r, _ = host_run
    assert r.returncode == 0 and "beamformer host: ok" in r.stdout and "FAIL" not in r.stdout
    assert "plugin: gr::blocks::fft::Beamformer<float32> available" in r.stdout


@pytest.mark.parametrize("form", ["full", "short"])
@pytest.mark.parametrize("S,B,N", [(1, 1, 8), (3, 5, 16), (9, 2, 8)])
def test_cpu_body_is_the_definition_bit_for_bit(host_run, S, B, N, form):
    _, prefix = host_run
    tag = f"{prefix}.S{S}.B{B}.N{N}.{form}"
    X = np.fromfile(tag + ".in", np.complex64).reshape(S, FRAMES, N)
    W = np.fromfile(tag + ".w", np.complex64).reshape((B, S, N) if form == "full" else (B, S))
    got = np.fromfile(tag + ".out", np.complex64).reshape(FRAMES, B, N)
    want = BO.beams_ordered(W, X).transpose(1, 0, 2)  # the block writes frames [f][b][c]
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
