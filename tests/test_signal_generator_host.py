"""SignalGenerator on the host side, no device: what gr4hip_siggen_check accepts and refuses, the exported run and tile, the xoshiro256++ jump-ahead
(gr4hip_siggen_jump_host) against stepping and against its own composition, and the time table (gr4hip_siggen_time_host) against the oracle's."""
import ctypes as C
import math

import numpy as np
import pytest

import signal_generator_oracle as SG


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


def _params(**kw):
    from gnuradio4_amd import capi
    p = capi.SigGenParams(capi.F32, SG.SIN, 1000.0, 1.0, 1.0, 0.0, 0.0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_check_accepts_the_four_types_and_eleven_signals(L):
    from gnuradio4_amd import capi
    for dtype in (capi.F32, capi.F64, capi.C32, capi.I16):
        for t in range(11):
            assert L.gr4hip_siggen_check(C.byref(_params(dtype=dtype, signal_type=t, frequency=0.0, seed=2 ** 64 - 1))) == 0
    assert L.gr4hip_siggen_check(C.byref(_params(frequency=-5.0, amplitude=-1.0, offset=-3e38, phase=1e30, sample_rate=1e-30))) == 0
    assert L.gr4hip_siggen_run() == 16 and L.gr4hip_siggen_tile() % L.gr4hip_siggen_run() == 0


@pytest.mark.parametrize("kw", [dict(sample_rate=0.0), dict(sample_rate=-1.0), dict(sample_rate=math.nan), dict(sample_rate=math.inf), dict(frequency=math.nan),
                                dict(frequency=math.inf), dict(amplitude=-math.inf), dict(amplitude=math.nan), dict(offset=math.inf), dict(offset=math.nan),
                                dict(phase=math.nan), dict(phase=-math.inf), dict(signal_type=11), dict(signal_type=-1), dict(dtype=-1), dict(dtype=14), dict(dtype=99),
                                dict(dtype=10, sample_rate=1e-45)])
def test_check_refuses_before_device_work(L, kw):
    from gnuradio4_amd import capi
    assert L.gr4hip_siggen_check(C.byref(_params(**kw))) == capi.INVALID_ARGUMENT
    assert L.gr4hip_last_error()
    h = C.c_void_p()
    assert L.gr4hip_siggen_create(C.byref(h), C.byref(_params(**kw))) == capi.INVALID_ARGUMENT and not h.value


@pytest.mark.parametrize("dtype", [0, 1, 2, 3, 4, 6, 7, 11, 12, 13])
def test_other_registered_types_are_unsupported(L, dtype):
    from gnuradio4_amd import capi
    assert L.gr4hip_siggen_check(C.byref(_params(dtype=dtype))) == capi.UNSUPPORTED
    assert L.gr4hip_siggen_check(None) == capi.INVALID_ARGUMENT


def _jump(L, st, n):
    a, o = (C.c_ulonglong * 4)(*st), (C.c_ulonglong * 4)()
    assert L.gr4hip_siggen_jump_host(a, n, o) == 0
    return list(o)


def test_jump_is_stepping(L):
    st = SG.seed_state(12345)
    s, at = list(st), 0
    for n in (0, 1, 2, 255, 256, 257, 65_537, 1_000_007):
        while at < n:
            SG.step(s)
            at += 1
        assert _jump(L, st, n) == s, n


@pytest.mark.parametrize("a,b", [(2 ** 40 - 3, 2 ** 40 + 11), (2 ** 40 + 1, 5), (2 ** 63 - 1, 2 ** 63 - 7), (2 ** 63 + 12345, 2 ** 62 + 1)])
def test_jump_composes(L, a, b):
    st = SG.seed_state(987654321)
    assert _jump(L, _jump(L, st, a), b) == _jump(L, st, (a + b) % 2 ** 64) == _jump(L, _jump(L, st, b), a)  # (the period divides 2^256 - 1, not 2^64: a + b below 2^64 here)
    assert _jump(L, st, a) == SG.jump(st, a)


def _time(L, dtype, fs, n0, count):
    out = np.empty(count, np.float64)
    assert L.gr4hip_siggen_time_host(dtype, fs, n0, count, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return out


def test_time_host_is_the_oracles_table_at_every_boundary(L):
    from gnuradio4_amd import capi
    F, tick = np.float32, np.float32(1) / np.float32(1000)
    tab = SG.time_table(F, tick)
    for nb in [s[0] for s in tab if s[0] <= 1 << 25] + [1 << 25, 1 << 40]:
        lo = max(nb - 1000, 0)
        assert np.array_equal(_time(L, capi.C32, 1000.0, lo, 2001), SG.time_at(tab, np.arange(lo, lo + 2001))), nb
    tab = SG.time_table(np.float64, 1.0 / 1000.0, n_end=1 << 40)
    for nb in [s[0] for s in tab]:
        lo = max(nb - 1000, 0)
        for dtype in (capi.F32, capi.F64, capi.I16):
            assert np.array_equal(_time(L, dtype, 1000.0, lo, 2001), SG.time_at(tab, np.arange(lo, lo + 2001))), nb
    # far binades from the first samples on, and sequential addition itself
    for F, dtype, fs in ((np.float64, capi.F64, 3e9), (np.float32, capi.C32, 48000.0), (np.float32, capi.C32, 4.0)):
        tick = F(F(1) / F(np.float32(fs)))
        assert np.array_equal(_time(L, dtype, fs, 0, 300_001).astype(F), SG.sequential_time(F, tick, 0, 300_000)), fs
    assert L.gr4hip_siggen_time_host(capi.I32, 1000.0, 0, 0, None) == capi.UNSUPPORTED


def test_graph_program_host_checks_and_loud_failure_without_a_device():
    """gnuradio4_amd/host/tests/test_host_signal_generator.cpp: its host-side checks pass (params of the blocks, the refusal of a bad setting), and without a GPU
    the device-domain SignalGenerator reports ERROR -- exit code 3, never the host loop in its place"""
    import os
    import subprocess

    import oracle_lib as O
    import torch
    subprocess.check_call(["bash", os.path.join(O.ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_signal_generator.py::test_blocks_in_a_graph runs the program")
    r = subprocess.run([os.path.join(O.ROOT, "build", "host", "test_host_signal_generator"), "1000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "returned ERROR" in r.stderr
