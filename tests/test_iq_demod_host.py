"""IQDemodulator on the host side: gr4hip_iqdemod_check's validation (the same as create's, before any device work), the plugin's two registered types and the
IQDemodulatorFixed settings rule (gnuradio4_amd/host/tests/test_host_iq_demod.cpp), the loud failure of the device-only block without a GPU and in the host
domain, and, on a GPU, two sources -> IQDemodulator<float32> -> three sinks on compute_domain gpu:hip:0 against the oracle (tests/iq_demod_oracle.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import iq_demod_oracle as IQ
import oracle_lib as O

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_iq_demod")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    return BIN


def _params(L, **kw):
    from gnuradio4_amd import capi
    p = capi.IQDemodParams()
    assert L.gr4hip_iqdemod_params_default(C.byref(p)) == 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults_are_the_blocks(L):
    p = _params(L)
    assert (p.sample_rate, p.f_high_pass, p.f_low_pass, p.phase_unit, p.invert_phase, p.derivative_method, p.epsilon, p.chunk) == \
        (62.5e6, 100.0, 10000.0, 0, 0, 0, 1e-12, 1024)
    from gnuradio4_amd import capi
    for dt in (capi.F32, capi.F64):
        assert L.gr4hip_iqdemod_check(dt, C.byref(p)) == 0


@pytest.mark.parametrize("kw", [dict(f_high_pass=0.0), dict(f_high_pass=-1.0), dict(f_low_pass=0.0), dict(f_high_pass=1e4),  # f_hp >= f_lp
                                dict(f_low_pass=31.25e6), dict(sample_rate=1e6, f_low_pass=5e5), dict(sample_rate=0.0), dict(sample_rate=-62.5e6),
                                dict(sample_rate=math.nan), dict(f_high_pass=math.inf), dict(f_low_pass=math.nan), dict(epsilon=math.nan), dict(epsilon=math.inf),
                                dict(derivative_method=3), dict(derivative_method=-1), dict(phase_unit=2), dict(phase_unit=-1), dict(chunk=0)])
def test_every_rejection_before_device_work(L, kw):
    from gnuradio4_amd import capi
    p = _params(L, **kw)
    for dt in (capi.F32, capi.F64):
        assert L.gr4hip_iqdemod_check(dt, C.byref(p)) == capi.INVALID_ARGUMENT, kw
        h = C.c_void_p()
        assert L.gr4hip_iqdemod_create(C.byref(h), dt, C.byref(p)) == capi.INVALID_ARGUMENT and not h.value


def test_rejections_of_types_and_of_float_only_overflow(L):
    from gnuradio4_amd import capi
    p = _params(L)
    for dt in (capi.C32, capi.I16, capi.UF32):
        assert L.gr4hip_iqdemod_check(dt, C.byref(p)) == capi.INVALID_ARGUMENT
    p = _params(L, epsilon=1e300)  # finite as double, inf as float
    assert L.gr4hip_iqdemod_check(capi.F32, C.byref(p)) == capi.INVALID_ARGUMENT
    assert L.gr4hip_iqdemod_check(capi.F64, C.byref(p)) == 0
    assert L.gr4hip_iqdemod_check(capi.F32, None) == capi.INVALID_ARGUMENT


def test_nyquist_test_is_in_float(L):
    """settingsChanged compares f_low_pass >= sample_rate / 2.f in float (:461): a value just below fs / 2 in float passes"""
    from gnuradio4_amd import capi
    fs = float(np.float32(1e6))
    just_below = float(np.nextafter(np.float32(fs / 2), np.float32(0)))
    assert L.gr4hip_iqdemod_check(capi.F32, C.byref(_params(L, sample_rate=fs, f_low_pass=just_below))) == 0
    assert L.gr4hip_iqdemod_check(capi.F32, C.byref(_params(L, sample_rate=fs, f_low_pass=fs / 2))) == capi.INVALID_ARGUMENT


def test_plugin_makes_both_types_and_the_fixed_rule_holds(prog):
    r = subprocess.run([prog, PLUGIN, "host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed (compute_domain host)" in r.stdout


def _signals(tmp_path, n):
    ref, resp = IQ.qa_signals(1.5e6, 62.5e6, 0.8, 0.5, 0.1, 0.01, n)
    ref.tofile(tmp_path / "ref.f32")
    resp.tofile(tmp_path / "resp.f32")
    return ref, resp


def test_device_block_fails_loudly_without_gpu(prog, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _signals(tmp_path, 1024 * 16)
    for domain in ("gpu:hip:0", "host"):  # no host arithmetic: the graph fails, it does not produce numbers
        r = subprocess.run([prog, PLUGIN, domain, str(tmp_path / "ref.f32"), str(tmp_path / "resp.f32"), str(tmp_path / "y")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 3, (domain, r.returncode, r.stdout, r.stderr)


def test_host_domain_fails_loudly(prog, tmp_path):
    _signals(tmp_path, 1024 * 16)
    r = subprocess.run([prog, PLUGIN, "host", str(tmp_path / "ref.f32"), str(tmp_path / "resp.f32"), str(tmp_path / "y")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
    assert "device-only" in r.stderr


@pytest.mark.gpu
def test_device_graph_matches_the_oracle(prog, tmp_path):
    n = 1024 * 600
    ref, resp = _signals(tmp_path, n)
    r = subprocess.run([prog, PLUGIN, "gpu:hip:0", str(tmp_path / "ref.f32"), str(tmp_path / "resp.f32"), str(tmp_path / "y")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "invert_phase by settings after two chunks: amplitude unchanged, phase turned from the third chunk on" in r.stdout  # set_params on the live handle
    assert "phase alone: 1 output, the all-connected graph's bit for bit" in r.stdout  # two outputs without a reader: not copied to a port, the third unchanged
    got = [np.fromfile(tmp_path / f"y_{k}.f32", np.float32).astype(np.float64) for k in ("amp", "phase", "freq")]
    amp, ph, fr, m = IQ.truth(IQ.Params(derivative_method=1, chunk=1024), ref, resp)
    ok = m["decided"]
    assert len(got[0]) == n // 1024 and ok.mean() > 0.9
    assert np.max(np.where(ok, np.abs(got[0] - amp) / np.maximum(np.abs(amp), 1e-300), 0)) <= 1e-6
    assert np.max(np.where(ok, np.abs(got[1] - ph), 0)) <= 1e-6
    assert np.max(np.where(ok, np.abs(got[2] - fr) / np.maximum(np.abs(fr), 1e-300), 0)) <= 1e-6
