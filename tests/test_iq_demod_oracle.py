"""CPU checks of the IQDemodulator restatement (tests/iq_demod_oracle.py): the reference QA's acceptance criteria (blocks/filter/test/qa_FrequencyEstimator.cpp:
216-735) met by the float64 truth, truth's vectorised form against a plain per-sample loop, and how far the reference's own float32 loop sits from truth."""
import numpy as np
import pytest

import iq_demod_oracle as IQ


def _means(out, settle):
    return [float(np.mean(v[settle:])) for v in out[:3]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("freq,fs", [(100e3, 1e6), (5e6, 62.5e6)])
@pytest.mark.parametrize("unit", [0, 1])
def test_basic_extraction(dtype, freq, fs, unit):
    ref, resp = IQ.qa_signals(freq, fs, 0.8, 0.5, 0.1, 0.01, 1024 * 100, dtype)
    p = IQ.Params(dtype, sample_rate=fs, f_high_pass=100.0, f_low_pass=10000.0, phase_unit=unit, chunk=1024)
    amp, ph, fr = _means(IQ.truth(p, ref, resp), 20)
    assert abs(amp - 0.8) <= 0.05
    if unit == 1:
        assert abs(ph - 0.5 * 180 / np.pi) <= 3.0
    else:
        assert abs(ph - 0.5) <= 0.1
    assert abs(fr - freq) <= 0.05 * freq


def test_phase_inversion():
    n = 256 * 300
    t = np.arange(n).astype(np.float32)
    om = np.float32(2 * np.pi * 150e3 / 1e6)
    ref, resp = np.sin(om * t), np.sin(om * t + np.float32(0.3))
    kw = dict(sample_rate=1e6, f_high_pass=50.0, f_low_pass=15000.0, chunk=256)
    a = IQ.truth(IQ.Params(**kw), ref, resp)[1]
    b = IQ.truth(IQ.Params(invert_phase=True, **kw), ref, resp)[1]
    assert abs(np.mean(a[100:]) + np.mean(b[100:])) < 0.05
    assert np.array_equal(a, -b)


def test_settings_change_resets_filters():
    n = 256 * 50
    t = np.arange(n).astype(np.float32)
    om = np.float32(2 * np.pi * 100e3 / 1e6)
    ref, resp = np.sin(om * t), np.sin(om * t + np.float32(0.2))
    p = IQ.Params(sample_rate=1e6, f_high_pass=100.0, f_low_pass=10000.0, chunk=256)
    IQ.truth(p, ref, resp)
    out = IQ.truth(p.replace(f_low_pass=5000.0), ref, resp)  # re-initialised: a fresh block with the new cut-off
    assert all(np.isfinite(v[-1]) for v in out[:3])


def test_derivative_methods():
    ref, resp = IQ.qa_signals(100e3, 1e6, 0.8, 0.3, 0.0, 0.01, 512 * 100)
    for m in range(3):
        amp = IQ.truth(IQ.Params(sample_rate=1e6, f_high_pass=50.0, f_low_pass=20000.0, derivative_method=m, chunk=512), ref, resp)[0]
        assert np.isfinite(np.mean(amp[30:])) and np.mean(amp[30:]) > 0


def test_zero_input_gives_exact_zero():
    z = np.zeros(256 * 50, np.float32)
    for m in range(3):
        out = IQ.truth(IQ.Params(sample_rate=1e6, derivative_method=m, chunk=256), z, z)
        assert all(np.all(v == 0.0) for v in out[:3])


def test_dc_only_input_gives_finite_outputs():
    n = 256 * 100
    ref, resp = np.full(n, 0.5, np.float32), np.full(n, np.float32(0.5) * np.float32(0.8), np.float32)
    out = IQ.truth(IQ.Params(sample_rate=1e6, f_high_pass=100.0, f_low_pass=10000.0, chunk=256), ref, resp)
    assert all(np.all(np.isfinite(v[50:])) for v in out[:3])


def test_carrier_at_the_high_pass_cutoff():
    ref, resp = IQ.qa_signals(1000.0, 1e6, 0.8, 0.3, 0.0, 0.0, 1024 * 200)
    amp = IQ.truth(IQ.Params(sample_rate=1e6, f_high_pass=1000.0, f_low_pass=10000.0, chunk=1024), ref, resp)[0]
    assert abs(np.mean(amp[100:]) - 0.8) <= 0.15


def test_near_nyquist():
    ref, resp = IQ.qa_signals(200e3, 1e6, 0.9, 0.4, 0.0, 0.0, 512 * 200)
    amp, ph, fr = _means(IQ.truth(IQ.Params(sample_rate=1e6, f_high_pass=100.0, f_low_pass=50000.0, chunk=512), ref, resp), 50)
    assert abs(amp - 0.9) <= 0.05 and abs(ph - 0.4) <= 0.1 and abs(fr - 200e3) <= 0.1 * 200e3


@pytest.mark.parametrize("method", range(3))
def test_chirp_0p1_to_5_mhz(method):
    """the QA's 0.1-5 MHz sweep at 62.5 MHz, swept in 0.1 s instead of 0.5 s (the float64 restatement of 31 M samples would need gigabytes)"""
    fs, C = 62.5e6, 1024
    ref, resp, f = IQ.chirp(fs, 0.1e6, 5e6, 0.1, 0.85, 0.4, 0.01)
    amp, ph, fr, _ = IQ.truth(IQ.Params(sample_rate=fs, f_high_pass=1000.0, f_low_pass=10000.0, derivative_method=method, chunk=C), ref, resp)
    true_f = f[np.arange(len(amp)) * C]
    s = slice(500, None)
    assert abs(np.mean(amp[s]) - 0.85) <= 0.1 and amp[s].min() > 0.6 * 0.85 and amp[s].max() < 1.4 * 0.85
    assert abs(np.mean(ph[s]) - 0.4) <= 0.2
    err = np.abs(fr[s] - true_f[s])
    fc = (0.1e6 + 5e6) / 2
    assert np.mean(err) < 0.02 * fc and np.max(err) < 0.05 * fc


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", range(3))
def test_truth_equals_a_plain_float64_loop(dtype, method):
    ref, resp = IQ.qa_signals(1.3e6, 62.5e6, 0.7, 0.9, 0.2, 0.05, 3003, dtype)
    p = IQ.Params(dtype, f_high_pass=2e5, f_low_pass=3e6, derivative_method=method, phase_unit=1, chunk=7)
    a, b = IQ.truth(p, ref, resp), IQ.plain_loop(p, ref, resp)
    assert b[3]["decided"].all()
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_allclose(u, v, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("freq,fs,C", [(100e3, 1e6, 256), (5e6, 62.5e6, 1024)])
def test_reference_float32_loop_sits_near_truth(freq, fs, C):
    """the reference's own float32 arithmetic against the float64 truth on the basic case (measured about 1e-6 at 100 kHz / 1 MHz, C = 256)"""
    ref, resp = IQ.qa_signals(freq, fs, 0.8, 0.5, 0.1, 0.01, C * 40)
    p = IQ.Params(sample_rate=fs, f_high_pass=100.0, f_low_pass=10000.0, chunk=C)
    want = IQ.truth(p, ref, resp)
    got = IQ.ref32(p, ref, resp)
    s = slice(20, None)
    assert np.max(np.abs(got[0][s] - want[0][s]) / want[0][s]) <= 1e-4
    assert np.max(np.abs(got[1][s] - want[1][s])) <= 1e-4
    assert np.max(np.abs(got[2][s] - want[2][s]) / want[2][s]) <= 1e-4
