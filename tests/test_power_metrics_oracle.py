"""The numpy restatement of PowerMetrics (tests/power_metrics_oracle.py) against the reference QA's own criteria, and the reason the device keeps its states
in float64: on the QA's signal the reference's float arithmetic is off by 1e-4 ... 1e-2 of the output."""
import numpy as np
import pytest

import power_metrics_oracle as PM


@pytest.fixture(scope="module")
def qa():
    u, i = PM.qa_signals()  # qa_PowerEstimators.cpp:28-70: 10 kHz, 1 s, three phases, current delays 0.1 / 0.2 / 0.3 rad
    return PM.run(u, i, np.float64, decimate=200), PM.run(u, i, np.float32, decimate=200)


def test_float32_oracle_meets_the_reference_qa_criteria(qa):
    """qa_PowerEstimators.cpp:134-157 at the last output: P, Q, S within 10 % of S, the RMS values within 5 %"""
    r = qa[1]
    Sx = 230.0 * 10.0
    assert r["P"].shape == (3, 50)
    for ph, delay in enumerate((0.1, 0.2, 0.3)):
        assert abs(r["P"][ph, -1] - Sx * np.cos(delay)) <= 0.1 * Sx
        assert abs(r["Q"][ph, -1] - Sx * np.sin(delay)) <= 0.1 * Sx
        assert abs(r["S"][ph, -1] - Sx) <= 0.1 * Sx
        assert abs(r["U_rms"][ph, -1] - 230.0) <= 0.05 * 230.0
        assert abs(r["I_rms"][ph, -1] - 10.0) <= 0.05 * 10.0


def test_float32_states_are_visibly_noisy(qa):
    """maximum error over output rms on the second half of the outputs: the direct-form-II state of the 2 Hz high-pass is about 1e6 times the signal"""
    t64, t32 = qa
    h = t64["P"].shape[1] // 2
    for k in ("P", "S", "I_rms"):
        e = np.abs(t32[k] - t64[k])[:, h:].max(axis=1) / np.sqrt(np.mean(t64[k][:, h:] ** 2, axis=1))
        print(k, e)
        assert np.all((e > 1e-4) & (e < 1e-2)), (k, e)


def test_a_burst_then_silence_rings_negative():
    """a second-order Butterworth low-pass undershoots: the moving averages go below zero behind a burst, and the RMS values there are NaN (:113-114)"""
    n, on = 6000, 2000
    t = np.arange(n) / 1e4
    u = np.where(np.arange(n) < on, 100.0 * np.sqrt(2.0) * np.sin(2 * np.pi * 50.0 * t), 0.0).astype(np.float32)
    i = np.where(np.arange(n) < on, 5.0 * np.sqrt(2.0) * np.sin(2 * np.pi * 50.0 * t - 0.3), 0.0).astype(np.float32)
    r = PM.run(u, i, decimate=10)
    e = r["ema_u2"][0]
    neg = e < -1e-6 * np.abs(e).max()
    assert neg.sum() >= 1 and (r["ema_i2"][0] < 0).any()
    assert np.all(np.isnan(r["U_rms"][0][neg])) and np.all(np.isnan(r["S"][0][neg])) and np.all(np.isnan(r["Q"][0][neg]))
    assert np.all(np.isfinite(r["P"]))


def test_split_calls_continue_the_states():
    u, i = PM.qa_signals(3000, n_phases=1)
    whole = PM.Block(decimate=100).process(u[0], i[0])
    b = PM.Block(decimate=100)
    parts = [b.process(u[0, :1200], i[0, :1200]), b.process(u[0, 1200:], i[0, 1200:])]
    for k in PM.NAMES:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
