"""CPU checks of the frequency estimators' restatement (tests/freq_est_oracle.py) and of the library's host-only entry points: the reference QA's acceptance
criteria (blocks/filter/test/qa_FrequencyEstimator.cpp:136-221), the time-domain identity, the biquad, gr4hip_freqest_geometry, and argument validation."""
import ctypes as C

import numpy as np
import pytest

import freq_est_oracle as FE

QA_TONES = [49.9, 50.0, 50.001, 50.002, 50.003, 50.004, 50.005, 50.006, 50.007, 50.008, 50.009, 50.01, 50.02, 50.03, 50.04, 50.05, 50.06, 50.07, 50.08, 50.09,
            50.1, 50.2, 50.3, 50.4, 50.5, 50.6, 50.7, 50.8, 50.9, 51.0]


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


def _qa(method, **kw):
    return FE.Params(method, sample_rate=1000.0, f_min=45.0, f_expected=50.0, f_max=55.0, **kw)


@pytest.mark.parametrize("chunk,n", [(1, 128), (10, 1280)])
def test_time_domain_meets_the_reference_qa(chunk, n):
    p = _qa(0, n_periods=3, chunk=chunk)
    for f in QA_TONES:
        x = FE.qa_signal(f, 1000.0, 0.01, n)
        last = n // chunk - 1
        out32, raw32, v32 = FE.td_ref32(p, x, outputs=[last])
        out, raw, valid, _ = FE.td_truth(p, x)
        assert v32[last] and valid[last]
        assert abs(raw32[last] - f) <= 0.03, (f, raw32[last])
        assert abs(out[-1] - f) <= 0.03, (f, out[-1])


@pytest.mark.parametrize("chunk,n", [(1, 4100), (4096, 40960)])
def test_frequency_domain_meets_the_reference_qa(chunk, n):
    p = _qa(1, min_fft_size=4096, chunk=chunk)
    assert FE.geometry(p)[0] == 4096
    for f in QA_TONES:
        x = FE.qa_signal(f, 1000.0, 0.01, n)
        last = n // chunk - 1
        _, raw32, v32 = FE.fd_ref32(p, x, outputs=[last])
        _, raw, valid, _ = FE.fd_truth(p, x, only=[last])
        assert v32[last] and valid[last]
        assert abs(raw32[last] - f) <= 1.0 and abs(raw[last] - f) <= 1.0, (f, raw32[last], raw[last])
        assert abs(raw32[last] - raw[last]) <= 1e-3 * f  # the float32 and float64 evaluations tell the same story


def test_time_domain_identity_on_a_clean_sinusoid():
    """y = sin(w n + phi): (y[n-1] + y[n+1])^2 / 2 = 2 cos^2(w) y^2, so C / B - 1 = cos 2w and f = fs / (4 pi) acos(cos 2w) = w fs / (2 pi)"""
    p = FE.Params(0)
    W, _, _ = FE.geometry(p)
    for f in (41.0, 50.0, 57.3, 120.0):
        w = 2 * np.pi * f / 1000.0
        y = np.sin(w * np.arange(2000) + 0.4)
        B, Cs = FE.td_sums64(p, y, W, np.arange(W - 1, 2000))
        assert np.max(np.abs(Cs / B - 1 - np.cos(2 * w))) < 1e-12
        assert np.allclose(1000.0 / (4 * np.pi) * np.arccos(Cs / B - 1), f, rtol=1e-9)


@pytest.mark.parametrize("fmax,fs", [(60.0, 1000.0), (55.0, 1000.0), (5e3, 48e3), (0.4, 1.0)])
def test_the_biquad_is_the_reference_single_section_design(L, fmax, fs):
    """designFilter<T, 0UZ>(LOWPASS, order 2, f_max, BESSEL) (FrequencyEstimator.hpp:77): one coefficient set, 3 + 3 taps, a[0] = 1; the library's
    gr4hip_iir_design (what the device handle is built from) gives the same one biquad"""
    p = FE.Params(0, sample_rate=fs, f_min=0.0, f_expected=fmax / 2, f_max=fmax)
    b, a = FE.biquad(p)
    assert b.shape == (3,) and a.shape == (3,) and a[0] == 1.0
    from gnuradio4_amd import capi
    q = capi.FilterParams()
    L.gr4hip_filter_params_default(C.byref(q))
    q.order, q.f_low, q.fs = 2, fmax, fs
    hb, ha, ns = (C.c_float * 6)(), (C.c_float * 6)(), C.c_size_t(0)
    assert L.gr4hip_iir_design(capi.LOWPASS, C.byref(q), capi.BESSEL, hb, ha, 2, C.byref(ns)) == 0 and ns.value == 1
    np.testing.assert_allclose(np.array(hb[:3], np.float32), b, rtol=2e-7, atol=0)  # (the two restatements agree to the last bit or one ulp)
    np.testing.assert_allclose(np.array(ha[:3], np.float32), a, rtol=2e-7, atol=0)
    # unit DC gain of a low-pass
    assert abs(float(np.sum(b.astype(np.float64)) / np.sum(a.astype(np.float64))) - 1) < 1e-5


def _params(L, method, **kw):
    from gnuradio4_amd import capi
    p = capi.FreqEstParams()
    assert L.gr4hip_freqest_params_default(method, C.byref(p)) == 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _geometry(L, method, **kw):
    w, a, b = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = L.gr4hip_freqest_geometry(method, C.byref(_params(L, method, **kw)), C.byref(w), C.byref(a), C.byref(b))
    return rc, (w.value, a.value, b.value)


def test_defaults_are_the_blocks_defaults(L):
    for m in (0, 1):
        p = _params(L, m)
        assert (p.sample_rate, p.f_min, p.f_expected, p.f_max, p.n_periods, p.min_fft_size, p.chunk) == (1000.0, 40.0, 50.0, 60.0, 4, 256, 1)
        assert p.epsilon == np.float32(1e-8)
    assert _geometry(L, 0) == (0, (100, 0, 0))
    assert _geometry(L, 1) == (0, (256, 10, 16))


SWEEP = [dict(sample_rate=fs, f_min=fmin, f_expected=fexp, f_max=fmax, n_periods=npd, min_fft_size=mfft)
         for fs in (1000.0, 48000.0, 3.0e4, 977.7)
         for (fmin, fexp, fmax) in ((40.0, 50.0, 60.0), (0.0, 50.0, 60.0), (45.0, 50.0, 0.4999), (55.0, 50.0, 45.0), (0.0, 13.3, 13.3), (10.0, 12.0, 10.2))
         for npd, mfft in ((4, 256), (1, 4), (7, 1000), (3, 4096))]


def test_geometry_matches_the_restatement(L):
    n = 0
    for s in SWEEP:
        fs = s["sample_rate"]
        s = dict(s)
        if s["f_max"] < 1:
            s["f_max"] = float(np.nextafter(np.float32(fs / 2), np.float32(0)))  # the largest f_max below fs/2
        for m in (0, 1):
            p = FE.Params(m, **s)
            want = FE.geometry(p)
            rc, got = _geometry(L, m, **p.kw())
            if rc != 0:
                assert rc == -103 and (want[0] > (1 << 20) or (m == 1 and want[2] - want[1] + 2 > 2048)), (m, s, rc, want)
                continue
            assert got == want, (m, s, got, want)
            n += 1
    assert n > 150
    # the empty search range (i_min >= i_max) is a geometry like any other
    p = FE.Params(1, f_min=55.0, f_expected=50.0, f_max=45.0)
    assert _geometry(L, 1, **p.kw())[1] == FE.geometry(p) and FE.geometry(p)[1] > FE.geometry(p)[2]


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("bad", [dict(f_min=-1.0), dict(f_max=500.0), dict(f_max=600.0), dict(f_expected=-1.0), dict(f_expected=500.0), dict(f_expected=0.0),
                                 dict(chunk=0), dict(sample_rate=0.0), dict(sample_rate=float("nan")), dict(f_min=float("inf"))])
def test_ill_formed_settings_are_invalid_arguments_without_a_gpu(L, method, bad):
    from gnuradio4_amd import capi
    p = _params(L, method, **bad)
    h = C.c_void_p()
    assert L.gr4hip_freqest_create(C.byref(h), method, C.byref(p)) == capi.INVALID_ARGUMENT and not h.value
    assert L.gr4hip_freqest_geometry(method, C.byref(p), None, None, None) == capi.INVALID_ARGUMENT


def test_settings_the_device_path_does_not_take(L):
    from gnuradio4_amd import capi
    h = C.c_void_p()
    for m, kw in ((0, dict(n_periods=0)),):
        assert L.gr4hip_freqest_create(C.byref(h), m, C.byref(_params(L, m, **kw))) == capi.INVALID_ARGUMENT
    for m, kw in ((0, dict(f_max=0.0)), (1, dict(f_max=-1.0)), (0, dict(f_min=0.0, f_expected=1e-3)), (1, dict(min_fft_size=1 << 21)),
                  (1, dict(sample_rate=1e6, f_min=1.0, f_expected=100.0, f_max=4e5, min_fft_size=1 << 16)), (1, dict(sample_rate=10.0, f_min=4.0, f_expected=4.0, f_max=4.9, min_fft_size=1))):
        assert L.gr4hip_freqest_create(C.byref(h), m, C.byref(_params(L, m, **kw))) == capi.UNSUPPORTED, (m, kw)
    assert L.gr4hip_freqest_create(C.byref(h), 2, C.byref(_params(L, 0))) == capi.INVALID_ARGUMENT
    assert L.gr4hip_freqest_create(None, 0, C.byref(_params(L, 0))) == capi.INVALID_ARGUMENT
