"""The CPU oracle pinned against the reference's own golden vectors / known-answer tests
and against the reference itself (digests of what oracle/_ref/libgr4ref.so, built from the reference's rng headers, computes)."""
import ctypes as C
import os
import math

import numpy as np
import pytest

import oracle_lib as O


# ------------------------------------------------------------------ rng (a15)
def test_xoshiro_seed0_known_answer(golden):
    g = golden["xoshiro_seed0_first5"]
    draws = O.xoshiro_draws(g["seed"], 5)
    assert [f"{int(d):016x}" for d in draws] == g["draws_hex"]


def test_rng_bit_exact_vs_reference_build():
    """tests/golden/rng_reference.json: SHA-256 of what the reference build (oracle/_ref, the reference's own rng code) draws and fills for these seeds
    and lengths, written by tests/golden/make_rng_fixture.py"""
    import hashlib
    import json
    ref = json.load(open(os.path.join(O.ROOT, "tests", "golden", "rng_reference.json")))
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    for seed in (0, 1, 42, 123456789):
        assert sha(O.xoshiro_draws(seed, 1000).astype(np.uint64)) == ref[f"draws_{seed}_1000"], seed
        for n in (1, 2, 7, 4096, 4097):
            assert sha(O.gauss_f32(seed, n, 1.5, 0.25).astype(np.float32)) == ref[f"gauss_f32_{seed}_{n}"], (seed, n)
            assert sha(O.gauss_c32(seed, n).astype(np.complex64)) == ref[f"gauss_c32_{seed}_{n}"], (seed, n)


def test_gauss_golden_fixture():
    """fixture generated from oracle/_ref (the reference's own code) by tests/golden/make_rng_fixture.py"""
    import os
    fx = np.load(os.path.join(O.ROOT, "tests", "golden", "rng_seed42.npz"))
    assert np.array_equal(fx["gauss_f32"].view(np.uint32), O.gauss_f32(42, 256).view(np.uint32))
    assert np.array_equal(fx["gauss_c32"].view(np.uint32), O.gauss_c32(42, 256).view(np.uint32))
    assert np.array_equal(fx["draws"], O.xoshiro_draws(42, 64))


def test_complex_noise_unit_power():
    x = O.gauss_c32(42, 200000)
    assert abs(np.mean(np.abs(x) ** 2) - 1.0) < 0.02


# ------------------------------------------------------------------ windows (a10)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_window_n8_golden(golden, dtype):
    g = golden["window_n8"]
    for wid, name in enumerate(O.WINDOWS):
        w = O.window(wid, 8, dtype)
        np.testing.assert_allclose(w, np.array(g[name]), rtol=2e-6, atol=2e-7, err_msg=name)
        assert len(O.window(wid, 0, dtype)) == 0  # zero-length windows (qa_algorithm_fourier.cpp:182-194)


def test_window_symmetry_and_size1():
    for wid in range(2, 10):
        w = O.window(wid, 1025, np.float64)
        np.testing.assert_allclose(w, w[::-1], atol=1e-12)


# ------------------------------------------------------------------ unwrap / magnitude / phase (a9)
def test_unwrap_golden(golden):
    g = golden["unwrap"]
    ph = np.array(g["phase"], np.float64)
    O.lib().gr4o_unwrap_f64(ph.ctypes.data, len(ph))
    np.testing.assert_allclose(ph, np.array(g["expected"]), atol=1e-7)
    np.testing.assert_allclose(ph, np.unwrap(np.array(g["phase"])), atol=1e-12)


def test_magnitude_shift_matches_definition():
    rng = np.random.default_rng(0)
    sp = (rng.standard_normal(64) + 1j * rng.standard_normal(64)).astype(np.complex128)
    m = O.magnitude(sp, shift=True)
    np.testing.assert_allclose(m, np.fft.fftshift(np.abs(sp) * 2 / 64), rtol=1e-14)
    mh = O.magnitude(sp, half=True, shift=True)  # half spectrum is never rotated (fft_common.hpp:48)
    np.testing.assert_allclose(mh, (np.abs(sp) * 2 / 64)[:32], rtol=1e-14)
    db = O.magnitude(np.zeros(8, np.complex64), in_db=True)
    assert np.all(db == np.finfo(np.float32).min)  # lowest() for log of zero (fft_common.hpp:41-43)
    p = O.phase(sp, in_deg=True, shift=True)
    np.testing.assert_allclose(p, np.fft.fftshift(np.degrees(np.angle(sp))), atol=1e-10)


# ------------------------------------------------------------------ FFT (a8)
def test_dft64_vs_numpy():
    rng = np.random.default_rng(1)
    for N in (1, 2, 16, 48, 60, 100, 1024, 8192):
        x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        np.testing.assert_allclose(O.dft64(x), np.fft.fft(x), atol=1e-9 * max(1, N))


def test_fft_n16_patterns(golden):
    g = golden["fft_n16_patterns"]
    for case in g["cases"]:
        if case.get("iota"):
            x = np.arange(1, 17, dtype=np.complex64)
        elif case.get("alternating"):
            x = (np.arange(16) % 2).astype(np.complex64)
        else:
            x = np.full(16, complex(*case["fill"]), np.complex64)
        for spec in (O.fft32(x), O.dft64(x)):
            mag = O.magnitude(np.ascontiguousarray(spec))
            assert int(np.argmax(mag)) == case["peak_index"]
            assert abs(mag.max() - case["peak_amplitude"]) < g["tolerance"] * 10
            assert abs(spec[0].real - case["fft0"][0]) < 1e-4 and abs(spec[0].imag - case["fft0"][1]) < 1e-4


def test_fft_sine_cases(golden):
    g = golden["fft_sine_cases"]
    for c in g["cases"]:
        N, fs, f, A = c["N"], c["sample_rate"], c["frequency"], c["amplitude"]
        t = np.arange(N) / fs
        x = (A * np.sin(2 * np.pi * f * t)).astype(np.complex64)
        for spec in (O.fft32(x), O.dft64(x)):
            mag = O.magnitude(np.ascontiguousarray(spec))
            k = int(np.argmax(mag[: N // 2]))
            assert abs(mag[k] - A) < 1e-4 * max(1, A)
            assert abs(k * fs / N - f) < g["tolerance"]


def test_fft32_edge_cases(golden):
    g = golden["simdfft_edge_cases"]
    for N in g["dc"]["sizes"]:
        sp = O.fft32(np.full(N, g["dc"]["value"], np.complex64))
        assert abs(sp[0].real - 1.5 * N) <= 1e-4 * N and np.all(np.abs(sp[1:]) <= 1e-4 * N)
    for N in g["nyquist"]["sizes"]:
        x = np.where(np.arange(N) % 2 == 0, 1.0, -1.0).astype(np.complex64)
        assert abs(O.fft32(x)[N // 2]) > 0.9 * N
    rng = np.random.default_rng(123)
    for N in g["linearity"]["sizes"]:
        x = (rng.uniform(-1, 1, N) + 1j * rng.uniform(-1, 1, N)).astype(np.complex64)
        y = (rng.uniform(-1, 1, N) + 1j * rng.uniform(-1, 1, N)).astype(np.complex64)
        err = np.max(np.abs(O.fft32(x + y) - (O.fft32(x) + O.fft32(y))))
        assert err < g["linearity"]["tolerance_times_N"] * N
        # forward/backward round trip within 1e-5*N (qa_SimdFFT.cpp:122-185): inverse via conjugation
        back = np.conj(O.fft32(np.conj(O.fft32(x)))) / N
        assert np.max(np.abs(back - x)) <= g["roundtrip_tolerance_times_N"] * N


def test_fft32_close_to_truth_8192():
    x = O.signal_c32(42, 8192)
    t = O.dft64(x)
    e = np.max(np.abs(O.fft32(x) - t)) / np.sqrt(np.mean(np.abs(t) ** 2))
    assert e < 1e-5


# ------------------------------------------------------------------ FIR / IIR (a1-a4)
def _settling(resp, thr=0.02):
    final = resp[-1]
    idx = 0
    for i, v in enumerate(resp):
        if abs(v - final) > thr * abs(final):
            idx = i + 1
    return idx


def test_fir_boxcar_step(golden):
    g = golden["fir_iir_step"]
    b = np.full(g["boxcar_taps"], g["boxcar_value"], np.float32)
    x = np.ones(g["n_steps"], np.float32)
    x[0] = 0
    y, _ = O.fir(b, x)
    assert y[0] == 0.0
    assert _settling(y) == g["fir_settling"]
    np.testing.assert_allclose(y[:6], [0, .1, .2, .3, .4, .5], atol=1e-7)


def test_fir_reference_harness_values():
    # box-car {0.25}*4 via the reference's HistoryBuffer+transform_reduce on 1,2,3,4,5,6 gives
    # 0.25,0.75,1.5,2.5,3.5,4.5 (probed against the reference header in the authoring container)
    y, _ = O.fir(np.full(4, 0.25, np.float32), np.arange(1, 7, dtype=np.float32))
    np.testing.assert_allclose(y, [0.25, 0.75, 1.5, 2.5, 3.5, 4.5])


def test_iir_forms_agree(golden):
    g = golden["fir_iir_step"]
    x = np.ones(g["n_steps"], np.float32)
    x[0] = 0
    outs = []
    for form in range(4):
        for f64 in (True, False):
            sec = O.make_sections([(g["biquad_b"], g["biquad_a"])])
            outs.append(O.iir_cascade(sec, x, form, f64).astype(np.float64))
    for o in outs[1:]:
        np.testing.assert_allclose(o, outs[0], atol=g["forms_tolerance"])
    sec = O.make_sections([(g["iir1_b"], g["iir1_a"])])
    r = O.iir_cascade(sec, x, O.DF_I)
    assert r[0] == 0.0 and _settling(r) <= g["iir1_settling"] + 1
    # against scipy's independent lfilter
    from scipy.signal import lfilter
    np.testing.assert_allclose(outs[0], lfilter(g["biquad_b"], g["biquad_a"], x.astype(np.float64)), atol=1e-12)


def test_fir_chunked_history_equals_one_shot():
    rng = np.random.default_rng(5)
    b = rng.standard_normal(37).astype(np.float32)
    x = (rng.standard_normal(1000) + 1j * rng.standard_normal(1000)).astype(np.complex64)
    full, _ = O.fir(b, x)
    hist, parts = None, []
    for lo, hi in ((0, 1), (1, 10), (10, 500), (500, 1000)):
        y, hist = O.fir(b, x[lo:hi], hist)
        parts.append(y)
    np.testing.assert_array_equal(np.concatenate(parts), full)
    from scipy.signal import lfilter
    np.testing.assert_allclose(full, lfilter(b.astype(np.float64), [1.0], x.astype(np.complex128)), atol=1e-12)


def test_decimating_filter_phase0():
    rng = np.random.default_rng(6)
    b = rng.standard_normal(64).astype(np.float32)
    x = rng.standard_normal(800).astype(np.float32)
    full, _ = O.fir(b, x)
    y, _ = O.fir_decim(b, x, 8)
    np.testing.assert_array_equal(y, full[::8])


def test_decimator(golden):
    g = golden["decimator"]
    x = np.arange(g["n_in"], dtype=np.int32)
    out = np.empty(g["n_out"], np.int32)
    n = O.lib().gr4o_decimate_bytes(x.ctypes.data, out.ctypes.data, len(x), 4, g["decim"])
    assert n == g["n_out"] and np.array_equal(out, x[:: g["decim"]])


# ------------------------------------------------------------------ design (a5)
def test_fir_design_tapcount_and_gain(golden):
    g = golden["fir_design_tapcount"]
    p = O.filter_params(order=g["order"], fLow=g["f_low"], fs=g["fs"])
    for is_float in (True, False):
        taps = O.fir_design(O.LOWPASS, p, 2, is_float)
        assert len(taps) == g["expected_taps"]
        assert abs(taps.sum() - 1.0) < 1e-5  # DC gain normalised (FilterTool.hpp:415-423)
        np.testing.assert_allclose(taps, taps[::-1], atol=1e-7)


@pytest.mark.parametrize("is_float", [True, False])
@pytest.mark.parametrize("ftype", ["FIR", "IIR"])
def test_basic_filter_lowpass_bands(golden, ftype, is_float):
    g = golden["basic_filter_lowpass"]
    fs, n = g["sample_rate"], g["num_samples"]
    p = O.filter_params(order=g["filter_order"], fLow=g["f_low"], fs=fs)
    for f_hz, check in ((g["pass_hz"], lambda m: m >= g["pass_min"]), (g["stop_hz"], lambda m: m <= g["stop_max"])):
        x = np.sin(2 * np.pi * f_hz / fs * np.arange(1, 2 * n + 1)).astype(np.float32)
        if ftype == "FIR":
            taps = O.fir_design(O.LOWPASS, p, 2, is_float).astype(np.float32)
            y, _ = O.fir(taps, x)
        else:
            sec = O.make_sections(O.iir_design(O.LOWPASS, p, O.CHEBYSHEV1, is_float))
            y = O.iir_cascade(sec, x, O.DF_II, f64=not is_float)
        assert check(np.max(np.abs(y[n:]))), (ftype, f_hz)
        yd = y[::g["decimation"]]  # BasicDecimatingFilter keeps i % decimate == 0
        assert check(np.max(np.abs(yd[n // g["decimation"]:])))


def test_iir_design_structure():
    # float -> biquads, all-pole low-pass sections b = {g,0,0}; double -> 4th-order sections
    p = O.filter_params(order=8, fLow=0.05, fs=1.0)
    secs = O.iir_design(O.LOWPASS, p, O.BUTTERWORTH, True)
    assert len(secs) == 4
    for b, a in secs:
        assert len(b) == 3 and len(a) == 3 and a[0] == 1.0 and b[1] == 0 and b[2] == 0
        assert abs(sum(b) / sum(a) - 1.0) < 1e-5  # per-section DC gain 1
    secs64 = O.iir_design(O.LOWPASS, p, O.BUTTERWORTH, False)
    assert len(secs64) == 2 and len(secs64[0][1]) == 5


def test_iir_digital_vs_analog_reference_grid():
    """Restates the reference's own design check (algorithm/test/qa_FilterTool.cpp:181-248): fLow 1, fHigh 10,
    fs 1000, attenuation 50 dB, orders 1..5, biquad sections vs analog prototype within 0.01 (x10 relax cases)."""
    freqs = np.concatenate([np.arange(0.1, 0.9001, 0.01), np.arange(1.0, 9.0001, 0.1), np.arange(10.0, 90.001, 1.0), np.arange(100.0, 490.001, 10.0)])
    fs, tol = 1000.0, 0.01
    for design in (O.BUTTERWORTH, O.BESSEL, O.CHEBYSHEV1, O.CHEBYSHEV2):
        for resp in (O.LOWPASS, O.HIGHPASS, O.BANDPASS, O.BANDSTOP):
            for order in range(3 if design == O.CHEBYSHEV2 else 1, 6):
                p = O.filter_params(order=order, fLow=1.0, fHigh=10.0, attenuationDb=50, fs=fs)
                sec = O.make_sections(O.iir_design(resp, p, design, is_float=True))  # biquads (maxSectionSize 2)
                dig = lambda f: float(np.prod([O.lib().gr4o_section_response(C.byref(s), f / fs) for s in sec]))
                if resp in (O.LOWPASS, O.BANDSTOP):
                    assert abs(dig(0.0) - 1.0) < tol
                relax = 10 if (design == O.BESSEL or order <= 1 or (design == O.CHEBYSHEV1 and resp == O.HIGHPASS)
                               or (design == O.CHEBYSHEV2 and resp == O.BANDSTOP)) else 1
                for f in freqs[::7]:
                    ref = O.lib().gr4o_analog_response(resp, C.byref(p), design, float(f))
                    if ref > 0.01:
                        assert abs(dig(float(f)) - ref) <= relax * tol * 1.5, (design, resp, order, f, ref, dig(float(f)))


def test_all_design_variants_run():
    for resp in range(4):
        for design in range(4):
            p = O.filter_params(order=4, fLow=100.0, fHigh=200.0, fs=1000.0)
            secs = O.iir_design(resp, p, design, True)
            assert len(secs) >= 2
            x = np.zeros(4000, np.float32)
            x[0] = 1
            y = O.iir_cascade(O.make_sections(secs), x)
            assert np.all(np.isfinite(y)) and abs(y[-1]) < 1e-3  # stable
        for win in (2, 3, 11):
            taps = O.fir_design(resp, p, win, True)
            assert len(taps) % 2 == 1 and np.all(np.isfinite(taps))


# ------------------------------------------------------------------ math / rotator (a11-a13)
_OPS = {"Add": O.ADD, "Subtract": O.SUB, "Multiply": O.MUL, "Divide": O.DIV}


def _cast(vals, dt):
    if np.issubdtype(dt, np.integer):
        return np.array([int(v) for v in vals]).astype(dt)  # T(4.2) truncates like the C++ literal conversion
    return np.array(vals).astype(dt)


@pytest.mark.parametrize("dtype_id", range(12))
def test_math_nary_golden(golden, dtype_id):
    dt = O.NP_DTYPES[dtype_id]
    for name, op in _OPS.items():
        for case in golden["math_nary"][name]:
            ins = [_cast(v, dt) for v in case["inputs"]]
            if np.issubdtype(dt, np.integer):
                exp = ins[0].copy()  # integer types: expected = op applied to the truncated operands
                for b in ins[1:]:
                    exp = {O.ADD: exp + b, O.SUB: exp - b, O.MUL: exp * b, O.DIV: exp // np.where(b == 0, 1, b)}[op].astype(dt)
                if all(float(v).is_integer() for row in case["inputs"] for v in row):
                    assert np.array_equal(exp, _cast(case["output"], dt))
                assert np.array_equal(O.math_nary(op, dtype_id, ins), exp)
            else:
                np.testing.assert_allclose(O.math_nary(op, dtype_id, ins), _cast(case["output"], dt), rtol=1e-6)


@pytest.mark.parametrize("dtype_id", range(12))
def test_math_const_golden(golden, dtype_id):
    g = golden["math_const"]
    dt = O.NP_DTYPES[dtype_id]
    for name, op in _OPS.items():
        out = O.math_const(op, dtype_id, np.array([g["x"]], dt), g["value"])
        assert out[0] == dt(g[name])
        assert O.math_const(op, dtype_id, np.array([g["x"]], dt), 1)[0] == {"Add": 5, "Subtract": 3, "Multiply": 4, "Divide": 4}[name]


@pytest.mark.parametrize("dtype_id", [O.UF32, O.UF64])
def test_math_uncertain_value_golden(golden, dtype_id):
    """MathOpImpl / MathOpMultiPortImpl on gr::UncertainValue<float | double> (Math.hpp:25-28, 68-71): the reference's own known answers for its operators
    (meta/test/qa_UncertainValue.cpp), as a const op and as a two-input op"""
    g = golden["uncertain_value"]
    dt = O.NP_DTYPES[dtype_id]
    for name, op in _OPS.items():
        c = g[name]
        a, b, want = np.array([c["a"]], dt), np.array([c["b"]], dt), np.array([c["out"]], dt)
        np.testing.assert_allclose(O.math_const(op, dtype_id, a, c["b"]), want, rtol=2e-7 if dt == np.float32 else 1e-15)
        np.testing.assert_allclose(O.math_nary(op, dtype_id, [a, b]), want, rtol=2e-7 if dt == np.float32 else 1e-15)
    # three inputs fold from the left like std::transform over the ports (Math.hpp:100-107): ((a + b) + c)
    a, b, c = (np.array([[1.0, 3.0]], dt), np.array([[2.0, 4.0]], dt), np.array([[3.0, 12.0]], dt))
    np.testing.assert_allclose(O.math_nary(O.ADD, dtype_id, [a, b, c]), np.array([[6.0, 13.0]], dt), rtol=1e-6)


@pytest.mark.parametrize("dtype_id", [O.UF32, O.UF64])
def test_math_uncertain_value_fixture_from_the_reference_header(dtype_id):
    """tests/golden/uncertain_value_ops.npz holds what the reference's own meta/UncertainValue.hpp computes for 2304 operand pairs per type (generated by
    tests/golden/make_uncertain_fixture.py, re-checked against the reference in the container by tests/test_host_cpp.py): the oracle's restatement gives the same"""
    fx = np.load(os.path.join(O.ROOT, "tests", "golden", "uncertain_value_ops.npz"))["f32" if dtype_id == O.UF32 else "f64"]
    a, b = np.ascontiguousarray(fx[:, 0:2]), np.ascontiguousarray(fx[:, 2:4])
    for k, op in enumerate((O.ADD, O.SUB, O.MUL, O.DIV)):
        want = fx[:, 4 + 2 * k:6 + 2 * k]
        got = O.math_nary(op, dtype_id, [a, b])
        assert np.array_equal(got[:, 0], want[:, 0]), op
        np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=2e-7 if dtype_id == O.UF32 else 4e-16, atol=0)


def test_math_integer_wraparound():
    x = np.array([250, 3, 255], np.uint8)
    assert np.array_equal(O.math_const(O.ADD, O.U8, x, 10), np.array([4, 13, 9], np.uint8))
    assert np.array_equal(O.math_const(O.MUL, O.I8, np.array([100, -100], np.int8), 2), np.array([-56, 56], np.int8))
    assert np.array_equal(O.math_const(O.DIV, O.I32, np.array([-7, 7], np.int32), 2), np.array([-3, 3], np.int32))


def test_rotator_golden(golden):
    g = golden["rotator"]
    inc = np.float32(np.pi * g["phase_increment_over_pi"])
    y, _ = O.rotator(np.ones(g["n"], np.complex64), float(inc))
    for i in range(g["n"]):
        want = (i + 1) * float(inc)
        assert abs(y[i].real - math.cos(want)) < g["tolerance"] and abs(y[i].imag - math.sin(want)) < g["tolerance"]


# ------------------------------------------------------------------ FFT block + chain (a7, headline)
def test_fft_block_peak_and_consistency(golden):
    g = golden["fft_block"]
    N = g["N"]
    x = np.cos(2 * np.pi * g["tone_frel"] * np.arange(N)).astype(np.complex64)
    mag, ph, re, im = O.fft_block_truth(x, window_id=3, in_db=True)
    freqs = (np.arange(N) - N // 2) / N
    assert abs(abs(freqs[int(np.argmax(mag))]) - g["tone_frel"]) <= 1.0 / N
    w = O.window(3, N)
    sp = np.fft.fft(x.astype(np.complex128) * w)
    np.testing.assert_allclose(re, sp.real, atol=1e-9)
    np.testing.assert_allclose(im, sp.imag, atol=1e-9)
    np.testing.assert_allclose(ph, np.fft.fftshift(np.angle(sp)), atol=1e-7)
    # real input: N/2 outputs
    magr, _, rer, _ = O.fft_block_truth(x.real.astype(np.float32), window_id=3)
    assert len(magr) == N // 2 and abs(np.argmax(magr) / N - g["tone_frel"]) <= 1.0 / N


def test_chain_mag2_relation_to_block_magnitude():
    """mag2[(k+N/2) mod N] == (mag_ref[k]*N/2)^2 links the mag2 stream to the reference block output."""
    N = 256
    b = O.design_taps_hamming_lowpass(33, 0.1)
    x = O.signal_c32(42, 4 * N)
    m2, _ = O.chain(b, x, N, window_id=3)
    y, _ = O.fir(b, x)
    for f in range(4):
        mag, _, _, _ = O.fft_block_truth(y[f * N:(f + 1) * N].astype(np.complex64), window_id=3)
        # (block oracle sees float-rounded FIR output; relation holds to float rounding)
        np.testing.assert_allclose(np.fft.fftshift(m2[f * N:(f + 1) * N]), (mag * N / 2) ** 2, rtol=2e-5, atol=1e-6)


def test_chain_f32_vs_truth():
    N = 1024
    b = O.design_taps_hamming_lowpass(256, 0.1)
    x = O.signal_c32(42, 3 * N)
    t, _ = O.chain(b, x, N, 0, truth=True)
    f, _ = O.chain(b, x, N, 0, truth=False)
    assert np.max(np.abs(f - t)) / np.sqrt(np.mean(t ** 2)) < 1e-5


def test_interpolating_fir_oracle_matches_its_polyphase_form():
    """the interpolating FIR has no reference block (parity unpinned upstream): the oracle states SURVEY.md Appendix A literally (zero-stuff, a1 sum,
    gain L); here it is checked against the independent polyphase identity y[m L + p] = L sum_q b[q L + p] x[m - q] in numpy float64, across calls"""
    rng = np.random.default_rng(11)
    for L, K, cplx in ((2, 33, False), (3, 10, True), (8, 64, False), (5, 1, True), (1, 7, False)):
        b = rng.standard_normal(K).astype(np.float32)
        x = (rng.standard_normal(300) + 1j * rng.standard_normal(300)).astype(np.complex64) if cplx else rng.standard_normal(300).astype(np.float32)
        y1, h = O.fir_interp(b, x[:101], L)
        y2, _ = O.fir_interp(b, x[101:], L, h)
        got = np.concatenate([y1, y2])
        xx = x.astype(np.complex128 if cplx else np.float64)
        want = np.zeros(len(x) * L, got.dtype)
        for n in range(len(want)):
            m, p = divmod(n, L)
            q = np.arange((K - p + L - 1) // L)
            q = q[m - q >= 0]
            want[n] = L * np.sum(b[q * L + p].astype(np.float64) * xx[m - q])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
