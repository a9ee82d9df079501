"""The polyphase filter bank's oracle against numpy, its impulse response, the leakage it is built for, and the library's host-only prototype design (no GPU)."""
import numpy as np
import pytest

import pfb_oracle as PO


def _cnoise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)


@pytest.mark.parametrize("N", [8, 64, 256])
def test_one_tap_per_channel_is_the_windowed_fft(N):
    rng = np.random.default_rng(N)
    x = _cnoise(rng, 5 * N)
    w = PO.window("Hann", N)
    np.testing.assert_allclose(PO.pfb(w, x, N, 1), np.fft.fft(x.reshape(-1, N) * w, axis=1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("N,P,j", [(8, 1, 5), (8, 4, 0), (16, 3, 37), (64, 4, 64 * 2 + 63), (32, 8, 32 * 9 + 1)])
def test_impulse_gives_the_prototype_in_exactly_p_frames(N, P, j):
    rng = np.random.default_rng(N + P)
    h = rng.standard_normal(N * P)
    M = j // N + P + 3
    x = np.zeros(M * N, np.complex128)
    x[j] = 1.0
    X = PO.pfb(h, x, N, P)
    f, i = divmod(j, N)
    c = np.arange(N)
    for m in range(M):
        k = f - m + P - 1  # the tap block that meets input frame f in output frame m
        want = h[k * N + i] * np.exp(-2j * np.pi * i * c / N) if 0 <= k < P else np.zeros(N)
        np.testing.assert_allclose(X[m], want, rtol=0, atol=1e-13, err_msg=f"frame {m}")
    assert sum(bool(np.any(X[m] != 0)) for m in range(M)) == P


def test_history_makes_two_calls_one_call():
    rng = np.random.default_rng(1)
    N, P = 16, 4
    h, x = rng.standard_normal(N * P), _cnoise(rng, 11 * N)
    whole = PO.pfb(h, x, N, P)
    a = PO.pfb(h, x[:2 * N], N, P)  # fewer than P - 1 frames: the history is shorter than the window
    b = PO.pfb(h, x[2 * N:], N, P, history=x[:2 * N])
    np.testing.assert_allclose(np.concatenate([a, b]), whole, rtol=0, atol=1e-13)


def test_front_end_f32_is_the_float32_fma_sum():
    rng = np.random.default_rng(2)
    N, P = 8, 3
    h = rng.standard_normal(N * P).astype(np.float32)
    x = _cnoise(rng, 6 * N).astype(np.complex64)
    got = np.fft.ifft(PO.front_end_f32(h, x, N, P), axis=1)
    xx = np.concatenate([np.zeros((P - 1) * N, np.complex64), x])
    for m, i in ((0, 0), (2, 5), (5, 7)):
        acc = np.float64(h[i]) * np.float64(xx[m * N + i].real)
        u = np.float32(acc)
        for k in range(1, P):
            u = np.float32(np.float64(u) + np.float64(h[k * N + i]) * np.float64(xx[(m + k) * N + i].real))
        assert abs(got[m, i].real - u) <= 1e-7 * max(1.0, abs(u))
    assert PO.rel(PO.front_end_f32(h, x, N, P), PO.pfb(h, x, N, P)) < 1e-6


def test_fma32_is_one_rounding_of_the_exact_value():
    import fractions
    rng = np.random.default_rng(9)
    h, s, u = (rng.standard_normal(4000).astype(np.float32) for _ in range(3))
    # ties of the double rounding: h s + u half-way between two float32 in 53 bits but not exactly
    h[:3], s[:3], u[:3] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32([2.0 ** -24, -2.0 ** -24, 2.0 ** 30])
    got = PO._fma32(h, s, u)
    for i in list(range(40)) + [1000, 3999]:
        exact = fractions.Fraction(float(h[i])) * fractions.Fraction(float(s[i])) + fractions.Fraction(float(u[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        d = abs(fractions.Fraction(float(got[i])) - exact)
        assert d <= abs(fractions.Fraction(float(lo)) - exact) and d <= abs(fractions.Fraction(float(hi)) - exact), i


def test_leakage_is_20_db_below_the_hann_fft():
    """a tone half-way between two bins (40.5 of 256): 4 Hamming-sinc taps per channel against the Hann-windowed FFT, 3.5 and 7.5 bins away"""
    N, P, M = 256, 4, 12
    x = np.exp(2j * np.pi * 40.5 / N * np.arange(M * N))
    bank = np.abs(PO.pfb(PO.design(N, P, "Hamming"), x, N, P)[M - 1]) ** 2
    hann = np.abs(np.fft.fft(x[-N:] * PO.window("Hann", N))) ** 2
    db = lambda p, c: 10 * np.log10(p[c] / p.max())
    for c in (44, 48):
        print(f"bin {c}: Hann FFT {db(hann, c):.1f} dB, polyphase {db(bank, c):.1f} dB")
        assert db(bank, c) <= db(hann, c) - 20.0


@pytest.mark.parametrize("N,P,window,beta", [(8, 1, "Hamming", 1.6), (256, 4, "Hamming", 1.6), (64, 3, "Hann", 1.6), (1024, 8, "Kaiser", 6.0), (16, 32, "Blackman", 1.6),
                                             (128, 2, "Rectangular", 1.6)])
def test_library_design_equals_the_oracle_bit_for_bit(N, P, window, beta):
    from gnuradio4_amd import capi
    L = capi.lib()  # host only: the library loads without a device
    h = np.empty(N * P, np.float32)
    assert L.gr4hip_pfb_design(h.ctypes.data, N, P, capi.WINDOWS.index(window), beta) == capi.OK
    want = PO.design(N, P, window, np.float64(np.float32(beta)))
    assert np.array_equal(h.view(np.uint32), want.view(np.uint32))
    assert abs(h[(N * P) // 2] - 1.0) < 0.1 and np.argmax(h) in ((N * P) // 2 - 1, (N * P) // 2)


def test_library_design_refuses_bad_arguments():
    from gnuradio4_amd import capi
    L = capi.lib()
    h = np.empty(64, np.float32)
    assert L.gr4hip_pfb_design(None, 8, 4, 2, 1.6) == capi.INVALID_ARGUMENT
    assert L.gr4hip_pfb_design(h.ctypes.data, 1, 4, 2, 1.6) == capi.INVALID_ARGUMENT
    assert L.gr4hip_pfb_design(h.ctypes.data, 8, 0, 2, 1.6) == capi.INVALID_ARGUMENT
    assert L.gr4hip_pfb_design(h.ctypes.data, 8, 4, 99, 1.6) == capi.INVALID_ARGUMENT
