"""The complex-tap FIR's oracle against numpy and against the real-tap oracle, and the band form the matrix-pipe kernel evaluates against the direct sum (no GPU)."""
import numpy as np
import pytest

import complex_fir_oracle as CO
import oracle_lib as O

SHAPES = [(K, D) for K in (1, 2, 5, 33, 64, 100) for D in (1, 2, 3, 4, 8)]


def _cnoise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)


@pytest.mark.parametrize("K", [1, 2, 5, 33, 100])
def test_cfir64_is_numpy_convolve(K):
    rng = np.random.default_rng(K)
    b, x = _cnoise(rng, K), _cnoise(rng, 600)
    y, hist = CO.cfir64(b, x)
    np.testing.assert_allclose(y, np.convolve(b, x)[:len(x)], rtol=0, atol=1e-13)
    assert np.array_equal(hist, x[len(x) - (K - 1):])
    for D in (2, 3, 8):
        np.testing.assert_allclose(CO.cfir64(b, x, D)[0], np.convolve(b, x)[:len(x):D], rtol=0, atol=1e-13)
    # the carried history: two calls are one call
    y1, h1 = CO.cfir64(b, x[:240], 4)
    y2, _ = CO.cfir64(b, x[240:], 4, h1)
    np.testing.assert_allclose(np.concatenate([y1, y2]), CO.cfir64(b, x, 4)[0], rtol=0, atol=1e-13)


@pytest.mark.parametrize("K,D", SHAPES)
def test_band_tile_is_the_direct_sum(K, D):
    rng = np.random.default_rng(100 * K + D)
    b = _cnoise(rng, K)
    x = _cnoise(rng, D * (3 * 128 + 11))
    hist = _cnoise(rng, max(K - 1, 1))
    y, _ = CO.cfir64(b, x, D, hist)
    for o0 in (0, 128, 256):
        t = CO.band_tile(b, x, D, o0, hist)
        assert np.max(np.abs(t - y[o0:o0 + 128])) <= 1e-13, (K, D, o0)


@pytest.mark.parametrize("K,D", SHAPES)
def test_band_table_holds_copies_and_sign_flips_of_the_taps_only(K, D):
    rng = np.random.default_rng(7 * K + D)
    b = _cnoise(rng, K).astype(np.complex64)
    A, r_min = CO.band_table(b, D, np.float32)
    assert r_min == -((2 * K - 1 + 15) // 16) and len(A) == (14 * D + 2) // 16 - r_min + 1
    vals = set(np.abs(A[A != 0]).tolist())
    assert vals <= set(np.abs(b.real).tolist()) | set(np.abs(b.imag).tolist())
    # every row of the band carries every tap: Re b[k] once, Im b[k] once (with p's sign)
    for i in range(16):
        row = np.concatenate([A[r, i, :] for r in range(len(A))])
        want = np.sort(np.concatenate([b.real, -b.imag if i % 2 == 0 else b.imag]))
        assert np.array_equal(np.sort(row[row != 0]), want[want != 0]), (K, D, i)


def test_cfir32_seq_is_the_float32_sum_in_fir_filters_order():
    rng = np.random.default_rng(3)
    b, x = _cnoise(rng, 9).astype(np.complex64), _cnoise(rng, 64).astype(np.complex64)
    y = CO.cfir32_seq(b, x, 2)
    f = np.float32
    for m in (0, 3, 17, 31):
        re, im = f(0), f(0)
        for k in range(9):
            n = 2 * m - k
            v = x[n] if n >= 0 else np.complex64(0)
            re = f(re + f(f(f(b[k].real) * f(v.real)) - f(f(b[k].imag) * f(v.imag))))
            im = f(im + f(f(f(b[k].real) * f(v.imag)) + f(f(b[k].imag) * f(v.real))))
        assert y[m].real == re and y[m].imag == im
    assert CO.rel(y, CO.cfir64(b, x, 2)[0]) < 1e-6


@pytest.mark.parametrize("K,D", [(1, 1), (5, 1), (33, 2), (100, 8)])
def test_real_taps_agree_with_the_real_tap_oracle(K, D):
    """Im b = 0: the block is fir_filter<complex<float>> with real taps (oracle_lib.fir, float64 accumulation), decimated"""
    rng = np.random.default_rng(K)
    b = rng.standard_normal(K).astype(np.float32)
    x = _cnoise(rng, 8 * 131).astype(np.complex64)
    t, _ = O.fir(b, x)
    y, _ = CO.cfir64(b.astype(np.complex64), x, D)
    np.testing.assert_allclose(y, t[::D], rtol=0, atol=1e-12)
