"""The rational resampler's own oracle (tests/rational_resampler_oracle.py) checked against itself and against the oracles the project already trusts: the literal
definition against the evaluated form, M = 1 against the interpolator's oracle, L = 1 against the decimating fir_filter's, impulses, a pass-band tone through the
designed low-pass, and gr4hip_resamp_design against the formula.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import rational_resampler_oracle as RO

SHAPES = [(1, 1), (2, 3), (3, 2), (3, 4), (5, 7), (7, 5), (4, 6), (8, 1), (1, 8), (16, 5), (147, 160), (160, 147)]


def _taps(K, L, M, seed=0):
    if K < 8:
        return (np.random.default_rng(seed + K).standard_normal(K) / K).astype(np.float32)
    return O.design_taps_hamming_lowpass(K, 0.4 / max(L, M))


def _signal(n, seed, cplx):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
    return x.astype(np.complex64 if cplx else np.float32)


@pytest.mark.parametrize("L,M", SHAPES)
@pytest.mark.parametrize("cplx", [False, True])
def test_literal_and_evaluated_forms_agree(L, M, cplx):
    for K in sorted({1, max(1, L - 1), L, L + 1, 8 * L + 3}):
        b, x = _taps(K, L, M), _signal(M * 23, 100 * L + M, cplx)
        t, h = RO.resamp64(b, x, L, M)
        p, hp = RO.resamp64_poly(b, x, L, M)
        assert t.shape == (23 * L,) and len(h) == RO.branch_length(K, L) - 1 and np.array_equal(h, hp)
        assert RO.rel(p, t) <= 1e-6  # (the evaluated form multiplies by float32(L b), the literal one by b and then by L)
        assert RO.rel(RO.resamp32_seq(b, x, L, M), t) <= 3e-6
        # cut into calls with the carried history: the same stream; float32 bit for bit
        cut = M * 9
        t1, h1 = RO.resamp64(b, x[:cut], L, M)
        t2, h2 = RO.resamp64(b, x[cut:], L, M, h1)
        assert np.allclose(np.concatenate([t1, t2]), t, rtol=0, atol=1e-12) and np.array_equal(h2, h)
        s = np.concatenate([RO.resamp32_seq(b, x[:cut], L, M), RO.resamp32_seq(b, x[cut:], L, M, x[:cut])])
        assert np.array_equal(s.view(np.uint32), RO.resamp32_seq(b, x, L, M).view(np.uint32))


@pytest.mark.parametrize("L,K", [(1, 7), (2, 9), (3, 2), (8, 67), (16, 131)])
@pytest.mark.parametrize("cplx", [False, True])
def test_decimate_one_is_the_interpolator(L, K, cplx):
    b, x = _taps(K, L, 1), _signal(300, L, cplx)
    want, _ = O.fir_interp(b, x, L)
    assert RO.rel(RO.resamp64(b, x, L, 1)[0], want) <= 1e-12


@pytest.mark.parametrize("M,K", [(1, 7), (2, 9), (3, 2), (8, 64), (5, 131)])
def test_interpolate_one_is_the_decimating_fir(M, K):
    b, x = _taps(K, 1, M), _signal(M * 100, M, False)
    want, _ = O.fir_decim(b, x, M)
    assert RO.rel(RO.resamp64(b, x, 1, M)[0], want) <= 1e-12
    xc = _signal(M * 100, M + 50, True)
    wantc, _ = O.fir(b, xc)
    assert RO.rel(RO.resamp64(b, xc, 1, M)[0], wantc[::M]) <= 1e-12


@pytest.mark.parametrize("L,M", SHAPES)
def test_unit_impulse_returns_the_branch_taps_at_their_indices(L, M):
    K = 4 * L + 1
    b = (0.5 + np.arange(K) / (2.0 * K)).astype(np.float32)  # all different, all non-zero
    w = RO.branch_taps(b, L, M)
    o, phi = RO.slots(L, M)
    assert w.shape == (5, L) and np.array_equal(w[0], np.float32(L) * b[phi])
    n_in = M * 12
    for i in (0, 1, M - 1, M, 3 * M + 1):
        x = np.zeros(n_in, np.float32)
        x[i] = 1.0
        y = RO.resamp32_seq(b, x, L, M)
        want = RO.impulse_response(b, L, M, i, n_in)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
        for j in np.flatnonzero(want):  # the definition, index by index: output j sees tap k = j M - i L
            k = int(j) * M - i * L
            assert 0 <= k < K and want[j] == np.float32(L) * b[k]
        assert np.count_nonzero(want) == len([j for j in range(12 * L) if 0 <= j * M - i * L < K])
        assert np.allclose(RO.resamp64(b, x, L, M)[0], want, rtol=1e-7, atol=0)  # (L b[k] in float64 against its float32 rounding; an impulse between kept samples gives all zeros)


@pytest.mark.parametrize("L,M", [(3, 4), (2, 3), (25, 32), (147, 160), (160, 147), (8, 1), (1, 8)])
def test_pass_band_tone_comes_out_at_the_new_rate_with_unit_gain(L, M):
    import gnuradio4_amd as G
    half = 8
    b = G.design_resampler_taps(L, M, half)
    assert len(b) == 2 * half * max(L, M) + 1 and abs(float(b.astype(np.float64).sum()) - 1.0) < 1e-6
    n_cyc = 40 * half  # (output cycles; the first 2 half max(L, M) / L + 1 input samples are the filter filling up)
    f = 0.25 * min(1.0, L / M)  # cycles per input sample: inside 0.4 / max(L, M) of the L-times rate, f / L < 0.4 / max(L, M)
    n = np.arange(M * n_cyc)
    x = np.exp(2j * np.pi * f * n).astype(np.complex64)
    y, _ = RO.resamp64(b, x, L, M)
    delay = (len(b) - 1) / 2.0 / L  # in input samples
    j = np.arange(len(y))
    want = np.exp(2j * np.pi * f * (j * M / L - delay))  # frequency f M / L per output sample
    skip = int(np.ceil((len(b) - 1) / M)) + 1
    err = np.max(np.abs(y[skip:] - want[skip:]))
    # the design's ripple at this tone: the zero-stuffed tone has L components of amplitude 1 / L at (f + m) / L, the gain L makes them 1, the filter's response H weighs
    # them: y = H(f / L) (the wanted tone; H has linear phase, the delay above) + the L - 1 images, each at most |H((f + m) / L)| wherever decimation folds it to
    k = np.arange(len(b))
    H = lambda nu: np.sum(b.astype(np.float64) * np.exp(-2j * np.pi * nu * k))  # noqa: E731
    ripple = abs(abs(H(f / L)) - 1.0) + sum(abs(H((f + m) / L)) for m in range(1, L))
    print(f"L {L} M {M}: tone error {err:.2e}, the design's ripple at this tone {ripple:.2e}")
    assert err <= ripple + 1e-9
    assert ripple <= 1e-2  # Hamming window: pass band within 0.2 %, stop band below -53 dB and falling


@pytest.mark.parametrize("L,M,half,window,beta", [(3, 4, 8, "Hamming", 1.6), (147, 160, 4, "Hamming", 1.6), (1, 1, 1, "Hann", 1.6), (5, 2, 3, "Kaiser", 6.0), (2, 7, 12, "Blackman", 1.6),
                                                  (16, 1024, 2, "Rectangular", 1.6)])
def test_library_design_equals_the_formula_bit_for_bit(L, M, half, window, beta):
    from gnuradio4_amd import capi
    lib = capi.lib()  # host only: the library loads without a device
    n = C.c_size_t(0)
    assert lib.gr4hip_resamp_design(None, 0, C.byref(n), L, M, half, capi.WINDOWS.index(window), beta) == capi.OK  # size query
    want = RO.design(L, M, half, window, beta)
    assert n.value == len(want) == 2 * half * max(L, M) + 1
    h = np.full(n.value + 2, 7.0, np.float32)
    assert lib.gr4hip_resamp_design(h.ctypes.data, n.value, C.byref(n), L, M, half, capi.WINDOWS.index(window), beta) == capi.OK
    assert np.array_equal(h[:-2].view(np.uint32), want.view(np.uint32)) and np.all(h[-2:] == 7.0)
    assert np.array_equal(want, want[::-1]) or np.allclose(want, want[::-1], rtol=1e-6, atol=0)  # linear phase


def test_library_design_refuses_bad_arguments():
    from gnuradio4_amd import capi
    lib = capi.lib()
    h, n = np.zeros(64, np.float32), C.c_size_t(0)
    assert lib.gr4hip_resamp_design(None, 0, None, 3, 4, 8, 2, 1.6) == capi.INVALID_ARGUMENT
    assert lib.gr4hip_resamp_design(None, 0, C.byref(n), 0, 4, 8, 2, 1.6) == capi.INVALID_ARGUMENT
    assert lib.gr4hip_resamp_design(None, 0, C.byref(n), 3, 0, 8, 2, 1.6) == capi.INVALID_ARGUMENT
    assert lib.gr4hip_resamp_design(None, 0, C.byref(n), 3, 4, 0, 2, 1.6) == capi.INVALID_ARGUMENT
    assert lib.gr4hip_resamp_design(h.ctypes.data, 64, C.byref(n), 3, 4, 8, 2, 1.6) == capi.INVALID_ARGUMENT and b"room for" in lib.gr4hip_last_error()
    assert lib.gr4hip_resamp_design(h.ctypes.data, 64, C.byref(n), 3, 4, 1, 99, 1.6) == capi.INVALID_ARGUMENT
    assert lib.gr4hip_resamp_design(None, 0, C.byref(n), 1025, 4, 1, 2, 1.6) == capi.UNSUPPORTED
    assert lib.gr4hip_resamp_design(None, 0, C.byref(n), 1024, 4, 33, 2, 1.6) == capi.UNSUPPORTED  # 67585 taps
    assert np.all(h == 0)
