"""The float64 oracle of the inverse transform and the synthesis bank (tests/synthesis_oracle.py) against numpy's transforms, the written-out sums, closed
forms and the analysis bank's oracle (tests/pfb_oracle.py): the adjoint identity that pins the bank's definition.  No device."""
import numpy as np
import pytest

import pfb_oracle as PO
import synthesis_oracle as SO

ADJOINT_SHAPES = [(8, 1), (8, 4), (64, 3), (256, 4), (1024, 8), (256, 32)]


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


@pytest.mark.parametrize("N", [2, 8, 64, 1024])
def test_against_numpy(N):
    X = noise(5 * N, N).reshape(5, N)
    assert np.allclose(SO.ifft_c2c(X, N), N * np.fft.ifft(X, axis=1), rtol=0, atol=1e-12 * N)
    half = np.array(X[:, :N // 2 + 1])
    half[:, 0], half[:, -1] = half[:, 0].real, half[:, -1].real
    want = N * np.fft.irfft(half, n=N, axis=1)
    got = SO.ifft_c2r(X, N)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=0, atol=1e-12 * N)
    # what the C2R form ignores: the imaginary parts of bins 0 and N/2, and every bin above N/2
    junk = np.array(X)
    junk[:, N // 2 + 1:] = np.nan
    junk.imag[:, 0] = np.nan
    junk.imag[:, N // 2] = np.nan
    assert np.array_equal(SO.ifft_c2r(junk, N), got)
    # and it is the real part of the C2C form on the Hermitian expansion, whose imaginary part vanishes
    full = SO.ifft_c2c(SO.hermitian(X, N), N)
    assert np.allclose(full.real, got, rtol=0, atol=1e-11 * N) and np.max(np.abs(full.imag)) <= 1e-11 * N


@pytest.mark.parametrize("N", [2, 4, 16])
def test_c2r_formula_written_out(N):
    """x[n] = Re X[0] + (-1)^n Re X[N/2] + 2 sum_{k = 1}^{N/2 - 1} Re(X[k] e^{+2 pi i k n / N})"""
    X = noise(N, 7 + N)
    n = np.arange(N)
    x = X[0].real + (-1.0) ** n * X[N // 2].real
    for k in range(1, N // 2):
        x = x + 2 * (X[k] * np.exp(2j * np.pi * k * n / N)).real
    half = np.array(X[:N // 2 + 1])
    half[0], half[-1] = half[0].real, half[-1].real
    assert np.allclose(x, N * np.fft.irfft(half, n=N), rtol=0, atol=1e-12 * N)
    assert np.allclose(SO.ifft_c2r(X, N)[0], x, rtol=0, atol=1e-12 * N)


@pytest.mark.parametrize("N,c", [(8, 0), (8, 3), (64, 63), (256, 128)])
def test_impulse_gives_the_exponential(N, c):
    X = np.zeros(N, np.complex128)
    X[c] = 1.0
    assert np.allclose(SO.ifft_c2c(X, N)[0], np.exp(2j * np.pi * c * np.arange(N) / N), rtol=0, atol=1e-13)


@pytest.mark.parametrize("N,P", [(8, 1), (8, 4), (64, 3)])
def test_impulse_frame_lays_out_the_prototype(N, P):
    """Y_0 = N in bin 0 and nothing else: v_0[i] = N for every i, so the P output frames that hold it are N g"""
    g = PO.design(N, P)
    Y = np.zeros((P + 2, N), np.complex128)
    Y[0, 0] = N
    y = SO.synth(g, Y, N, P)
    assert np.allclose(y[:P].ravel(), N * g.astype(np.float64), rtol=0, atol=1e-12 * N)
    assert np.max(np.abs(y[P:])) <= 1e-12 * N
    # value for value in float32 too: one term per sample, the rest are fma(g, 0, y)
    v = np.zeros((P + 2, N), np.complex64)
    v[0] = N
    assert np.array_equal(SO.back_end_u32(g, v, N, P)[:P].ravel(), (np.float32(N) * g).astype(np.complex64))


@pytest.mark.parametrize("N", [8, 256])
def test_one_tap_is_the_windowed_transform(N):
    w = PO.window("Hann", N).astype(np.float32)
    Y = noise(6 * N, 3).reshape(6, N)
    assert np.allclose(SO.synth(w, Y, N, 1), w.astype(np.float64) * SO.ifft_c2c(Y, N), rtol=0, atol=1e-12 * N)


@pytest.mark.parametrize("N,P", ADJOINT_SHAPES)
def test_adjoint_of_the_analysis_bank(N, P):
    """<A x, Y> = <x, D^-1 S Y>: the synthesis bank with the analysis bank's prototype, advanced by P - 1 frames, is the analysis bank's adjoint"""
    M = P + 5
    h = PO.design(N, P)
    x, Y = noise(M * N, 11 * N + P), noise(M * N, 13 * N + P).reshape(M, N)
    Ax = PO.pfb(h, x, N, P)
    SY = SO.synth(h, np.concatenate([Y, np.zeros((P - 1, N))]), N, P)[P - 1:]  # the delay taken out: frames P - 1 .. M + P - 2
    lhs, rhs = np.sum(Ax * np.conj(Y)), np.sum(x.reshape(M, N) * np.conj(SY))
    err = abs(lhs - rhs) / abs(lhs)
    print(f"N {N} P {P}: adjoint mismatch {err:.1e}")
    assert err <= 1e-12


@pytest.mark.parametrize("N,P", [(8, 1), (8, 4), (64, 3), (256, 32)])
def test_chunk_invariance(N, P):
    M = P + 6
    g = PO.design(N, P)
    Y = noise(M * N, 5 * N + P).reshape(M, N)
    whole = SO.synth(g, Y, N, P)
    v = SO.ifft_c2c(Y, N).astype(np.complex64)
    whole32 = SO.back_end_u32(g, v, N, P)
    at, parts, parts32 = 0, [], []
    for n in (1, 2, max(P - 2, 0), P - 1, M):
        n = min(n, M - at)
        parts.append(SO.synth(g, Y[at:at + n], N, P, history=Y[:at] if at else None))
        parts32.append(SO.back_end_u32(g, v[at:at + n], N, P, history=v[:at] if at else None))
        at += n
    assert at == M
    assert np.array_equal(np.concatenate(parts), whole)  # (the same float64 operations in the same order)
    assert np.array_equal(np.concatenate(parts32), whole32)
    assert SO.rel(whole32, whole) <= 1e-6
