"""float64 oracle of the inverse transform and the polyphase synthesis bank (include/gr4hip.h, gr4hip_ifft_* / gr4hip_pfb_synth_*; INVERSE_FFT.md).

    ifft_c2c:  x[n] = sum_{k < N} X[k] e^{+2 pi i k n / N}                     = N numpy.fft.ifft            (the reference's Direction::Backward: unnormalised)
    ifft_c2r:  the same of the Hermitian expansion of bins 0 .. N/2, real      = N numpy.fft.irfft with the imaginary parts of bins 0 and N/2 zeroed
    synth:     v_m = ifft_c2c(Y_m);  y[m N + i] = sum_{k < P} g[k N + i] v_{m - k}[i]      (v_m = 0 for m < 0, or the transform of the carried spectra)

The bank is the project's own definition, so synth IS that definition.  back_end_u32 evaluates the bank's sums the way the kernel does (float32, from 0, k
ascending, one fma per term and component), value for value, on transformed frames v it is given."""
import numpy as np

import pfb_oracle as PO

rel = PO.rel


def ifft_c2c(X, N):
    """complex128 [frames, N]"""
    X = np.asarray(X, np.complex128).reshape(-1, N)
    return N * np.fft.ifft(X, axis=1)


def ifft_c2r(X, N):
    """float64 [frames, N] from full N-bin frames: bins 0 .. N/2 are used, the imaginary parts of bins 0 and N/2 and every bin above N/2 are ignored"""
    X = np.array(np.asarray(X, np.complex128).reshape(-1, N)[:, :N // 2 + 1])
    X[:, 0] = X[:, 0].real
    X[:, N // 2] = X[:, N // 2].real
    return N * np.fft.irfft(X, n=N, axis=1)


def hermitian(X, N):
    """the full N-bin frames the C2R form stands for: bin k > N/2 is the conjugate of bin N - k, bins 0 and N/2 are real"""
    X = np.asarray(X).reshape(-1, N)
    H = np.array(X)
    H[:, 0] = X[:, 0].real
    H[:, N // 2] = X[:, N // 2].real
    for k in range(1, N // 2):
        H[:, N - k] = np.conj(X[:, k])
    return H


def synth(g, Y, N, P, history=None):
    """complex128 [frames, N]; history: the spectra in front of Y (its last P - 1 frames count), None: zeros"""
    g = np.asarray(g, np.float64).reshape(P, N)
    f = PO._frames(Y, N, P, history, np.complex128)  # [P - 1 + frames, N]
    M = len(f) - (P - 1)
    v = N * np.fft.ifft(f, axis=1)
    y = np.zeros((M, N), np.complex128)
    for k in range(P):
        y += g[k] * v[P - 1 - k:P - 1 - k + M]
    return y


def back_end_u32(g, v, N, P, history=None):
    """the kernel's sums value for value: complex64 [frames, N] from transformed frames v (complex64); history: the transformed frames in front of v"""
    g = np.asarray(g, np.float32).reshape(P, N)
    f = PO._frames(v, N, P, history, np.complex64)
    M = len(f) - (P - 1)
    re = np.zeros((M, N), np.float32)
    im = np.zeros((M, N), np.float32)
    for k in range(P):
        s = f[P - 1 - k:P - 1 - k + M]
        gk = np.broadcast_to(g[k], (M, N))
        re = PO._fma32(gk, np.ascontiguousarray(s.real), re)
        im = PO._fma32(gk, np.ascontiguousarray(s.imag), im)
    y = np.empty((M, N), np.complex64)
    y.real, y.imag = re, im
    return y
