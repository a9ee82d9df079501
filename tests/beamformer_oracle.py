"""Oracle of the beamformer (include/gr4hip.h, gr4hip_beamform_*; BEAMFORMER.md).  The reference has no such block, so this file IS the definition: S streams of
frames X_s[f][c], B beams, weights W[b][s][c], complex64, bin fastest;

    per beam, frame and bin, float32, streams ascending, re = im = +0 at the start:
        re = fmaf( wr_s, xr_s, re);   re = fmaf(-wi_s, xi_s, re);
        im = fmaf( wi_s, xr_s, im);   im = fmaf( wr_s, xi_s, im);
    Y_b[f][c] = (re, im)
    p_b[f][c] = fmaf(yr, yr, yi * yi), then the spectrum integrator's definition (tests/spectrum_integrator_oracle.py) on frames of B N floats laid out [b][c]

beams_exact is the plain complex128 sum, beams_ordered the definition with the exact float32 fma of tests/pfb_oracle.py, abs_bound the scale of the error bound
|Y - exact| <= (2 S + 1) 2^-24 sum_s |W[b][s][c]| |X_s[f][c]| per component."""
import numpy as np

import spectrum_integrator_oracle as SI
from pfb_oracle import _fma32


def weights(B, S, N, seed):
    """the tests' weights: complex64 [B, S, N], complex Gaussian of variance 1 / S"""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((B, S, N)) + 1j * rng.standard_normal((B, S, N))) / np.sqrt(2.0 * S)).astype(np.complex64)


def _full(W, N):
    W = np.asarray(W, np.complex64)
    return np.broadcast_to(W[:, :, None], W.shape + (N,)) if W.ndim == 2 else W


def beams_exact(W, X):
    """complex128 [B, frames, N]"""
    X = np.asarray(X, np.complex128)
    return np.einsum("bsc,sfc->bfc", _full(W, X.shape[2]).astype(np.complex128), X)


def abs_bound(W, X):
    """float64 [B, frames, N]: sum_s |W[b][s][c]| |X_s[f][c]|"""
    X = np.asarray(X, np.complex128)
    return np.einsum("bsc,sfc->bfc", np.abs(_full(W, X.shape[2]).astype(np.complex128)), np.abs(X))


def beams_ordered(W, X):
    """complex64 [B, frames, N], the definition's operations one by one; W [B, S, N] or [B, S] (the same weight in every bin)"""
    X = np.asarray(X, np.complex64)
    S, F, N = X.shape
    W = _full(W, N)
    B = W.shape[0]
    assert W.shape == (B, S, N)
    wr = np.ascontiguousarray(W.real)[:, :, None, :]  # [B, S, 1, N]
    wi = np.ascontiguousarray(W.imag)[:, :, None, :]
    xr = np.ascontiguousarray(X.real)[None]  # [1, S, F, N]
    xi = np.ascontiguousarray(X.imag)[None]
    re = np.zeros((B, F, N), np.float32)
    im = np.zeros((B, F, N), np.float32)
    shape = (B, F, N)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            a, b = np.broadcast_to(wr[:, s], shape), np.broadcast_to(wi[:, s], shape)
            u, v = np.broadcast_to(xr[:, s], shape), np.broadcast_to(xi[:, s], shape)
            re = _fma32(a, u, re)
            re = _fma32(-b, v, re)
            im = _fma32(b, u, im)
            im = _fma32(a, v, im)
    Y = np.empty(shape, np.complex64)
    Y.real = re
    Y.imag = im
    return Y


def power(Y):
    """float32 [frames, B, N]: fmaf(yr, yr, yi * yi) of voltage beams [B, frames, N], as the frames the integrator sees"""
    Y = np.asarray(Y, np.complex64)
    yr, yi = np.ascontiguousarray(Y.real), np.ascontiguousarray(Y.imag)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = _fma32(yr, yr, yi * yi)  # float32 * float32 -> one IEEE float32 multiply
    return np.ascontiguousarray(p.transpose(1, 0, 2))


def power_integrated_ordered(W, X, A, mean=False):
    """float32 [frames // A, B, N]: the integrator's ordered definition applied to the power of the ordered beams, frames [b][c]"""
    p = power(beams_ordered(W, X))
    F, B, N = p.shape
    return SI.integrate_ordered(p.reshape(F, B * N), A, mean).reshape(F // A, B, N)
