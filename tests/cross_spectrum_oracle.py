"""Oracle of the cross-spectrum correlator (include/gr4hip.h, gr4hip_xcorr_*; CROSS_SPECTRUM.md).  The reference has no such block, so this file IS the definition:
S streams of frames X_s[f][c]; output q covers frames [q A, (q + 1) A), leaf l of it frames q A + [64 l, min(64 (l + 1), A)); baselines j <= i packed
p = i (i + 1) / 2 + j;

    per leaf, per (i, j), per bin, float32, frames ascending, re = im = +0 at the leaf's start:
        re = fmaf(xr_i, xr_j, re);   re = fmaf(xi_i, xi_j, re);
        im = fmaf(xi_i, xr_j, im);   im = fmaf(-xr_i, xi_j, im);
    acc_re, acc_im: float64, leaves ascending, ((0 + (double)leaf_0) + (double)leaf_1) + ...
    V_q[p][c] = ((float)acc_re, (float)acc_im)   or, mean,   ((float)(acc_re / A), (float)(acc_im / A))
    the imaginary part of the diagonal (i == j) is exactly +0

cross_exact is the plain complex128 sum, cross_ordered the definition with the exact float32 fma of tests/pfb_oracle.py.  A trailing incomplete integration is
dropped by both.  coherence is the float64 formula of gr4hip_xcorr_coherence."""
import numpy as np

from pfb_oracle import _fma32

LEAF = 64


def baseline(i, j):
    """packed index of the pair (i, j), j <= i"""
    assert j <= i
    return i * (i + 1) // 2 + j


def streams(S, frames, N, seed, common=0.7):
    """the tests' input: complex64 [S, frames, N], unit complex noise per stream plus a component all streams share, so the cross terms neither vanish nor dominate"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((S, frames, N)) + 1j * rng.standard_normal((S, frames, N))) / np.sqrt(2.0)
    c = (rng.standard_normal((frames, N)) + 1j * rng.standard_normal((frames, N))) / np.sqrt(2.0)
    g = np.exp(2j * np.pi * rng.random(S))[:, None, None]  # a fixed phase per stream: the cross spectra are complex
    return (z + common * g * c[None]).astype(np.complex64)


def cross_exact(X, A):
    """complex128 [frames // A, P, N]"""
    X = np.asarray(X, np.complex128)
    S, F, N = X.shape
    Q = F // A
    V = np.empty((Q, S * (S + 1) // 2, N), np.complex128)
    for i in range(S):
        for j in range(i + 1):
            V[:, baseline(i, j)] = (X[i, :Q * A] * np.conj(X[j, :Q * A])).reshape(Q, A, N).sum(axis=1)
    return V


def abs_bound(X, A):
    """float64 [frames // A, P, N]: sum over the integration of |X_i| |X_j|, the scale of the definition's error bound"""
    M = np.abs(np.asarray(X, np.complex128))
    S, F, N = M.shape
    Q = F // A
    W = np.empty((Q, S * (S + 1) // 2, N))
    for i in range(S):
        for j in range(i + 1):
            W[:, baseline(i, j)] = (M[i, :Q * A] * M[j, :Q * A]).reshape(Q, A, N).sum(axis=1)
    return W


def cross_ordered(X, A, mean=False):
    """complex64 [frames // A, P, N], the definition's operations one by one"""
    X = np.asarray(X, np.complex64)
    S, F, N = X.shape
    Q, P = F // A, S * (S + 1) // 2
    xr = np.ascontiguousarray(X.real)
    xi = np.ascontiguousarray(X.imag)
    ii = np.array([i for i in range(S) for j in range(i + 1)])
    jj = np.array([j for i in range(S) for j in range(i + 1)])
    V = np.empty((Q, P, N), np.complex64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Q):
            acc_re = np.zeros((P, N), np.float64)
            acc_im = np.zeros((P, N), np.float64)
            for s in range(0, A, LEAF):
                re = np.zeros((P, N), np.float32)
                im = np.zeros((P, N), np.float32)
                for f in range(q * A + s, q * A + min(s + LEAF, A)):
                    ar, ai, br, bi = xr[ii, f], xi[ii, f], xr[jj, f], xi[jj, f]
                    re = _fma32(ar, br, re)
                    re = _fma32(ai, bi, re)
                    im = _fma32(ai, br, im)
                    im = _fma32(-ar, bi, im)
                acc_re = acc_re + re.astype(np.float64)
                acc_im = acc_im + im.astype(np.float64)
            if mean:
                acc_re, acc_im = acc_re / np.float64(A), acc_im / np.float64(A)
            out_re, out_im = acc_re.astype(np.float32), acc_im.astype(np.float32)
            out_im[ii == jj] = np.float32(0.0)
            V[q].real = out_re
            V[q].imag = out_im
    return V


def coherence(vis, S, i, j):
    """(msc float32 [..., N], h1 complex64 [..., N]) of the pair (i, j) from emitted matrices vis complex64 [..., P, N]"""
    vis = np.asarray(vis, np.complex64)
    v = vis[..., baseline(max(i, j), min(i, j)), :]
    re = v.real.astype(np.float64)
    im = v.imag.astype(np.float64)
    if i < j:
        im = -im
    vii = vis[..., baseline(i, i), :].real.astype(np.float64)
    vjj = vis[..., baseline(j, j), :].real.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        msc = ((re * re + im * im) / (vii * vjj)).astype(np.float32)
        h1 = np.empty(v.shape, np.complex64)
        h1.real = (re / vjj).astype(np.float32)
        h1.imag = (im / vjj).astype(np.float32)
    return msc, h1
