"""Oracle of the adaptive (MVDR / Capon) beamformer weights (include/gr4hip.h, gr4hip_mvdr_*; ADAPTIVE_WEIGHTS.md).  The reference has no such block, so this file
IS the definition: matrices V[q][p][c] as the X-engine writes them (packed lower triangle p = i (i + 1) / 2 + j, j <= i, bin fastest, complex64), steering
vectors a[b][s][c] (complex64), loading >= 0; all arithmetic float64, per matrix q and bin c:

    R_ij = V_ij (j < i),  R_ji = conj(V_ij),  R_ii = Re V_ii (the imaginary part is ignored)
    lambda = loading * (sum_i R_ii) / S ;   R'_ii = R_ii + lambda
    R' = L L^H   Cholesky, columns j ascending, every inner sum with k ascending:
        s_j  = R'_jj - sum_{k<j} |L_jk|^2 ;   L_jj = sqrt(s_j)
        L_ij = (R'_ij - sum_{k<j} L_ik conj(L_jk)) / L_jj            (i > j)
    per beam b:   L y = a_b  (forward, k ascending) ;   d = sum_k |y_k|^2
                  L^H u = y  (backward) ;   w = u / d
    W[q][b][s][c] = conj(w_s)  rounded once to complex<float>
    P[q][b][c]    = (float)(1 / d)
    a pivot s_j that is not > 0 (NaN included) fails the bin: every W and P of that (q, c) is a quiet NaN and the bin is counted

mvdr_ordered is these operations in numpy float64, vectorised over matrices and bins; mvdr_exact the same routine in numpy.clongdouble, not rounded.  bound_w and
bound_p are the error bounds every comparison with mvdr_exact uses:
    per component |W - W_exact| <= 2^-24 |W_exact| + (8 + S) cond2(R') 2^-53 ||w||_2          |P - P_exact| <= 2^-24 P + 2 (8 + S) cond2(R') 2^-53 P"""
import numpy as np

import cross_spectrum_oracle as XO
from cross_spectrum_oracle import baseline

assert np.finfo(np.longdouble).eps < 1e-18, "mvdr_exact needs a long double of at least 64 mantissa bits (x87 80-bit)"


def steering(B, S, N, seed):
    """the tests' steering vectors: complex64 [B, S, N] of unit modulus, phases drawn from default_rng(seed)"""
    rng = np.random.default_rng(seed)
    return np.exp(2j * np.pi * rng.random((B, S, N))).astype(np.complex64)


def hand_made(S=4, N=6):
    """the tests' failing bins: (four matrices complex64 [4, P, N], well conditioned but for one bin each, [(q, c) of those bins]): (0, 1) all zero, (1, 2)
    V_00 = -1, (2, 3) a NaN on a diagonal, (3, 4) a NaN off the diagonal.  Without them: cross_ordered(streams(S, 64, N, 5), 16, mean=True)."""
    V = np.array(XO.cross_ordered(XO.streams(S, 4 * 16, N, 5), 16, mean=True))
    assert V.shape == (4, S * (S + 1) // 2, N)
    V[0, :, 1] = 0
    V[1, baseline(0, 0), 2] = -1
    V[2, baseline(2, 2), 3] = np.nan
    V[3, baseline(3, 1), 4] = np.nan + 0j
    return V, [(0, 1), (1, 2), (2, 3), (3, 4)]


def loaded_matrix(V, S, loading, ct=np.complex128):
    """R' [S, S, Q, N] of matrices V [Q, P, N] in the complex type ct"""
    V = np.asarray(V)
    rt = np.float64 if ct == np.complex128 else np.longdouble
    Q, P, N = V.shape
    assert P == S * (S + 1) // 2
    R = np.zeros((S, S, Q, N), ct)
    for i in range(S):
        for j in range(i):
            v = V[:, baseline(i, j)].astype(ct)
            R[i, j] = v
            R[j, i] = np.conj(v)
        R[i, i] = V[:, baseline(i, i)].real.astype(rt)
    tr = np.zeros((Q, N), rt)
    for i in range(S):
        tr = tr + R[i, i].real
    lam = rt(loading) * tr / rt(S)
    for i in range(S):
        R[i, i] = R[i, i].real + lam
    return R


def _mod2(z):
    return z.real * z.real + z.imag * z.imag


def _solve(V, a, loading, ct):
    V = np.asarray(V)
    if V.ndim == 2:
        V = V[None]
    a = np.asarray(a)
    rt = np.float64 if ct == np.complex128 else np.longdouble
    B, S, N = a.shape
    Q = V.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        R = loaded_matrix(V, S, loading, ct)
        L = np.zeros((S, S, Q, N), ct)
        failed = np.zeros((Q, N), bool)
        for j in range(S):
            s = R[j, j].real.copy()
            for k in range(j):
                s = s - _mod2(L[j, k])
            failed |= ~(s > 0)
            d = np.sqrt(s)
            L[j, j] = d
            for i in range(j + 1, S):
                t = R[i, j].copy()
                for k in range(j):
                    t = t - L[i, k] * np.conj(L[j, k])
                L[i, j] = t / d
        W = np.zeros((Q, B, S, N), ct)
        P = np.zeros((Q, B, N), rt)
        for b in range(B):
            y = np.zeros((S, Q, N), ct)
            for i in range(S):
                t = np.broadcast_to(a[b, i].astype(ct), (Q, N)).copy()
                for k in range(i):
                    t = t - L[i, k] * y[k]
                y[i] = t / L[i, i].real
            dd = np.zeros((Q, N), rt)
            for k in range(S):
                dd = dd + _mod2(y[k])
            u = np.zeros((S, Q, N), ct)
            for i in range(S - 1, -1, -1):
                t = y[i].copy()
                for k in range(i + 1, S):
                    t = t - np.conj(L[k, i]) * u[k]
                u[i] = t / L[i, i].real
            W[:, b] = np.conj(u / dd).transpose(1, 0, 2)
            P[:, b] = 1 / dd
        W[np.broadcast_to(failed[:, None, None, :], W.shape)] = np.nan + 1j * np.nan
        P[np.broadcast_to(failed[:, None, :], P.shape)] = np.nan
    return W, P, failed


def mvdr_ordered(V, a, loading=0.0):
    """(W complex64 [Q, B, S, N], P float32 [Q, B, N], failed bool [Q, N]): the definition in float64, rounded once"""
    W, P, failed = _solve(V, a, loading, np.complex128)
    with np.errstate(invalid="ignore", over="ignore"):
        return W.astype(np.complex64), P.astype(np.float32), failed


def mvdr_exact(V, a, loading=0.0):
    """(W clongdouble [Q, B, S, N], P longdouble [Q, B, N], failed bool [Q, N]): the same routine in long double, not rounded"""
    return _solve(V, a, loading, np.clongdouble)


def kappa(V, S, loading=0.0):
    """cond2 of R' per matrix and bin, float64 [Q, N]"""
    V = np.asarray(V)
    if V.ndim == 2:
        V = V[None]
    R = loaded_matrix(V, S, loading, np.complex128)
    return np.linalg.cond(np.ascontiguousarray(R.transpose(2, 3, 0, 1)))


def bound_w(Wx, kap, S):
    """per component of W: (bound of the real parts, bound of the imaginary parts), float64 [Q, B, S, N] each"""
    Wx = np.asarray(Wx)
    nrm = np.sqrt(_mod2(Wx).sum(axis=2)).astype(np.float64)  # ||w||_2 [Q, B, N]
    tail = (8 + S) * kap[:, None, None, :] * 2.0 ** -53 * nrm[:, :, None, :]
    return 2.0 ** -24 * np.abs(Wx.real).astype(np.float64) + tail, 2.0 ** -24 * np.abs(Wx.imag).astype(np.float64) + tail


def bound_p(Px, kap, S):
    Px = np.asarray(Px).astype(np.float64)
    return 2.0 ** -24 * Px + 2 * (8 + S) * kap[:, None, :] * 2.0 ** -53 * Px


def ratios(W, P, Wx, Px, kap, S):
    """(worst |W - W_exact| / bound over both components, worst |P - P_exact| / bound); P may be None"""
    W = np.asarray(W)
    br, bi = bound_w(Wx, kap, S)
    er = np.abs(W.real.astype(np.longdouble) - Wx.real).astype(np.float64)
    ei = np.abs(W.imag.astype(np.longdouble) - Wx.imag).astype(np.float64)
    rw = max(float(np.max(er / br)), float(np.max(ei / bi)))
    rp = None
    if P is not None:
        rp = float(np.max(np.abs(np.asarray(P).astype(np.longdouble) - Px).astype(np.float64) / bound_p(Px, kap, S)))
    return rw, rp
