"""Oracle of the Savitzky-Golay blocks (numpy / Python only): the reference's computeCoefficients<T>, apply, applyZeroPhase and the streaming processOne
(algorithm/filter/SavitzkyGolay.hpp:43-267) restated under the contract of SAVITZKY_GOLAY.md.

  design        the singular values of the Vandermonde matrix from numpy.linalg.svd in float64, the truncation rule with T's epsilon (:128-133), row d of
                the truncated pseudo-inverse rounded to T and scaled in T (:142-148)
  exact_row     the least-squares coefficients as exact rationals (fractions.Fraction), for settings where the rule drops nothing
  streaming     y[n] = sum_k c[k] x[n - (W - 1) + k] over a history of zeros (:226-233 with BoundaryPolicy::Default)
  zero_phase    t[j] = sum_k c[k] x[b(j + k - D)] rounded to T, out[n] = sum_k c[k] t[b(n - k + D)] rounded to T
  zero_phase_literal   apply, reverse, apply, reverse (:177-193) word for word, in plain loops (small inputs only)
Sums are taken in numpy's widest float (at least float64), so the oracle's own rounding is the rounding of its results to T."""
from fractions import Fraction
from math import factorial

import numpy as np

WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
AMBIGUOUS_FACTOR = 16.0


def clamp(window_size, poly_order, deriv_order):
    """(:95-97)"""
    W = max(int(window_size), 1)
    p = min(int(poly_order), W - 1)
    d = min(int(deriv_order), p)
    return W, p, d


def centre(W, alignment="Centred"):
    """D (:105): "Causal", or anything else = Centred (SavitzkyGolayFilter.hpp:53-55)"""
    return W - 1 if alignment == "Causal" else (W - 1) // 2


def vandermonde(W, p, alignment="Centred"):
    """A[i][j] = (i - D)^j by the running product (:108-115), in float64"""
    D = centre(W, alignment)
    A = np.empty((W, p + 1), np.float64)
    for i in range(W):
        t, power = float(i - D), 1.0
        for j in range(p + 1):
            A[i, j] = power
            power *= t
    return A


def reflect_index(i, N):
    """detail::reflectIndex (:51-64)"""
    if N == 0:
        return 0
    if i < 0:
        i = -i - 1
    period = 2 * N
    i = i % period
    if i >= N:
        i = period - i - 1
    return i


def replicate_index(i, N):
    """detail::replicateIndex (:66-77)"""
    if N == 0:
        return 0
    return 0 if i < 0 else (N - 1 if i >= N else i)


def _index_table(lo, hi, N, policy):
    """b(i) for i in [lo, hi), vectorised"""
    i = np.arange(lo, hi, dtype=np.int64)
    if policy == "Replicate":
        return np.clip(i, 0, N - 1)
    i = np.where(i < 0, -i - 1, i) % (2 * N)
    return np.where(i >= N, 2 * N - i - 1, i)


def pinv_row(dtype, window_size, poly_order, deriv_order, alignment="Centred"):
    """row d of the truncated pseudo-inverse in float64 and the facts of the truncation"""
    W, p, d = clamp(window_size, poly_order, deriv_order)
    A = vandermonde(W, p, alignment)
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    eps = float(np.finfo(dtype).eps)
    thr = eps * max(W, p + 1) * s[0]
    keep = s >= thr
    row = np.zeros(W, np.float64)
    for k in range(len(s)):  # (:130-140) the largest first
        if keep[k]:
            row += Vt[k, d] / s[k] * U[:, k]
    info = dict(W=W, p=p, d=d, rank=int(keep.sum()), sigma=s, sigma_max=float(s[0]), sigma_min_kept=float(s[keep][-1]), threshold=float(thr),
                ambiguous=bool(np.any(np.abs(s - thr) <= AMBIGUOUS_FACTOR * eps * s[0])))
    return row, info


def scale(dtype, d, delta):
    """T(d!) / std::pow(delta, T(d)) with delta = max(T(delta), eps_T) (:98, :147); d! in 64-bit unsigned arithmetic (:43-49)"""
    T = np.dtype(dtype).type
    delta = max(T(delta), np.finfo(dtype).eps)
    return T(T(factorial(d) % (1 << 64)) / T(_libm_pow(dtype, delta, T(d))))


_LIBM = None


def _libm_pow(dtype, x, y):
    """std::pow in T is libm's powf / pow: called through ctypes, because numpy's own float32 power need not round as libm does"""
    global _LIBM
    if _LIBM is None:
        import ctypes
        import ctypes.util
        _LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _LIBM.powf.restype, _LIBM.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
        _LIBM.pow.restype, _LIBM.pow.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]
    return (_LIBM.powf if np.dtype(dtype) == np.float32 else _LIBM.pow)(float(x), float(y))


def design(dtype, window_size=11, poly_order=4, deriv_order=0, delta=1.0, alignment="Centred"):
    """computeCoefficients<T>: (coefficients of T, info)"""
    T = np.dtype(dtype).type
    row, info = pinv_row(dtype, window_size, poly_order, deriv_order, alignment)
    c = row.astype(dtype)
    c = (c * scale(dtype, info["d"], delta)).astype(dtype)
    assert c.dtype == np.dtype(T)
    return c, info


def exact_row(window_size, poly_order, deriv_order, alignment="Centred"):
    """row d of (A^T A)^-1 A^T as Fractions: the least-squares coefficients nothing has been dropped from"""
    W, p, d = clamp(window_size, poly_order, deriv_order)
    D = centre(W, alignment)
    t = [Fraction(i - D) for i in range(W)]
    m = p + 1
    G = [[sum(ti ** (a + b) for ti in t) for b in range(m)] + [Fraction(int(a == d))] for a in range(m)]  # normal equations, right-hand side e_d
    for col in range(m):
        piv = next(r for r in range(col, m) if G[r][col] != 0)
        G[col], G[piv] = G[piv], G[col]
        G[col] = [v / G[col][col] for v in G[col]]
        for r in range(m):
            if r != col and G[r][col] != 0:
                f = G[r][col]
                G[r] = [vr - f * vc for vr, vc in zip(G[r], G[col])]
    z = [G[a][m] for a in range(m)]
    return [sum(z[a] * ti ** a for a in range(m)) for ti in t]


def streaming(coeffs, x, history=None):
    """processOne per sample (:226-233): y[n] = sum_k c[k] x[n - (W - 1) + k], zeros in front of the stream.  Returns (y of x's dtype, sum_k |c_k x_k| per output)."""
    c = np.asarray(coeffs)
    W = len(c)
    x = np.asarray(x)
    xp = np.concatenate([np.zeros(W - 1, x.dtype) if history is None else np.asarray(history, x.dtype), x]).astype(WIDE)
    win = np.lib.stride_tricks.sliding_window_view(xp, W)  # win[n][k] = x[n - (W - 1) + k]
    cw = c.astype(WIDE)
    y = (win * cw).sum(axis=1)
    mag = (np.abs(win) * np.abs(cw)).sum(axis=1)
    return y.astype(x.dtype), mag.astype(np.float64)


def _pass(c, v, D, policy, reverse):
    """sum_k c[k] v[b(j + k - D)] (reverse: v[b(j - k + D)]) for every j, in WIDE"""
    N, W = len(v), len(c)
    vw = np.asarray(v).astype(WIDE)
    cw = np.asarray(c).astype(WIDE)
    out = np.zeros(N, WIDE)
    lo = -D if not reverse else D - (W - 1)
    tab = _index_table(lo, lo + N + W - 1, N, policy)  # b(lo + m)
    for k in range(W):
        m0 = k if not reverse else (W - 1 - k)  # index j + k - D = lo + j + k; j - k + D = lo + j + (W - 1 - k)
        out += cw[k] * vw[tab[m0:m0 + N]]
    return out


def zero_phase(coeffs, x, policy="Reflect"):
    """applyZeroPhase (:177-193) as two explicit passes; x's dtype is T.  Returns (out, t)."""
    x = np.asarray(x)
    c = np.asarray(coeffs)
    if len(x) == 0:
        return x.copy(), x.copy()
    D = (len(c) - 1) // 2
    t = _pass(c, x, D, policy, False).astype(x.dtype)
    out = _pass(c, t, D, policy, True).astype(x.dtype)
    return out, t


def apply_literal(c, v, policy):
    """apply (:156-172), Centred, plain loops"""
    N, W = len(v), len(c)
    D = (W - 1) // 2
    b = replicate_index if policy == "Replicate" else reflect_index
    out = np.zeros(N, v.dtype)
    for n in range(N):
        acc = WIDE(0)
        for k in range(W):
            acc += WIDE(c[k]) * WIDE(v[b(n + k - D, N)])
        out[n] = acc
    return out


def zero_phase_literal(coeffs, x, policy="Reflect"):
    """apply, reverse, apply, reverse (:184-192)"""
    x = np.asarray(x)
    if len(x) == 0:
        return x.copy()
    temp = apply_literal(coeffs, x, policy)[::-1].copy()
    return apply_literal(coeffs, temp, policy)[::-1].copy()
