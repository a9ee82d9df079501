"""float64 oracle of the complex-tap FIR (include/gr4hip.h, gr4hip_cfir_*; COMPLEX_FIR.md).  The reference has no such block, so this file IS the definition:

    y[n] = sum_{k < K} b[k] x[n - k],   b, x complex;  decimate D: output m = y[m D];  zero initial history, the last K - 1 inputs carried across calls

cfir64 is the direct sum in complex128, cfir32_seq the same sum the way fir_filter evaluates it in complex64 (k ascending, acc = acc + b[k] * x[n - k], every complex
product as four real products), band_table / band_tile the realified band form the matrix-pipe kernel evaluates (the algebra of the issue, restated)."""
import numpy as np


def _with_hist(x, K, hist, dtype):
    """the K - 1 samples in front of x (zeros where hist is None or shorter), then x"""
    h = np.zeros(K - 1, dtype)
    if hist is not None and K > 1:
        hh = np.asarray(hist, dtype)[-(K - 1):]
        if len(hh):
            h[K - 1 - len(hh):] = hh
    return np.concatenate([h, np.asarray(x, dtype)])


def cfir64(b, x, D=1, hist=None):
    """complex128 direct sum; returns (y, new_hist) with new_hist the last K - 1 inputs"""
    b = np.asarray(b, np.complex128)
    K = len(b)
    xx = _with_hist(x, K, hist, np.complex128)
    n = len(xx) - (K - 1)
    assert n % D == 0
    y = np.zeros(n // D, np.complex128)
    for k in range(K):  # y[m] += b[k] x[m D - k]; x[j] sits at xx[K - 1 + j]
        y += b[k] * xx[K - 1 - k:K - 1 - k + n:D][:n // D]
    return y, xx[len(xx) - (K - 1):] if K > 1 else xx[:0]


def cfir32_seq(b, x, D=1, hist=None):
    """fir_filter's order in complex64: k ascending, acc = acc + b[k] * x[n - k]; products and sums rounded to float32 one by one (four real products, two sums per tap)"""
    b = np.asarray(b, np.complex64)
    K = len(b)
    xx = _with_hist(x, K, hist, np.complex64)
    n = len(xx) - (K - 1)
    assert n % D == 0
    m = n // D
    re, im = np.zeros(m, np.float32), np.zeros(m, np.float32)
    xr, xi = np.ascontiguousarray(xx.real), np.ascontiguousarray(xx.imag)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            s = slice(K - 1 - k, K - 1 - k + n, D)
            vr, vi = xr[s][:m], xi[s][:m]
            br, bi = np.float32(b[k].real), np.float32(b[k].imag)
            re = re + (br * vr - bi * vi)
            im = im + (br * vi + bi * vr)
    return (re + 1j * im).astype(np.complex64)


def _g(b, p, j):
    """g_p[j]: g_0[2k] = Re b[k], g_0[2k - 1] = -Im b[k], g_1[2k] = Re b[k], g_1[2k + 1] = +Im b[k]; 0 elsewhere"""
    K = len(b)
    if j < -1 or j > 2 * K - 1:
        return 0.0
    if j % 2 == 0:
        return b[j // 2].real
    k = (j + 1) // 2 if p == 0 else (j - 1) // 2
    if k < 0 or k >= K:
        return 0.0
    return -b[k].imag if p == 0 else b[k].imag


def band_steps(K, D):
    """(r_min, r_max) of the band form: floor(-(2K - 1) / 16) .. floor((14 D + 2) / 16)"""
    return (-(2 * K - 1)) // 16, (14 * D + 2) // 16


def band_table(b, D, dtype=np.float64):
    """A[r - r_min][i][u] = g_p[2 D io + p - (16 r + u)] with i = 2 io + p; returns (A, r_min)"""
    b = np.asarray(b)
    r_min, r_max = band_steps(len(b), D)
    A = np.zeros((r_max - r_min + 1, 16, 16), dtype)
    for r in range(r_min, r_max + 1):
        for i in range(16):
            io, p = i >> 1, i & 1
            for u in range(16):
                A[r - r_min, i, u] = _g(b, p, 2 * D * io + p - (16 * r + u))
    return A, r_min


def band_tile(b, x, D, o0, hist=None):
    """the 128 complex outputs o0 + 8 c + io of one 16 x 16 tile, Y = sum_r A_r B_r, B_r[u][c] = x'[2 D o0 + 16 (D c + r) + u] (float64)"""
    b = np.asarray(b, np.complex128)
    K = len(b)
    A, r_min = band_table(b, D)
    xx = _with_hist(x, K, hist, np.complex128)
    xp = np.empty(2 * len(xx))
    xp[0::2], xp[1::2] = xx.real, xx.imag
    off = 2 * (K - 1)  # x'[j] sits at xp[off + j]

    def at(j):
        j = np.asarray(j) + off
        ok = (j >= 0) & (j < len(xp))
        return np.where(ok, xp[np.clip(j, 0, len(xp) - 1)], 0.0)
    Y = np.zeros((16, 16))
    u, c = np.arange(16)[:, None], np.arange(16)[None, :]
    for r in range(r_min, r_min + len(A)):
        Y += A[r - r_min] @ at(2 * D * o0 + 16 * (D * c + r) + u)
    out = np.empty(128, np.complex128)
    for cc in range(16):
        for io in range(8):
            out[8 * cc + io] = Y[2 * io, cc] + 1j * Y[2 * io + 1, cc]
    return out


def rel(y, t):
    """the parity formula of include/gr4hip.h: max |y - t| / max(|t|, rms(t))"""
    y, t = np.asarray(y, np.complex128), np.asarray(t, np.complex128)
    rms = np.sqrt(np.mean(np.abs(t) ** 2))
    return float(np.max(np.abs(y - t) / np.maximum(np.abs(t), rms))) if len(t) else 0.0
