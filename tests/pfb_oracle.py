"""float64 oracle of the polyphase filter bank (include/gr4hip.h, gr4hip_pfb_*; PFB.md).  The reference has no polyphase form, so this file IS the definition:

    s_m[j] = x[(m - P + 1) N + j]   (j < P N; x[n] = 0 for n < 0, or the carried history)
    u_m[i] = sum_{k < P} h[k N + i] s_m[k N + i]
    X_m[c] = sum_{i < N} u_m[i] e^{-2 pi i i c / N}

pfb is that in complex128, front_end_u32 the sums the way the kernels evaluate them (float32, k ascending from 0, one fma per term and component: exactly),
front_end_f32 those followed by a float64 transform, design the windowed-sinc prototype of gr4hip_pfb_design."""
import math

import numpy as np


def rel(y, t):
    """the parity formula of include/gr4hip.h: max_k |y_k - t_k| / max(|t_k|, rms(t))"""
    y, t = np.asarray(y).ravel(), np.asarray(t).ravel()
    rms = np.sqrt(np.mean(np.abs(t) ** 2))
    return float(np.max(np.abs(y - t) / np.maximum(np.abs(t), rms)))


def _frames(x, N, P, history, dtype):
    """[P - 1 + frames, N]: the P - 1 frames in front of x (zeros, or the last (P - 1) N samples of `history`), then x"""
    x = np.asarray(x, dtype).ravel()
    assert len(x) % N == 0
    past = np.zeros((P - 1) * N, dtype)
    if history is not None and P > 1:
        hh = np.asarray(history, dtype).ravel()[-(P - 1) * N:]
        past[len(past) - len(hh):] = hh
    return np.concatenate([past, x]).reshape(-1, N)


def pfb(h, x, N, P, history=None):
    """complex128 [frames, N]"""
    h = np.asarray(h, np.float64).reshape(P, N)
    f = _frames(x, N, P, history, np.complex128)
    M = len(f) - (P - 1)
    u = np.zeros((M, N), np.complex128)
    for k in range(P):
        u += h[k] * f[k:k + M]
    return np.fft.fft(u, axis=1)


def _fma32(h, s, u):
    """float32 fma(h, s, u), exactly: the product of two float32 is exact in float64; the float64 sum is rounded to odd (its error term from two-sum decides), and
    rounding that to float32 is then the single rounding of the exact value (53 >= 24 + 2 bits)"""
    p = h.astype(np.float64) * s.astype(np.float64)
    a = u.astype(np.float64)
    t = a + p
    bb = t - a
    err = (a - (t - bb)) + (p - bb)  # t + err = a + p exactly
    odd = (t.view(np.int64) & 1) == 1
    fix = (err != 0) & ~odd & np.isfinite(t)
    t = np.where(fix, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
    return t.astype(np.float32)


def front_end_u32(h, x, N, P, history=None):
    """the kernels' front end value for value: complex64 [frames, N], u = 0, then k ascending: fma(hk, sk, u) per component"""
    h = np.asarray(h, np.float32).reshape(P, N)
    f = _frames(x, N, P, history, np.complex64)
    M = len(f) - (P - 1)
    re = np.zeros((M, N), np.float32)
    im = np.zeros((M, N), np.float32)
    for k in range(P):
        s = f[k:k + M]
        hk = np.broadcast_to(h[k], (M, N))
        re = _fma32(hk, np.ascontiguousarray(s.real), re)
        im = _fma32(hk, np.ascontiguousarray(s.imag), im)
    return (re + 1j * im).astype(np.complex64)


def front_end_f32(h, x, N, P, history=None):
    """the float32 sums of the kernels (front_end_u32) followed by a float64 transform"""
    return np.fft.fft(front_end_u32(h, x, N, P, history).astype(np.complex128), axis=1)


def _bessel_i0(x):
    s, term, k = 1.0, 1.0, 1
    while True:
        term *= (x / 2) / k
        s += term * term
        k += 1
        if not term * term > s * np.finfo(np.float64).eps:
            return s


def window(name, n, beta=1.6):
    """gr4hip_window_create_f64's formulas through the C library's own cos (math.cos), value by value"""
    a = 2 * 3.14159265358979323846 / (n - 1)
    name = name.lower()
    if name in ("none", "rectangular"):
        return np.ones(n)
    if name == "hamming":
        return np.array([0.53836 - 0.46164 * math.cos(a * i) for i in range(n)])
    if name == "hann":
        return np.array([.5 - .5 * math.cos(a * i) for i in range(n)])
    if name == "blackman":
        return np.array([0.42 - 0.5 * math.cos(a * i) + 0.08 * math.cos(2. * (a * i)) for i in range(n)])
    if name == "kaiser":
        factor, i0b = 1.0 / (n - 1), _bessel_i0(beta)
        return np.array([_bessel_i0(beta * math.sqrt(abs(1.0 - ((2 * i) * factor - 1.0) ** 2))) / i0b for i in range(n)])
    raise ValueError(name)


def design(N, P, window_name="Hamming", beta=1.6):
    """h[j] = w_{PN}[j] sinc((j - (P N - 1) / 2) / N), float64 rounded once to float32"""
    L = N * P
    w = window(window_name, L, beta)
    mid = (L - 1) * 0.5
    h = np.empty(L, np.float32)
    for j in range(L):
        a = math.pi * ((j - mid) / N)
        h[j] = np.float32(w[j] * (1.0 if a == 0.0 else math.sin(a) / a))
    return h
