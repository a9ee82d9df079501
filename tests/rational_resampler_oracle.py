"""float64 oracle of the rational resampler (include/gr4hip.h, gr4hip_resamp_*; RATIONAL_RESAMPLER.md).  The reference has no such block, so this file IS the definition:

    u[n] = x[n / L] if n % L == 0 else 0,    v[n] = L sum_{k < K} b[k] u[n - k],    y[j] = v[j M]        (real taps, zero initial history)

resamp64 is that, literally: the zero-stuffed stream, the full sum over all K taps, every M-th sample kept.  resamp64_poly / resamp32_seq are the evaluated form --
with Kp = ceil(K / L), output j = c L + p, o_p = floor(p M / L), phi_p = (p M) mod L, w_p[q] = float32(L) * b[q L + phi_p] (0 past the taps)

    y[c L + p] = sum_{q < Kp} w_p[q] x[c M + o_p - q]

-- in float64 and in float32 in the kernel's order (q ascending from 0, one fused multiply-add per term and component, the zero-padded terms included).  Every function
takes the carried history (the inputs in front of x, any length; zeros in front of those) and returns the one for the next call (the last Kp - 1 inputs)."""
import math

import numpy as np

import pfb_oracle as PO


def rel(y, t):
    """the parity formula of include/gr4hip.h: max |y - t| / max(|t|, rms(t))"""
    y, t = np.asarray(y, np.complex128), np.asarray(t, np.complex128)
    rms = np.sqrt(np.mean(np.abs(t) ** 2))
    return float(np.max(np.abs(y - t) / np.maximum(np.abs(t), rms))) if len(t) else 0.0


def _wide(x):
    return np.complex128 if np.iscomplexobj(x) else np.float64


def _with_hist(x, H, hist, dtype):
    """the H samples in front of x (zeros where hist is None or shorter), then x"""
    h = np.zeros(H, dtype)
    if hist is not None and H > 0:
        hh = np.asarray(hist, dtype)[-H:]
        if len(hh):
            h[H - len(hh):] = hh
    return np.concatenate([h, np.asarray(x, dtype)])


def branch_length(K, L):
    return -(-K // L)


def slots(L, M):
    """(o_p, phi_p) for p < L"""
    p = np.arange(L, dtype=np.int64)
    return p * M // L, p * M % L


def branch_taps(b, L, M):
    """w[q][p] = float32(L) * float32(b[q L + phi_p]) rounded once to float32; 0 where q L + phi_p >= K.  Shape [Kp][L]: the device's tap table"""
    b = np.asarray(b, np.float32)
    K, Kp = len(b), branch_length(len(b), L)
    _, phi = slots(L, M)
    w = np.zeros((Kp, L), np.float32)
    for q in range(Kp):
        k = q * L + phi
        ok = k < K
        w[q, ok] = np.float32(L) * b[k[ok]]
    return w


def resamp64(b, x, L, M, hist=None):
    """the literal definition in float64: zero-stuff, the full sum, keep every M-th.  Returns (y, new_hist)"""
    b = np.asarray(b, np.float64)
    K, H = len(b), branch_length(len(b), L) - 1
    dt = _wide(x)
    xx = _with_hist(x, H, hist, dt)
    n = len(xx) - H
    assert n % M == 0
    n_out = n // M * L
    off = (H + 1) * L  # u[off + t] = the L-times-rate stream at position t; K - 1 <= (H + 1) L - 1 positions in front of 0
    u = np.zeros(off + n * L, dt)
    u[L::L][:len(xx)] = xx  # position (i - H) L holds xx[i]
    # the sum walks u with stride M: u[s + j M] for all j is contiguous in row s % M; complex data as (re, im) pairs of float64, the taps are real
    c = 2 if dt is np.complex128 else 1
    rows = [np.ascontiguousarray(u[r::M]).view(np.float64) for r in range(M)]
    y, tmp = np.zeros(n_out * c), np.empty(n_out * c)
    for k0 in range(min(M, K)):  # y[j] += b[k] u[j M - k], all K terms; the taps that share a row one after the other (the row stays in the cache)
        for k in range(k0, K, M):
            s = off - k
            np.multiply(rows[s % M][s // M * c:(s // M + n_out) * c], b[k], out=tmp)
            y += tmp
    y = float(L) * y
    return y.view(dt) if c == 2 else y, xx[len(xx) - H:] if H else xx[:0]


def _gather(xx, H, L, M, n_cyc):
    """idx[c][p]: where x[c M + o_p] sits in xx = (H history samples, then x)"""
    o, _ = slots(L, M)
    return H + np.arange(n_cyc, dtype=np.int64)[:, None] * M + o[None, :]


def resamp64_poly(b, x, L, M, hist=None):
    """the evaluated form in float64, with the float32 branch taps widened (what the device multiplies by).  Returns (y, new_hist)"""
    w = branch_taps(b, L, M).astype(np.float64)
    Kp, H = len(w), len(w) - 1
    dt = _wide(x)
    xx = _with_hist(x, H, hist, dt)
    n = len(xx) - H
    assert n % M == 0
    idx = _gather(xx, H, L, M, n // M)
    y = np.zeros(idx.shape, dt)
    for q in range(Kp):
        y += w[q][None, :] * xx[idx - q]
    return y.ravel(), xx[len(xx) - H:] if H else xx[:0]


def _fma32(w, v, a):
    """fmaf(w, v, a) on float32 arrays: the product is exact in float64, the sum is rounded to 53 bits and then to 24 (equal to one rounding except on rare ties)"""
    return (w.astype(np.float64) * v.astype(np.float64) + a.astype(np.float64)).astype(np.float32)


def resamp32_seq(b, x, L, M, hist=None):
    """the evaluated form in float32 in the kernel's order: acc = 0; for q ascending: acc = fmaf(w_p[q], x[c M + o_p - q], acc), per component"""
    w = branch_taps(b, L, M)
    Kp, H = len(w), len(w) - 1
    cplx = np.iscomplexobj(x)
    xx = _with_hist(x, H, hist, np.complex64 if cplx else np.float32)
    n = len(xx) - H
    assert n % M == 0
    idx = _gather(xx, H, L, M, n // M)
    parts = [np.ascontiguousarray(xx.real), np.ascontiguousarray(xx.imag)] if cplx else [xx]
    accs = [np.zeros(idx.shape, np.float32) for _ in parts]
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Kp):
            wq = np.broadcast_to(w[q][None, :], idx.shape)
            for i, part in enumerate(parts):
                accs[i] = _fma32(wq, part[idx - q], accs[i])
    y = (accs[0] + 1j * accs[1]).astype(np.complex64) if cplx else accs[0]
    return y.ravel()


def impulse_response(b, L, M, i, n_in):
    """the exact output for a unit impulse at input i: y[c L + p] = w_p[c M + o_p - i] where that index is in [0, Kp), else 0 (products with 1 and 0 are exact)"""
    w = branch_taps(b, L, M)
    o, _ = slots(L, M)
    q = np.arange(n_in // M, dtype=np.int64)[:, None] * M + o[None, :] - i
    ok = (q >= 0) & (q < len(w))
    y = np.zeros(q.shape, np.float32)
    pp = np.broadcast_to(np.arange(L)[None, :], q.shape)
    y[ok] = w[q[ok], pp[ok]]
    return y.ravel()


def design(L, M, half_len, window_name="Hamming", beta=1.6):
    """gr4hip_resamp_design: K = 2 half_len max(L, M) + 1, fc = 0.4 / max(L, M), h[k] = w_K[k] 2 fc sinc(2 fc (k - (K - 1) / 2)), h / sum(h); float64 value by
    value through the C library's sin, summed in index order, rounded once to float32"""
    R = max(L, M)
    K = 2 * half_len * R + 1
    w = PO.window(window_name, K, beta)
    fc2 = 2.0 * (0.4 / R)
    mid = (K - 1) * 0.5
    h = []
    for k in range(K):
        a = math.pi * (fc2 * (k - mid))
        h.append((float(w[k]) * fc2) * (1.0 if a == 0.0 else math.sin(a) / a))
    s = 0.0
    for v in h:
        s = s + v
    return np.array([v / s for v in h], np.float64).astype(np.float32)
