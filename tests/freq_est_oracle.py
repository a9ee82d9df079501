"""numpy restatement of FrequencyEstimatorTimeDomain<float> / FrequencyEstimatorFrequencyDomain<float> (blocks/filter/.../FrequencyEstimator.hpp:30-351) for
tests/test_freq_est_*.py.  The pinned pieces come from oracle_lib (iir_design BESSEL, iir_cascade, window, fft32, magnitude).  Two evaluations of each method:

  truth  -- float64 arithmetic throughout (the biquad with the float block's coefficients, the window sums, a windowed DFT of the needed bins);
  ref32  -- the reference's float32 arithmetic in its order (DF-I in float32, newest-first float32 sums, float32 FFT magnitudes; frequency domain only where
            the test asks for it: one FFT per output).

Every evaluation returns (outputs, raw, valid): the forward-filled outputs, the raw estimate per output, and whether the reference's checks passed there, plus the
decision margins the parity tests assert on."""
from __future__ import annotations

import numpy as np

import oracle_lib as O

F32 = np.float32


class Params:
    def __init__(self, method: int, sample_rate=1e3, f_min=40.0, f_expected=50.0, f_max=60.0, epsilon=1e-8, n_periods=4, min_fft_size=256, chunk=1):
        self.method = method
        self.sample_rate, self.f_min, self.f_expected, self.f_max, self.epsilon = (float(F32(v)) for v in (sample_rate, f_min, f_expected, f_max, epsilon))
        self.n_periods, self.min_fft_size, self.chunk = int(n_periods), int(min_fft_size), int(chunk)

    def kw(self):
        k = dict(sample_rate=self.sample_rate, f_min=self.f_min, f_expected=self.f_expected, f_max=self.f_max, epsilon=self.epsilon)
        k["n_periods" if self.method == 0 else "min_fft_size"] = self.n_periods if self.method == 0 else self.min_fft_size
        return k


def _per(p: Params) -> float:
    fs, fmin, fexp = F32(p.sample_rate), F32(p.f_min), F32(p.f_expected)
    return float(fs / min(fmin, fexp)) if fmin > 0 else float(fs / fexp)  # float division (:72, :232)


def geometry(p: Params):
    """(W, i_min, i_max) as the reference computes them, float-rounded"""
    if p.method == 0:
        return p.n_periods * int(_per(p)), 0, 0
    m = max(p.min_fft_size, int(_per(p)))
    N = 1 << max(0, (m - 1).bit_length())
    scaled = F32(N // 2) * F32(2)
    fs = F32(p.sample_rate)
    a = int(np.floor(F32(F32(p.f_min) / fs) * scaled))
    b = int(np.ceil(F32(F32(p.f_max) / fs) * scaled))
    half = N // 2
    return N, min(max(a, 1), half - 1), min(max(b, 1), half - 1)


def biquad(p: Params):
    """iir::designFilter<float, 0UZ>(LOWPASS, order 2, f_max, BESSEL) (:77): an order-2 prototype is one conjugate pole pair, so the restatement's single
    section is the single coefficient set"""
    secs = O.iir_design(O.LOWPASS, O.filter_params(order=2, fLow=float(p.f_max), fs=float(p.sample_rate)), O.BESSEL, is_float=True)
    assert len(secs) == 1
    b, a = secs[0]
    return np.asarray(b, np.float32), np.asarray(a, np.float32)


def fill(raw, valid, prev):
    """every output that failed a check repeats the previous output"""
    raw = np.asarray(raw, np.float64)
    idx = np.where(valid, np.arange(len(raw)), -1)
    last = np.maximum.accumulate(idx) if len(idx) else idx
    return np.where(last >= 0, raw[np.maximum(last, 0)], prev)


# ------------------------------------------------------------------------------------------------ time domain
def td_filter(p: Params, x, f64=True):
    b, a = biquad(p)
    if f64:
        return O.iir_cascade(O.make_sections([(b.astype(np.float64), a.astype(np.float64))]), x, form=O.DF_I, f64=True)
    return td_filter_f32(b, a, x)


def td_filter_f32(b, a, x):
    """processOne's DF-I in float32, its order: inner_product(b, x-history) - inner_product(a[1:], y-history)"""
    x = np.asarray(x, np.float32)
    y = np.zeros(len(x), np.float32)
    x1 = x2 = y1 = y2 = F32(0)
    for n in range(len(x)):
        ff = F32(F32(F32(F32(0) + F32(b[0] * x[n])) + F32(b[1] * x1)) + F32(b[2] * x2))
        fb = F32(F32(F32(0) + F32(a[1] * y1)) + F32(a[2] * y2))
        yn = F32(ff - fb)
        y[n] = yn
        x2, x1, y2, y1 = x1, x[n], y1, yn
    return y


def td_sums64(p: Params, y, W, positions):
    """B, C (float64) of the windows ending at `positions` (indices into y, each >= W - 1), and the smallest |4 y| / eps of the terms used"""
    y = np.asarray(y, np.float64)
    n = len(y)
    yc = np.concatenate([[0.0], y, [0.0]])
    s = yc[:-2] + yc[2:]  # y[q-1] + y[q+1] at q = 0 .. n-1
    use = ~(np.abs(4.0 * y) < p.epsilon)
    tb = np.where(use, y * y, 0.0).astype(np.longdouble)
    tc = np.where(use, 0.5 * s * s, 0.0).astype(np.longdouble)
    cb = np.concatenate([[0.0], np.cumsum(tb)]).astype(np.longdouble)
    cc = np.concatenate([[0.0], np.cumsum(tc)]).astype(np.longdouble)
    pos = np.asarray(positions)
    lo, hi = pos - W + 2, pos  # terms q in [lo, hi)
    lo = np.minimum(lo, hi)
    B = np.asarray(cb[hi] - cb[lo], np.float64)
    C = np.asarray(cc[hi] - cc[lo], np.float64)
    return B, C


def td_truth(p: Params, x, prev=None, y=None):
    """outputs for one call from a fresh (reset) state: (out, raw, valid, margins)"""
    W, _, _ = geometry(p)
    x = np.asarray(x, np.float32)
    if y is None:
        y = td_filter(p, x, True)
    C_ = p.chunk
    nout = len(x) // C_
    pos = (np.arange(nout) + 1) * C_ - 1
    ok = pos >= W - 1
    raw = np.zeros(nout)
    valid = np.zeros(nout, bool)
    margins = dict(b_over_eps=np.inf, z_to_edge=np.inf, y_over_eps=np.inf)
    if ok.any():
        B, Cs = td_sums64(p, y, W, pos[ok])
        z = Cs / B - 1.0
        good = (B > p.epsilon) & ~((z >= 1) | (z <= -1))
        r = np.where(good, p.sample_rate / (4 * np.pi) * np.arccos(np.clip(z, -1, 1)), 0.0)
        raw[ok] = r
        valid[ok] = good
        margins["b_over_eps"] = float(np.min(B / p.epsilon))
        margins["z_to_edge"] = float(np.min(1 - np.abs(z)))
        used = y[max(0, int(pos[ok][0]) - W + 1):]
        margins["y_over_eps"] = float(np.min(np.abs(np.abs(4 * used) / p.epsilon - 1))) if len(used) else np.inf
    out = fill(raw, valid, p.f_expected if prev is None else prev)
    return out, raw, valid, margins


def td_ref32(p: Params, x, prev=None, outputs=None):
    """the reference's float32 arithmetic, sample by sample in its order (small inputs; outputs: the output indices to evaluate, default all)"""
    W, _, _ = geometry(p)
    b, a = biquad(p)
    y = td_filter_f32(b, a, x)
    eps = F32(p.epsilon)
    nout = len(x) // p.chunk
    raw = np.zeros(nout, np.float32)
    valid = np.zeros(nout, bool)
    for m in (range(nout) if outputs is None else outputs):
        pidx = (m + 1) * p.chunk - 1
        if pidx < W - 1:
            continue
        d = y[pidx - np.arange(W)]  # newest first
        aB = aC = F32(0)
        for i in range(1, W - 1):
            den = F32(4) * d[i]
            if abs(den) < eps:
                continue
            sn = F32(d[i - 1] + d[i + 1])
            an = F32(F32(sn * sn) / den)
            aB = F32(aB + F32(d[i] * d[i]))
            aC = F32(aC + F32(F32(F32(2) * an) * d[i]))
        if aB <= eps:
            continue
        z = F32(F32(aC / aB) - F32(1))
        if z >= 1 or z <= -1:
            continue
        raw[m] = F32(F32(F32(p.sample_rate) / F32(F32(4) * F32(np.pi))) * F32(np.arccos(z)))
        valid[m] = True
    return fill(raw, valid, p.f_expected if prev is None else prev), raw, valid


# ------------------------------------------------------------------------------------------------ frequency domain
def fd_bins(p: Params):
    N, a, b = geometry(p)
    lo, hi = (a - 1, b) if a < b else (b - 1, b + 1)
    return N, a, b, lo, hi


def fd_mag64(p: Params, x, positions):
    """|X_k| 2 / N, float64, of the Hann-windowed newest-first window ending at each position (>= N - 1), bins lo .. hi: [len(positions), nbins]"""
    N, a, b, lo, hi = fd_bins(p)
    x = np.asarray(x, np.float64)
    i = np.arange(N)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * i / (N - 1))
    pos = np.asarray(positions)
    L = len(x) + N
    nfft = 1 << (L - 1).bit_length()
    Xf = np.fft.fft(x, nfft)
    out = np.empty((len(pos), hi - lo + 1))
    for c, k in enumerate(range(lo, hi + 1)):
        h = w * np.exp(-2j * np.pi * k * i / N)  # X_k(p) = sum_i h[i] x[p - i]: a convolution
        yk = np.fft.ifft(Xf * np.fft.fft(h, nfft))
        out[:, c] = np.abs(yk[pos]) * 2.0 / N
    return out


def fd_decide(p: Params, mags):
    """the reference's peak search and Gaussian interpolation on magnitudes [n, nbins] of bins lo .. hi (float64): raw, valid, margins"""
    N, a, b, lo, hi = fd_bins(p)
    mags = np.atleast_2d(mags)
    n = mags.shape[0]
    m = dict(top2=np.inf, delta_to_1=np.inf, den_over_eps=np.inf)
    if a < b:
        seg = mags[:, a - lo:b - lo]
        k = a + np.argmax(seg, axis=1)  # first maximum
        if seg.shape[1] > 1:
            s2 = np.sort(seg, axis=1)
            m["top2"] = float(np.min((s2[:, -1] - s2[:, -2]) / s2[:, -1]))
    else:
        k = np.full(n, b)
    valid = (k != 0) & (k < N // 2 - 1)
    kc = np.clip(k, lo + 1, hi - 1)
    r = np.arange(n)
    sm, s0, sp = mags[r, kc - 1 - lo], mags[r, kc - lo], mags[r, kc + 1 - lo]
    fin = np.isfinite(sm) & np.isfinite(s0) & np.isfinite(sp) & (sm > 0) & (s0 > 0) & (sp > 0)
    valid &= fin
    with np.errstate(all="ignore"):
        lm, l0, lp = np.log(np.where(fin, sm, 1)), np.log(np.where(fin, s0, 1)), np.log(np.where(fin, sp, 1))
        den = 2 * l0 - lm - lp
        if valid.any():
            m["den_over_eps"] = float(np.min(np.abs(np.abs(den[valid]) / p.epsilon - 1)))
        valid &= np.isfinite(den) & ~(np.abs(den) < p.epsilon)
        d = 0.5 * (lp - lm) / den
        if valid.any():
            m["delta_to_1"] = float(np.min(np.abs(1 - np.abs(d[valid]))))
        valid &= np.isfinite(d) & ~(np.abs(d) >= 1)
        raw = np.where(valid, (k + d) * p.sample_rate / N, 0.0)
    return raw, valid, m


def fd_mag64_direct(p: Params, x, positions):
    """fd_mag64 by one float64 FFT per window (a few positions of a long N)"""
    N, a, b, lo, hi = fd_bins(p)
    x = np.asarray(x, np.float64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / (N - 1))
    return np.array([np.abs(np.fft.fft(x[q - np.arange(N)] * w)[lo:hi + 1]) * 2.0 / N for q in positions])


def fd_truth(p: Params, x, prev=None, only=None):
    """outputs for one call from a fresh state.  only: output indices to evaluate (the others count as settling / invalid) -- for long N"""
    N, *_ = fd_bins(p)
    x = np.asarray(x, np.float32)
    nout = len(x) // p.chunk
    pos = (np.arange(nout) + 1) * p.chunk - 1
    ok = pos >= N - 1
    if not np.isfinite(x).all():  # a window that holds a non-finite sample: non-finite magnitudes in the reference's FFT
        cb = np.concatenate([[0], np.cumsum(~np.isfinite(x))])
        ok &= (cb[pos + 1] - cb[np.maximum(pos - N + 1, 0)]) == 0
    if only is not None:
        sel = np.zeros(nout, bool)
        sel[only] = True
        ok &= sel
    raw = np.zeros(nout)
    valid = np.zeros(nout, bool)
    margins = dict(top2=np.inf, delta_to_1=np.inf, den_over_eps=np.inf)
    if ok.any():
        xs = np.where(np.isfinite(x), x, 0.0)
        mags = fd_mag64(p, xs, pos[ok]) if only is None else fd_mag64_direct(p, xs, pos[ok])
        r, v, margins = fd_decide(p, mags)
        raw[ok] = r
        valid[ok] = v
    return fill(raw, valid, p.f_expected if prev is None else prev), raw, valid, margins


def fd_ref32(p: Params, x, prev=None, outputs=None):
    """the reference's float32 arithmetic for the outputs listed (default all): float32 window, float32 FFT, half-spectrum float32 magnitude"""
    N, a, b = geometry(p)
    x = np.asarray(x, np.float32)
    w = O.window(3, N, np.float32)
    nout = len(x) // p.chunk
    raw = np.zeros(nout, np.float32)
    valid = np.zeros(nout, bool)
    for m in (range(nout) if outputs is None else outputs):
        q = (m + 1) * p.chunk - 1
        if q < N - 1:
            continue
        d = x[q - np.arange(N)] * w
        S = O.magnitude(O.fft32(d.astype(np.complex64)), half=True).astype(np.float32)
        k = b if a >= b else a + int(np.argmax(S[a:b]))
        if k == 0 or k >= N // 2 - 1:
            continue
        sm, s0, sp = S[k - 1], S[k], S[k + 1]
        if not np.isfinite([sm, s0, sp]).all() or min(sm, s0, sp) <= 0:
            continue
        lm, l0, lp = np.log(sm), np.log(s0), np.log(sp)
        den = F32(F32(F32(2) * l0) - lm) - lp
        if not np.isfinite(den) or abs(den) < F32(p.epsilon):
            continue
        dk = F32(F32(0.5) * F32(lp - lm)) / den
        if not np.isfinite(dk) or abs(dk) >= 1:
            continue
        raw[m] = F32(F32(F32(k) + dk) * F32(p.sample_rate)) / F32(N)
        valid[m] = True
    return fill(raw, valid, p.f_expected if prev is None else prev), raw, valid


# ------------------------------------------------------------------------------------------------ inputs
def qa_signal(f: float, fs: float, noise: float, n: int) -> np.ndarray:
    """generateTestSignal of qa_FrequencyEstimator.cpp: float phase accumulator, std::mt19937(42) + uniform_real_distribution<float>(-0.5, 0.5)"""
    draws = np.random.RandomState(42).randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.float32)
    u = np.minimum(draws / F32(2 ** 32), np.nextafter(F32(1), F32(0)))
    dist = (u * F32(1) + F32(-0.5)).astype(np.float32)
    inc = F32(F32(F32(2) * F32(np.pi)) * F32(f)) / F32(fs)
    phase = np.cumsum(np.full(n, inc, np.float32), dtype=np.float32)
    return (np.sin(phase).astype(np.float32) + F32(noise) * dist).astype(np.float32)


def tone(f: float, fs: float, n: int, noise=0.01, seed=1, amp=1.0, phase0=0.3) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    return (amp * np.sin(2 * np.pi * f / fs * t + phase0) + noise * rng.standard_normal(n)).astype(np.float32)


def rel_err(got, truth):
    """the parity contract's normalisation (include/gr4hip.h): |y - t| / max(|t|, rms(t))"""
    got = np.asarray(got, np.float64)
    truth = np.asarray(truth, np.float64)
    rms = np.sqrt(np.mean(truth ** 2)) if len(truth) else 1.0
    return np.abs(got - truth) / np.maximum(np.abs(truth), rms)
