"""numpy / scipy restatement of IQDemodulator<T> (blocks/filter/.../FrequencyEstimator.hpp:356-653) for tests/test_iq_demod_*.py.

  truth  -- float64 arithmetic with the coefficients the reference computes in T (initialiseFilters, :468-506; float exp through the C library's expf, as the
            block's host code calls it): scipy.signal.lfilter runs the high-passes and the low-passes, np.convolve the derivative, with the reference's
            history-size conditions (:548-555).  The low-pass states at every chunk end go through extract(), step 5 (:571-640) in float64.
  ref32  -- the reference's per-sample loop in T, in its order (short inputs only).

Both give (amplitude, phase, frequency) per chunk.  truth also gives the decision margins of every output: how far Pr, Pd, Px and max(|I|, |Q|) are from eps
(relative), the closest any asin argument of the frequency iteration came to +-1 and any Aitken denominator to eps, and how far a rounding-sized nudge of
the iteration moves its result."""
from __future__ import annotations

import ctypes
import math

import numpy as np
from scipy.signal import lfilter

F32 = np.float32
_libm = ctypes.CDLL("libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]

MARGIN = 1e-6  # a decision closer than this (relative) to its threshold is not asserted on


class Params:
    def __init__(self, dtype=np.float32, sample_rate=62.5e6, f_high_pass=100.0, f_low_pass=10000.0, phase_unit=0, invert_phase=False, derivative_method=0,
                 epsilon=1e-12, chunk=1024):
        self.dtype = np.dtype(dtype).type
        self.sample_rate, self.f_high_pass, self.f_low_pass = (float(F32(v)) for v in (sample_rate, f_high_pass, f_low_pass))
        self.phase_unit, self.invert_phase, self.derivative_method = int(phase_unit), bool(invert_phase), int(derivative_method)
        self.epsilon = float(self.dtype(epsilon))
        self.chunk = int(chunk)

    def kw(self):
        return dict(sample_rate=self.sample_rate, f_high_pass=self.f_high_pass, f_low_pass=self.f_low_pass, phase_unit=self.phase_unit,
                    invert_phase=self.invert_phase, derivative_method=self.derivative_method, epsilon=self.epsilon)

    def replace(self, **kw):
        d = dict(dtype=self.dtype, chunk=self.chunk, **self.kw())
        d.update(kw)
        return Params(**d)


def _exp(v, T):
    return T(_libm.expf(F32(v))) if T == np.float32 else T(math.exp(v))


def coefficients(p: Params):
    """initialiseFilters (:468-506) in T, widened: alpha_hp, alpha_lp, taps (tap[k] multiplies h_ref[n - k]), delay; and the extraction's T constants"""
    T = p.dtype
    pi = T(np.pi)
    fs = T(p.sample_rate)
    ahp = _exp(T(-2) * pi * T(p.f_high_pass) / fs, T)
    alp = T(1) - _exp(T(-2) * pi * T(p.f_low_pass) / fs, T)
    taps = [[T(1), T(0), T(-1)],
            [T(0.2), T(0.1), T(0), T(-0.1), T(-0.2)],
            [T(3) / T(28), T(2) / T(28), T(1) / T(28), T(0), T(-1) / T(28), T(-2) / T(28), T(-3) / T(28)]][p.derivative_method]
    return dict(ahp=float(ahp), alp=float(alp), taps=np.array([float(t) for t in taps]), d=p.derivative_method + 1, g0=2.0 if p.derivative_method == 0 else 1.0,
                g08=float(T(0.8)), g02=float(T(0.2)), pi=float(pi), fs=float(fs))


def lp_states(p: Params, ref, resp):
    """the five low-pass states {I, Q, Pr, Pd, Px} (float64) at the last sample of every chunk, from a freshly initialised block"""
    c = coefficients(p)
    n = len(ref)
    a, al, taps, d = c["ahp"], c["alp"], c["taps"], c["d"]
    hr = lfilter([a, -a], [1.0, -a], np.asarray(ref, np.float64))  # h[n] = a (h[n-1] + v[n] - v[n-1]), v[-1] = h[-1] = 0
    hx = lfilter([a, -a], [1.0, -a], np.asarray(resp, np.float64))
    rq = np.convolve(hr, taps)[:n]
    rq[:len(taps) - 1] = 0.0  # only once the history holds K values
    ri = np.concatenate([np.zeros(d), hr[:n - d]])[:n]  # 0 until d samples are in
    xi = np.concatenate([np.zeros(d), hx[:n - d]])[:n]
    del hr, hx
    ends = np.arange(p.chunk - 1, n, p.chunk)
    out = np.empty((5, len(ends)))
    for k, q in enumerate((lambda: xi * ri, lambda: xi * rq, lambda: ri * ri, lambda: rq * rq, lambda: xi * xi)):
        out[k] = lfilter([al], [1.0, -(1.0 - al)], q())[ends]  # s += al (p - s)
    return out


def _gain(p, c, om):
    if p.derivative_method == 0:
        return np.full_like(om, 2.0)
    cs = np.cos(om)
    if p.derivative_method == 1:
        return c["g08"] * cs + c["g02"]
    return (6.0 * cs * cs + 2.0 * cs - 1.0) / 7.0


def extract(p: Params, S):
    """step 5 (:571-640) in float64 on low-pass states S = (5, m): (amplitude, phase, frequency, margins)"""
    c = coefficients(p)
    I, Q, Pr, Pd, Px = S
    eps = p.epsilon
    with np.errstate(all="ignore"):
        amp = np.where((Pr > eps) & (Px > eps), np.sqrt(Px / Pr), 0.0)
        okf = (Pr > eps) & (Pd > eps)
        ratio = np.sqrt(np.where(okf, Pd / Pr, 0.0))
        edge = np.full(ratio.shape, np.inf)  # the closest any asin argument came to +-1, any Aitken denominator to eps (relative)

        def iterate(jitter):  # jitter: a relative nudge of every asin result, the size of an implementation's rounding
            def asin(v):
                edge[...] = np.minimum(edge, np.where(okf, np.abs(np.abs(v) - 1.0), np.inf))
                return np.arcsin(np.clip(v, -1.0, 1.0)) * (1.0 + jitter)
            om0 = asin(ratio / c["g0"])
            for _ in range(3):
                om1 = asin(ratio / _gain(p, c, om0))
                om2 = asin(ratio / _gain(p, c, om1))
                om3 = asin(ratio / _gain(p, c, om2))
                den = om3 - 2.0 * om2 + om1
                edge[...] = np.minimum(edge, np.where(okf, np.abs(np.abs(den) / eps - 1.0), np.inf))
                om0 = np.where(np.abs(den) > eps, om1 - (om2 - om1) ** 2 / den, om3)
            return om0
        om0 = iterate(0.0)
        # the iteration's own condition: where a rounding-sized nudge moves the result, the Aitken step has amplified it (|G| near 0, a tiny denominator)
        cond = np.where(okf, np.abs(iterate(1e-14) - om0) / np.maximum(np.abs(om0), 1e-300), 0.0)
        fr = np.where(okf, om0 * c["fs"] / (2.0 * c["pi"]), 0.0)
        okp = okf & ((np.abs(I) > eps) | (np.abs(Q) > eps))
        ph = np.where(okp, np.arctan2(Q, I * ratio), 0.0)
        if p.invert_phase:
            ph = -ph
        if p.phase_unit == 1:
            ph = ph * (180.0 / c["pi"])

        def rel(v):  # distance of a threshold decision from eps, relative; a NaN state decides exactly (every test fails)
            return np.where(np.isnan(v), np.inf, np.abs(v / eps - 1.0))
        m = dict(pr=rel(Pr), pd=rel(Pd), px=rel(Px), iq=rel(np.maximum(np.abs(I), np.abs(Q))),
                 asin=edge, cond=cond)
    decided = (m["pr"] > MARGIN) & (m["pd"] > MARGIN) & (m["px"] > MARGIN) & (m["iq"] > MARGIN) & (m["asin"] > MARGIN) & (m["cond"] < 1e-11)
    return amp, ph, fr, dict(m, decided=decided)


def truth(p: Params, ref, resp):
    """(amplitude, phase, frequency, margins) of a freshly initialised block over the whole input"""
    return extract(p, lp_states(p, ref, resp))


def plain_loop(p: Params, ref, resp):
    """the reference's per-sample loop in float64 with the T coefficients (the check of truth's vectorised form)"""
    c = coefficients(p)
    a, al, taps, d = c["ahp"], c["alp"], c["taps"], c["d"]
    K = len(taps)
    hs = [0.0, 0.0]
    vp = [0.0, 0.0]
    hist_r, hist_x = [], []
    s = [0.0] * 5
    out = []
    for i in range(len(ref)):
        v = (float(ref[i]), float(resp[i]))
        for k in range(2):
            hs[k] = a * (hs[k] + v[k] - vp[k])
            vp[k] = v[k]
        hist_r.insert(0, hs[0])
        hist_x.insert(0, hs[1])
        rq = sum(taps[k] * hist_r[k] for k in range(K)) if len(hist_r) >= K else 0.0
        ri = hist_r[d] if len(hist_r) > d else 0.0
        xi = hist_x[d] if len(hist_x) > d else 0.0
        del hist_r[8:], hist_x[8:]
        for k, q in enumerate((xi * ri, xi * rq, ri * ri, rq * rq, xi * xi)):
            s[k] += al * (q - s[k])
        if (i + 1) % p.chunk == 0:
            out.append(list(s))
    return extract(p, np.array(out).T.reshape(5, -1))


def ref32(p: Params, ref, resp):
    """the reference's loop and step 5 in T (float32 for a float block), one sample at a time: (amplitude, phase, frequency)"""
    T = p.dtype
    pi = T(np.pi)
    fs = T(p.sample_rate)
    a = _exp(T(-2) * pi * T(p.f_high_pass) / fs, T)
    al = T(1) - _exp(T(-2) * pi * T(p.f_low_pass) / fs, T)
    c = coefficients(p)
    taps = [T(t) for t in c["taps"]]
    K, d = len(taps), c["d"]
    eps = T(p.epsilon)
    hs, vp = [T(0), T(0)], [T(0), T(0)]
    hist_r, hist_x = [], []
    s = [T(0)] * 5
    amp, ph, fr = [], [], []

    def G(om):
        cs = T(np.cos(om))
        return T(2) if p.derivative_method == 0 else (T(0.8) * cs + T(0.2) if p.derivative_method == 1 else (T(6) * cs * cs + T(2) * cs - T(1)) / T(7))

    def asin(v):
        return T(np.arcsin(T(min(max(v, T(-1)), T(1)))))

    with np.errstate(all="ignore"):
        for i in range(len(ref)):
            v = (T(ref[i]), T(resp[i]))
            for k in range(2):
                hs[k] = T(a * T(T(hs[k] + v[k]) - vp[k]))
                vp[k] = v[k]
            hist_r.insert(0, hs[0])
            hist_x.insert(0, hs[1])
            rq = T(0)
            if len(hist_r) >= K:
                for k in range(K):
                    rq = T(rq + T(taps[k] * hist_r[k]))
            ri = hist_r[d] if len(hist_r) > d else T(0)
            xi = hist_x[d] if len(hist_x) > d else T(0)
            del hist_r[8:], hist_x[8:]
            for k, q in enumerate((xi * ri, xi * rq, ri * ri, rq * rq, xi * xi)):
                s[k] = T(s[k] + T(al * T(T(q) - s[k])))
            if (i + 1) % p.chunk:
                continue
            I, Q, Pr, Pd, Px = s
            amp.append(T(np.sqrt(Px / Pr)) if Pr > eps and Px > eps else T(0))
            f = T(0)
            if Pr > eps and Pd > eps:
                ratio = T(np.sqrt(Pd / Pr))
                om0 = asin(ratio / T(2 if p.derivative_method == 0 else 1))
                for _ in range(3):
                    om1 = asin(ratio / G(om0))
                    om2 = asin(ratio / G(om1))
                    om3 = asin(ratio / G(om2))
                    den = T(om3 - T(2) * om2 + om1)
                    om0 = T(om1 - T(om2 - om1) ** 2 / den) if abs(den) > eps else om3
                f = T(om0 * fs / (T(2) * pi))
            fr.append(f)
            q = T(0)
            if Pr > eps and Pd > eps and (abs(I) > eps or abs(Q) > eps):
                q = T(np.arctan2(Q, I * T(np.sqrt(Pd / Pr))))
            if p.invert_phase:
                q = -q
            if p.phase_unit == 1:
                q = T(q * (T(180) / pi))
            ph.append(q)
    return np.array(amp, np.float64), np.array(ph, np.float64), np.array(fr, np.float64)


def qa_signals(freq, fs, amp_ratio, phase_shift, dc, noise, n, dtype=np.float32, seed=42):
    """generateIQTestSignals (qa_FrequencyEstimator.cpp:202-214): sin(omega t) + dc + noise U(-0.5, 0.5), omega in T (numpy's generator for the noise)"""
    T = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    om = T(2) * T(np.pi) * T(freq) / T(fs)
    t = np.arange(n).astype(T)
    ref = np.sin(om * t) + T(dc) + T(noise) * rng.uniform(-0.5, 0.5, n).astype(T)
    resp = T(amp_ratio) * np.sin(om * t + T(phase_shift)) + T(dc) + T(noise) * rng.uniform(-0.5, 0.5, n).astype(T)
    return ref.astype(T), resp.astype(T)


def chirp(fs, f0, f1, sweep_s, amp_ratio, phase_shift, noise, dtype=np.float32, seed=42):
    """the 0.1-5 MHz linear sweep of qa_FrequencyEstimator.cpp:533-580 (phase accumulated in float64), and the true frequency per sample"""
    n = int(fs * sweep_s)
    t = np.arange(n) / fs
    f = f0 + (f1 - f0) * t / sweep_s
    ph = np.cumsum(2.0 * np.pi * f / fs)
    rng = np.random.default_rng(seed)
    ref = np.sin(ph) + noise * rng.uniform(-0.5, 0.5, n)
    resp = amp_ratio * np.sin(ph + phase_shift) + noise * rng.uniform(-0.5, 0.5, n)
    return ref.astype(dtype), resp.astype(dtype), f
