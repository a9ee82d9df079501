"""numpy restatement of gr::electrical::PowerMetrics<float, nPhases> (blocks/electrical/.../PowerEstimators.hpp:21-131) for tests/test_*power_metrics*.py.

The coefficients are oracle_lib.iir_design(..., is_float=True): iir::designFilter<float> as initFilters calls it (:63-93).  Every filter is the plain
direct-form-II loop of Filter<float>::processOne (FilterTool.hpp:130-136) in a selectable dtype: float64 is the truth the device is held to, float32 is what
the reference's Filter<float> computes.  Decimation keeps the first sample of every chunk (:111); sqrt of a negative average and std::max(NaN, 0) give NaN."""
from __future__ import annotations

import numpy as np

import oracle_lib as O

NAMES = ("P", "Q", "S", "U_rms", "I_rms")


def coefficients(sample_rate=10000.0, high_pass=2.0, low_pass=90.0, decimate=100):
    """((b_hp, a_hp) or None for the identity (:73), (b_lp, a_lp)): float coefficients as float64 arrays of three values"""
    fs, hp, lp = (float(np.float32(v)) for v in (sample_rate, high_pass, low_pass))

    def one(resp, **kw):
        secs = O.iir_design(resp, O.filter_params(order=2, fs=fs, **kw), O.BUTTERWORTH, is_float=True)
        assert len(secs) == 1, secs
        b, a = (np.concatenate([np.asarray(v, np.float64), np.zeros(3)])[:3] for v in secs[0])
        return b, a

    hpc = one(O.HIGHPASS, fHigh=hp) if hp > 0.0 else None
    cutoff = min(0.5 * (fs / float(decimate)), lp)  # (:83), in double
    return hpc, one(O.LOWPASS, fLow=cutoff)


def biquad(b, a, x, dtype=np.float64, state=None):
    """direct form II: w = x - (a1 w1 + a2 w2), y = b0 w + b1 w1 + b2 w2, every operation rounded to dtype; `state` ([w1, w2]) is updated in place"""
    T = np.dtype(dtype).type
    n = len(x)
    y = np.empty(n, dtype)
    st = state if state is not None else [0.0, 0.0]
    with np.errstate(all="ignore"):
        if T is np.float64:  # python floats are IEEE doubles: the same arithmetic, faster
            b0, b1, b2 = (float(v) for v in b)
            a1, a2 = float(a[1]), float(a[2])
            w1, w2 = float(st[0]), float(st[1])
            out = [0.0] * n
            for k, xv in enumerate(np.asarray(x, np.float64).tolist()):
                w = xv - (a1 * w1 + a2 * w2)
                out[k] = b0 * w + b1 * w1 + b2 * w2
                w2 = w1
                w1 = w
            y[:] = out
        else:
            b0, b1, b2 = (T(v) for v in b)
            a1, a2 = T(a[1]), T(a[2])
            w1, w2 = T(st[0]), T(st[1])
            xs = np.asarray(x, dtype)
            for k in range(n):
                w = T(xs[k] - T(T(a1 * w1) + T(a2 * w2)))
                y[k] = T(T(T(b0 * w) + T(b1 * w1)) + T(b2 * w2))
                w2 = w1
                w1 = w
    st[0], st[1] = w1, w2
    return y


class Block:
    """one phase of the block with its five filter states: process(u, i) continues where the last call ended (n a multiple of decimate)"""

    def __init__(self, dtype=np.float64, sample_rate=10000.0, high_pass=2.0, low_pass=90.0, decimate=100):
        self.dtype = np.dtype(dtype).type
        self.decimate = int(decimate)
        self.hp, self.lp = coefficients(sample_rate, high_pass, low_pass, decimate)
        self.reset()

    def reset(self):
        self.st = [[0.0, 0.0] for _ in range(5)]

    def process(self, u, i):
        """dict of the five outputs and the three moving averages ema_p, ema_u2, ema_i2 at the kept samples (float64 arrays)"""
        T, D = self.dtype, self.decimate
        assert len(u) == len(i) and len(u) % D == 0
        u, i = np.asarray(u, np.float32).astype(T), np.asarray(i, np.float32).astype(T)
        if self.hp is not None:
            u = biquad(*self.hp, u, T, self.st[0])
            i = biquad(*self.hp, i, T, self.st[1])
        with np.errstate(all="ignore"):
            ep = biquad(*self.lp, u * i, T, self.st[2])[::D]
            eu = biquad(*self.lp, u * u, T, self.st[3])[::D]
            ei = biquad(*self.lp, i * i, T, self.st[4])[::D]
            ur, ir = np.sqrt(eu), np.sqrt(ei)
            S = ur * ir
            d = S * S - ep * ep
            Q = np.sqrt(np.where(d < 0, T(0), d))  # std::max(d, T(0)) = (d < 0) ? 0 : d: NaN stays
        f = lambda v: np.asarray(v, np.float64)
        return dict(P=f(ep), Q=f(Q), S=f(S), U_rms=f(ur), I_rms=f(ir), ema_p=f(ep), ema_u2=f(eu), ema_i2=f(ei))


def run(u, i, dtype=np.float64, **settings):
    """rows of u / i are phases: dict of [n_phases, n / decimate] arrays from freshly initialised filters"""
    u, i = np.atleast_2d(u), np.atleast_2d(i)
    rows = [Block(dtype, **settings).process(u[k], i[k]) for k in range(len(u))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def qa_signals(n=10000, fs=10000.0, n_phases=3, seed=42, f=50.0, v_rms=230.0, i_rms=10.0, noise=0.01, offset=1.0):
    """the reference QA's inputs (qa_PowerEstimators.cpp:28-70), in float as there: a 50 Hz system, phases shifted by 0, -2 pi / 3, +2 pi / 3, the current
    of phase k delayed by 0.1 (k + 1) rad, noise N(0, 1 %) of the peak on every sample, +offset on the voltages and -offset on the currents (numpy's
    generator for the noise)"""
    F = np.float32
    rng = np.random.default_rng(seed)
    t = np.arange(n).astype(F) / F(fs)
    vp, ip = F(v_rms) * F(np.sqrt(2.0)), F(i_rms) * F(np.sqrt(2.0))
    shift = [F(0), F(-2.0) * F(np.pi) / F(3), F(2.0) * F(np.pi) / F(3)]
    u = np.empty((n_phases, n), F)
    i = np.empty((n_phases, n), F)
    for k in range(n_phases):
        om = F(2) * F(np.pi) * F(f) * t
        nz = rng.normal(0.0, noise, (n, 2)).astype(F)
        u[k] = F(offset) + vp * (np.sin(om + shift[k % 3]) + nz[:, 0])
        i[k] = F(-offset) + ip * (np.sin(om + shift[k % 3] + F(0.1) * F(k + 1)) + nz[:, 1])
    return u, i
