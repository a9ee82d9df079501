"""Plain numpy float64 restatement of gr::filter::SvdDenoiser<T> (blocks/filter/.../SvdDenoiser.hpp over algorithm/filter/SvdFilter.hpp).

The contract (SVD_DENOISER.md): every `hop` samples the last W samples (zeros before the stream's start) form the L x K Hankel matrix H[i][j] = w[i + j]; its
singular values go through computeEffectiveRank (SvdFilter.hpp:43-65) IN RealT ARITHMETIC; the anti-diagonal average of the rank-k approximation gives d[0..W),
and d[safe .. safe + hop) are the outputs of the hop.  The SVD itself is numpy's, in float64, whatever T: float inputs are exact in float64.

The oracle also says, per window, whether it is SETTLED: whether the answer is well defined beyond the reference's own knife edges (settled()).
"""
import numpy as np

REAL_OF = {"f32": np.float32, "f64": np.float64, "c32": np.float32, "c64": np.float64}
NUMPY_OF = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}
SIZE_MAX = 2**64 - 1


def defaults(dtype):
    eps = float(np.finfo(REAL_OF[dtype]).eps)
    return dict(window_size=64, hankel_rows=0, max_rank=SIZE_MAX, relative_threshold=eps, absolute_threshold=eps, energy_fraction=1.0, hop_fraction=0.25)


def derive(dtype, window_size=64, hankel_rows=0, hop_fraction=0.25, **_):
    """W, L, K, hop, delay, safe (SvdFilter.hpp:183, :174-176); the hop's product is evaluated in RealT."""
    R = REAL_OF[dtype]
    W = max(int(window_size), 2)
    L = W // 2 if hankel_rows == 0 else int(hankel_rows)
    K = W - L + 1
    hop = max(1, int(R(W) * R(hop_fraction)))
    delay = (W - 1) // 2
    safe = min(W - 1 - delay, W - hop if W > hop else 0)
    return dict(W=W, L=L, K=K, hop=hop, delay=delay, safe=safe)


def effective_rank(sigma, R, max_rank=SIZE_MAX, relative_threshold=None, absolute_threshold=None, energy_fraction=1.0):
    """computeEffectiveRank (:43-65) in the arithmetic of R, before the clamp to min(L, K).  The total is summed as libstdc++'s transform_reduce does for random
    access iterators: four at a time, (s0^2 + s1^2) + (s2^2 + s3^2) added to the running total, then the rest one by one."""
    s = np.asarray(sigma, dtype=np.float64).astype(R)
    if s.size == 0:
        return 0
    rel = R(np.finfo(R).eps if relative_threshold is None else relative_threshold)
    ab = R(np.finfo(R).eps if absolute_threshold is None else absolute_threshold)
    ef = R(energy_fraction)
    with np.errstate(all="ignore"):
        tot = R(0)
        i = 0
        while s.size - i >= 4:
            tot = R(tot + R(R(R(s[i] * s[i]) + R(s[i + 1] * s[i + 1])) + R(R(s[i + 2] * s[i + 2]) + R(s[i + 3] * s[i + 3]))))
            i += 4
        for j in range(i, s.size):
            tot = R(tot + R(s[j] * s[j]))
        cut = R(ef * tot)
        cum = R(0)
        rank = 0
        s0 = s[0]
        for v in s:
            if rank >= max_rank or R(v / s0) < rel or v < ab:
                break
            cum = R(cum + R(v * v))
            rank += 1
            if cum >= cut:
                break
    return max(rank, 1)


def _rule_args(settings):
    return {k: settings[k] for k in ("max_rank", "relative_threshold", "absolute_threshold", "energy_fraction") if k in settings}


def settled(sigma, L, K, **settings):
    """(a) the rank rule gives the same k in float32 and float64 arithmetic with the odd- and even-indexed sigma scaled independently by 1 - 1e-4, 1, 1 + 1e-4;
    (b) k = min(L, K), or sigma_k <= 1e-6 sigma_0, or sigma_{k-1} - sigma_k >= 1e-3 sigma_0.  All-zero windows are settled."""
    s = np.asarray(sigma, dtype=np.float64)
    if s[0] == 0.0:
        return True
    n = min(L, K)
    rule = _rule_args(settings)
    ks = set()
    for R in (np.float32, np.float64):
        for fe in (1 - 1e-4, 1.0, 1 + 1e-4):
            for fo in (1 - 1e-4, 1.0, 1 + 1e-4):
                t = s.copy()
                t[0::2] *= fe
                t[1::2] *= fo
                ks.add(min(effective_rank(t, R, **rule), n))
    if len(ks) != 1:
        return False
    k = ks.pop()
    return k == n or s[k] <= 1e-6 * s[0] or s[k - 1] - s[k] >= 1e-3 * s[0]


def low_rank_window(w, L, R, **settings):
    """d[0..W) of one window in float64 (hankelAverage of the rank-k approximation), k, sigma."""
    w = np.asarray(w)
    W = w.size
    K = W - L + 1
    H = w[np.arange(L)[:, None] + np.arange(K)[None, :]]
    U, s, Vh = np.linalg.svd(H, full_matrices=False)
    k = min(effective_rank(s, R, **_rule_args(settings)), min(L, K))
    Hk = (U[:, :k] * s[:k]) @ Vh[:k]
    d = np.zeros(W, dtype=Hk.dtype)
    cnt = np.zeros(W)
    idx = np.arange(L)[:, None] + np.arange(K)[None, :]
    np.add.at(d, idx, Hk)
    np.add.at(cnt, idx, 1.0)
    return d / cnt, k, s


class Result:
    """y: the outputs rounded to T; per window: start (index of its first output), k, settled, peak (max |x| of its window), sigma."""

    def __init__(self, y, windows, geom):
        self.y, self.windows, self.geom = y, windows, geom

    def unsettled(self):
        return sum(1 for w in self.windows if not w["settled"])

    def mask(self):
        """True for the outputs of settled windows."""
        m = np.zeros(self.y.size, dtype=bool)
        for w in self.windows:
            if w["settled"]:
                m[w["start"]:w["start"] + self.geom["hop"]] = True
        return m

    def peak(self):
        """per output: the peak |x| of its window"""
        p = np.zeros(self.y.size)
        for w in self.windows:
            p[w["start"]:w["start"] + self.geom["hop"]] = w["peak"]
        return p


def run(x, dtype, **settings):
    """The whole stream from a reset (zero pre-fill), processOne (:190-202) sample by sample."""
    s = defaults(dtype)
    s.update(settings)
    g = derive(dtype, **s)
    R = REAL_OF[dtype]
    T = NUMPY_OF[dtype]
    W, L, hop, safe = g["W"], g["L"], g["hop"], g["safe"]
    x = np.asarray(x).astype(T)
    wide = np.complex128 if np.iscomplexobj(x) else np.float64
    xp = np.concatenate([np.zeros(W - 1, dtype=wide), x.astype(wide)])
    y = np.zeros(x.size, dtype=T)
    windows = []
    for n in range(0, x.size, hop):
        w = xp[n:n + W]  # the last W samples ending at n inclusive
        peak = float(np.max(np.abs(w)))
        if not np.all(np.isfinite(w)):
            d = np.full(W, np.nan, dtype=wide)
            k, ok, sig = 0, True, None
        else:
            d, k, sig = low_rank_window(w, L, R, **s)
            ok = settled(sig, L, g["K"], **s)
        m = min(hop, x.size - n)
        with np.errstate(all="ignore"):
            y[n:n + m] = d[safe:safe + m].astype(T)
        windows.append(dict(start=n, k=k, settled=ok, peak=peak, sigma=sig))
    return Result(y, windows, g)


# ------------------------------------------------------------------ the inputs of the device tests (tests/test_gpu_svd_denoiser.py), generated in float32
def case_input(name, n, seed=2024):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    N = lambda: rng.standard_normal(n)
    if name == "A":
        x = np.sin(2 * np.pi * 0.05 * t) + 0.3 * N()
    elif name == "B":
        x = N()
    elif name == "C":
        x = np.sin(2 * np.pi * t / 8) + 0.5 * np.sin(2 * np.pi * t / 5.3) + 0.05 * N()
    elif name == "D":
        x = np.exp(2j * np.pi * t / 16) + 0.1 * (N() + 1j * N()) / np.sqrt(2)
        return x.astype(np.complex64)
    elif name == "E":
        x = t + 0.01 * N()
    elif name == "F":
        x = np.sin(2 * np.pi * t / 16) + 0.2 * N()
    elif name == "G":
        x = np.sin(2 * np.pi * t / 8) + 0.02 * N()
    elif name == "H":
        x = np.sin(2 * np.pi * t / 9) + 0.1 * N()
    else:
        raise KeyError(name)
    return x.astype(np.float32)


CASES = {  # name: (input, samples, dtypes, settings)
    "A": ("A", 1536, ("f32", "f64"), dict(window_size=64, max_rank=3, energy_fraction=0.95)),
    "B": ("B", 1536, ("f32", "f64"), dict()),
    "C": ("C", 700, ("f32", "f64"), dict(window_size=32, hankel_rows=8, hop_fraction=0.1, relative_threshold=0.1)),
    "D": ("D", 700, ("c32", "c64"), dict(window_size=32, max_rank=2, energy_fraction=0.95)),
    "E": ("E", 700, ("f32", "f64"), dict(window_size=4, max_rank=1)),
    "F": ("F", 700, ("f32", "f64"), dict(window_size=32, hop_fraction=0.75, energy_fraction=0.9)),
    "G": ("G", 700, ("f32", "f64"), dict(window_size=32, absolute_threshold=0.5)),
    "H": ("H", 700, ("f32", "f64"), dict(window_size=33, hankel_rows=5, hop_fraction=1.0, max_rank=2)),
    "I": ("A", 300, ("f32", "f64"), dict(window_size=2)),
    "Ic": ("D", 300, ("c32", "c64"), dict(window_size=2)),
    "J": ("C", 700, ("f32", "f64"), dict(window_size=128, hankel_rows=64, relative_threshold=0.1)),
    "K": ("D", 700, ("c32", "c64"), dict(window_size=64, max_rank=2, energy_fraction=0.95)),
}

_cache = {}


def case(name, dtype):
    """(x as T, Result): computed once and shared; callers leave both unchanged."""
    key = (name, dtype)
    if key not in _cache:
        inp, n, dtypes, settings = CASES[name]
        assert dtype in dtypes
        x = case_input(inp, n).astype(NUMPY_OF[dtype])
        x.setflags(write=False)
        r = run(x, dtype, **settings)
        r.y.setflags(write=False)
        _cache[key] = (x, r)
    return _cache[key]
