"""Oracle of gr::basic::SignalGenerator<T> for the device source (include/gr4hip.h "Signal generator", SIGNAL_GENERATOR.md), in plain numpy and Python integers.

It restates, per sample as SignalGeneratorCore<T>::generateSample() does (SignalGeneratorCore.hpp:95-106):
  * the time base by SEQUENTIAL addition in the compute type F (ToneGenerator.hpp:224-225) -- `sequential_time` -- and, separately, the segment table that gives
    the same values in closed form -- `time_table` / `time_at`;
  * the tones (ToneGenerator.hpp:235-255, complex :77-102) in F, operation by operation; sin / cos / log of F = float32 are evaluated in float64 and rounded once;
  * FastSin / FastCos by the closed-form phasor model in float64 -- `phasor_model` -- which is what the device computes instead of the recurrence;
  * xoshiro256++ (Xoshiro256pp.hpp:32-66) with splitmix64 seeding, vectorised over lanes whose start states come from GF(2) matrix powers -- `draws`, `jump`;
  * Uniform, Triangular and Marsaglia-polar Gaussian noise with the cached second variate (NoiseGenerator.hpp, GaussianNoise.hpp:33-55).
`Generator` strings them together with the life cycle of the handle: configure re-seeds the noise, drops the spare, restarts the phasor and keeps the time running;
reset also zeroes the time."""
import math

import numpy as np

TYPES = ["Const", "Sin", "Cos", "Square", "Saw", "Triangle", "FastSin", "FastCos", "UniformNoise", "TriangularNoise", "GaussianNoise"]
CONST, SIN, COS, SQUARE, SAW, TRIANGLE, FAST_SIN, FAST_COS, UNIFORM, TRIANGULAR, GAUSSIAN = range(11)
NP_DTYPE = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "i16": np.int16}
MASK = (1 << 64) - 1


def compute_type(dtype: str):
    return np.float32 if dtype == "c32" else np.float64  # SignalGeneratorCore.hpp:27-41


# ---------------------------------------------------------------------------------------------- xoshiro256++
def seed_state(seed: int):
    s, v = [], seed & MASK
    for _ in range(4):  # splitmix64 (Xoshiro256pp.hpp:33-39)
        v = (v + 0x9e3779b97f4a7c15) & MASK
        z = v
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
        s.append(z ^ (z >> 31))
    return s


def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & MASK


def step(s):
    """one draw from the state s (a list of four Python integers, updated in place): Xoshiro256pp.hpp:41-52"""
    r = (_rotl((s[0] + s[3]) & MASK, 23) + s[0]) & MASK
    t = (s[1] << 17) & MASK
    s[2] ^= s[0]
    s[3] ^= s[1]
    s[1] ^= s[2]
    s[0] ^= s[3]
    s[2] ^= t
    s[3] = _rotl(s[3], 45)
    return r


_POW = []  # _POW[k][i] = the 256 bits of T^(2^k) applied to basis state i


def _bits(states) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(states, dtype=np.uint64).reshape(-1, 4))
    return np.unpackbits(a.view(np.uint8).reshape(-1, 32), axis=1, bitorder="little")


def _unbits(bits: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")).view(np.uint64).reshape(-1, 4)


def _pow2(k: int) -> np.ndarray:
    if not _POW:
        rows = []
        for i in range(256):
            s = [0, 0, 0, 0]
            s[i >> 6] = 1 << (i & 63)
            step(s)
            rows.append(s)
        _POW.append(_bits(rows).astype(np.float32))
    while len(_POW) <= k:
        m = _POW[-1]
        _POW.append(np.mod(m @ m, 2.0).astype(np.float32))
    return _POW[k]


def _matrix(n: int) -> np.ndarray:
    m = None
    for k in range(64):
        if (n >> k) & 1:
            m = _pow2(k) if m is None else np.mod(m @ _pow2(k), 2.0)
    return np.eye(256, dtype=np.float32) if m is None else m.astype(np.float32)


def jump(state, n: int):
    """the state n draws further on"""
    if n == 0:
        return [int(x) for x in state]
    b = _bits([state]).astype(np.float32)
    return [int(x) for x in _unbits(np.mod(b @ _matrix(n), 2.0))[0]]


def draws(state, n: int, lanes: int = 8192) -> np.ndarray:
    """the next n raw draws from `state` (not modified), lanes of consecutive draws stepped together"""
    if n == 0:
        return np.empty(0, np.uint64)
    per = -(-n // lanes)
    lanes = -(-n // per)
    st = np.zeros((lanes, 256), np.float32)
    st[0] = _bits([state])[0]
    have, m = 1, _matrix(per)
    while have < lanes:  # doubling: lanes [have, 2 have) are T^(per have) times lanes [0, have)
        take = min(have, lanes - have)
        st[have:have + take] = np.mod(st[:take] @ m, 2.0)
        have += take
        m = np.mod(m @ m, 2.0)
    s = _unbits(st).T.copy()
    s0, s1, s2, s3 = s[0], s[1], s[2], s[3]
    out = np.empty((per, lanes), np.uint64)

    def rotl(x, k):
        return (x << np.uint64(k)) | (x >> np.uint64(64 - k))
    with np.errstate(over="ignore"):
        for i in range(per):
            out[i] = rotl(s0 + s3, 23) + s0
            t = s1 << np.uint64(17)
            s2 = s2 ^ s0
            s3 = s3 ^ s1
            s1 = s1 ^ s2
            s0 = s0 ^ s3
            s2 = s2 ^ t
            s3 = rotl(s3, 45)
    return out.T.reshape(-1)[:n].copy()


def u01(raw: np.ndarray, F) -> np.ndarray:  # Xoshiro256pp.hpp:55-61
    if F == np.float32:
        return (raw >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return (raw >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)


# ---------------------------------------------------------------------------------------------- time
def sequential_time(F, tick, t0, count: int) -> np.ndarray:
    """count + 1 values t0, fl(t0 + tick), fl(fl(t0 + tick) + tick), ... in F: ufunc.accumulate adds strictly in order"""
    a = np.full(count + 1, tick, dtype=F)
    a[0] = t0
    return np.add.accumulate(a, dtype=F)


def time_table(F, tick, n=0, t=0.0, n_end=1 << 64):
    """segments (n0, a, b, scale): t_n = (a + (n - n0) b) scale for n0 <= n < the next n0.  Inside a binade the increment is constant after at most one settling step
    (a tie rounds to even, and the parity repeats from then on); the step past the binade's top is a real addition.  SIGNAL_GENERATOR.md "Time"."""
    F = np.dtype(F).type
    p = np.finfo(F).nmant + 1
    min_exp = np.finfo(F).minexp
    tick, t = F(tick), F(t)
    tab = []
    while n < n_end:
        a, ge, scale = 0, 0, 1.0
        if t > 0:
            e = max(math.frexp(float(t))[1] - 1, min_exp)
            ge = e - (p - 1)
            a = int(math.ldexp(float(t), -ge))
            scale = math.ldexp(1.0, ge)
        t1 = F(t + tick)
        if t1 == t:
            tab.append((n, a, 0, scale))
            break
        run = False
        if t > 0:
            top = F(math.ldexp(1.0, ge + p))
            t2 = F(t1 + tick)
            if t1 < top and t2 <= top and F(t1 - t) == F(t2 - t1):
                run = True
                inc = int(math.ldexp(float(F(t1 - t)), -ge))
                room = int(math.ldexp(float(F(top - t)), -ge))
                K = room // inc
                tab.append((n, a, inc, scale))
                n += K + 1
                t = F(F(math.ldexp(float(a + K * inc), ge)) + tick)
        if not run:
            tab.append((n, a, 0, scale))
            n += 1
            t = t1
    return tab


def time_at(tab, n) -> np.ndarray:
    """the table's t_n, as float64 (exact for either F)"""
    n = np.asarray(n, dtype=np.uint64)
    n0 = np.array([s[0] for s in tab], dtype=np.uint64)
    a = np.array([s[1] for s in tab], dtype=np.uint64)
    b = np.array([s[2] for s in tab], dtype=np.uint64)
    sc = np.array([s[3] for s in tab], dtype=np.float64)
    i = np.searchsorted(n0, n, side="right") - 1
    with np.errstate(over="ignore"):
        m = a[i] + (n - n0[i]) * b[i]
    return m.astype(np.float64) * sc[i]


# ---------------------------------------------------------------------------------------------- values
def _sin(x):
    return np.sin(x.astype(np.float64)).astype(x.dtype)


def _cos(x):
    return np.cos(x.astype(np.float64)).astype(x.dtype)


def _log(x):
    return np.log(x.astype(np.float64)).astype(x.dtype)


def phasor_model(F, frequency, sample_rate, phase, k) -> np.ndarray:
    """the phasor of samples k (counted from configure) as complex128: |rot|^(k mod 65536) exp(j (arg p0 + k arg rot)) on the constants initPhasor rounds to F
    (ToneGenerator.hpp:204-214); the magnitude starts at |p0| and at 1 after every renormalisation (:228-231)"""
    F = np.dtype(F).type
    pi2 = F(2) * F(np.pi)
    f, ph, tick = F(np.float32(frequency)), F(np.float32(phase)), F(F(1) / F(np.float32(sample_rate)))  # the settings are float
    w = np.array([pi2 * f * tick], dtype=F)
    rot = complex(float(_cos(w)[0]), float(_sin(w)[0]))
    p0 = complex(float(_cos(np.array([ph], dtype=F))[0]), float(_sin(np.array([ph], dtype=F))[0]))
    k = np.asarray(k, dtype=np.uint64)
    mag = np.where(k < 65536, abs(p0), 1.0) * abs(rot) ** (k & np.uint64(0xFFFF)).astype(np.float64)
    th = math.atan2(p0.imag, p0.real) + k.astype(np.float64) * math.atan2(rot.imag, rot.real)
    return mag * np.cos(th) + 1j * (mag * np.sin(th))


def to_int16(raw: np.ndarray) -> np.ndarray:  # SignalGeneratorCore.hpp:49-60
    return np.where(raw >= 32767.0, 32767.0, np.where(raw <= -32768.0, -32768.0, np.trunc(raw))).astype(np.int16)


class Generator:
    """the stream of one handle.  `table_time` takes the time from the segment table instead of the sequential additions (same values)."""

    def __init__(self, dtype: str, signal_type=SIN, sample_rate=1000.0, frequency=1.0, amplitude=1.0, offset=0.0, phase=0.0, seed=0, table_time=False):
        self.dtype, self.F = dtype, np.dtype(compute_type(dtype)).type
        self.table_time = table_time
        self.set = dict(signal_type=signal_type, sample_rate=sample_rate, frequency=frequency, amplitude=amplitude, offset=offset, phase=phase, seed=seed)
        self.reset()

    def configure(self, **settings):
        for k in settings:
            if k not in self.set:
                raise TypeError(k)
        if "sample_rate" in settings and np.float32(settings["sample_rate"]) != np.float32(self.set["sample_rate"]):
            self._tab = None
        self.set.update(settings)
        t = self.set["signal_type"]
        self.type = TYPES.index(t) if isinstance(t, str) else int(t)
        self.k = 0
        self.state = seed_state(int(self.set["seed"]))
        self.spare = None

    def reset(self):
        self.n, self.t = 0, self.F(0)
        self._tab, self._tab_n0 = None, 0
        self.configure()

    def _times(self, n):
        F = self.F
        tick = F(F(1) / F(np.float32(self.set["sample_rate"])))
        if self.table_time:
            if self._tab is None:
                self._tab = time_table(F, tick, self.n, self.t)
            ts = time_at(self._tab, np.arange(self.n, self.n + n + 1, dtype=np.uint64)).astype(F)
        else:
            ts = sequential_time(F, tick, self.t, n)
        self.t = ts[-1]
        self.n += n
        return ts[:-1]

    def _convert(self, re, im=None):
        if self.dtype == "c32":
            out = np.empty(len(re), np.complex64)
            out.real = re
            out.imag = im if im is not None else 0
            return out
        if self.dtype == "i16":
            return to_int16(re)
        return re.astype(NP_DTYPE[self.dtype])

    def _variates(self, count):
        """the next `count` Gaussian variates (GaussianNoise.hpp:33-55): attempt k is draws 2k and 2k + 1"""
        F = self.F
        out = []
        have = 0
        if self.spare is not None and count > 0:
            out.append(np.array([self.spare], dtype=F))
            self.spare = None
            have = 1
        while have < count:
            pairs = (count - have + 1) // 2
            att = int(pairs * 1.4) + 64
            r = draws(self.state, 2 * att)
            u = F(2) * u01(r[0::2], F) - F(1)
            v = F(2) * u01(r[1::2], F) - F(1)
            s = u * u + v * v
            ok = np.nonzero((s < 1) & (s != 0))[0][:pairs]
            s, u, v = s[ok], u[ok], v[ok]
            f = np.sqrt(F(-2) * _log(s) / s)
            g = np.empty(2 * len(ok), dtype=F)
            g[0::2] = u * f
            g[1::2] = v * f
            used = int(ok[-1]) + 1 if len(ok) else att
            self.state = jump(self.state, 2 * used)
            take = min(len(g), count - have)
            if take < len(g):
                self.spare = g[-1]
            out.append(g[:take])
            have += take
        return np.concatenate(out) if out else np.empty(0, F)

    def generate(self, n: int) -> np.ndarray:
        F, s = self.F, self.set
        f, A, O, ph = F(np.float32(s["frequency"])), F(np.float32(s["amplitude"])), F(np.float32(s["offset"])), F(np.float32(s["phase"]))
        cplx = self.dtype == "c32"
        typ = self.type
        if typ <= FAST_COS and f <= 0:
            typ = CONST  # ToneGenerator.hpp:48
        if typ <= FAST_COS:
            t = self._times(n)
            pi2 = F(2) * F(np.pi)
            k = np.arange(self.k, self.k + n, dtype=np.uint64)
            self.k += n
            if typ in (SIN, COS):
                theta = (pi2 * f) * t + ph
                sn, cs = _sin(theta), _cos(theta)
                return self._convert(A * sn + O, -A * cs) if typ == SIN else self._convert(A * cs + O, A * sn)
            if typ in (FAST_SIN, FAST_COS):
                p = phasor_model(F, s["frequency"], s["sample_rate"], s["phase"], k)
                a64, o64 = float(A), float(O)
                if typ == FAST_SIN:
                    return self._convert((a64 * p.imag + o64).astype(F), (-a64 * p.real).astype(F))
                return self._convert((a64 * p.real + o64).astype(F), (a64 * p.imag).astype(F))
            cycle = f * t + F(ph / pi2)
            if typ == SQUARE:
                return self._convert(np.where(cycle - np.floor(cycle) < F(0.5), A + O, -A + O).astype(F))
            if typ == SAW:
                return self._convert(A * (F(2) * (cycle - np.floor(cycle + F(0.5)))) + O)
            if typ == TRIANGLE:
                return self._convert(A * (F(4) * np.abs(cycle - np.floor(cycle + F(0.75)) + F(0.25)) - F(1)) + O)
            return self._convert(np.full(n, A + O, dtype=F))
        self.k += n
        comps = 2 if cplx else 1
        if typ == GAUSSIAN:
            g = self._variates(comps * n)
            if cplx:
                scale = F(1) / F(np.sqrt(2.0))
                return self._convert(A * (g[0::2] * scale) + O, A * (g[1::2] * scale))
            return self._convert(A * g + O)
        per = (2 if typ == TRIANGULAR else 1) * comps
        u = u01(draws(self.state, per * n), F)
        self.state = jump(self.state, per * n)
        if typ == UNIFORM:
            x = F(2) * u - F(1)
        else:
            x = u[0::2] + u[1::2] - F(1)
        if cplx:
            return self._convert(A * x[0::2] + O, A * x[1::2])
        return self._convert(A * x + O)
