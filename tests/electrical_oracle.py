"""numpy restatement of gr::electrical::PowerFactor and SystemUnbalance (blocks/electrical/.../PowerEstimators.hpp:144-257) as gr4/electrical_ops.hpp states them:
every operation in the sample type (float32 / float64), in the order written; acos in float64 on the sample-type argument, rounded once.  Rows are [n_phases, n]."""
import itertools

import numpy as np

FLOATS = [np.float32, np.float64]


def specials(dtype):
    """the 14 special values of the issue's grid"""
    fi = np.finfo(dtype)
    return np.array([0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, fi.smallest_subnormal, 230.0, 232.3, 227.7], dtype=dtype)


def grid(dtype, n_rows):
    """the Cartesian grid of the special values over n_rows rows: [n_rows, 14 ** n_rows]"""
    sp = specials(dtype)
    return np.ascontiguousarray(np.array(list(itertools.product(sp, repeat=n_rows)), dtype=dtype).T)


def power_factor(P, S):
    """(power_factor, phase) (:166-176)"""
    P, S = np.asarray(P), np.asarray(S)
    T = P.dtype.type
    assert P.dtype == S.dtype and P.dtype.kind == "f"
    with np.errstate(all="ignore"):
        c = np.where(S != T(0), P / np.where(S != T(0), S, T(1)), T(0)).astype(T)  # (the guarded divisor only keeps numpy quiet: the quotient is unused there)
        c = np.where(c < T(-1), T(-1), np.where(T(1) < c, T(1), c)).astype(T)      # std::clamp: NaN and -0.0 pass through
        phase = np.arccos(c.astype(np.float64)).astype(T)
    return c, phase


def _sum(x):
    s = np.zeros(x.shape[1:], x.dtype)
    for row in x:
        s = s + row  # ((0 + x_0) + x_1) + ...
    return s


def _percent(dmax, avg):
    T = avg.dtype.type
    with np.errstate(all="ignore"):
        return np.where(avg > T(0), (dmax / avg) * T(100), T(0)).astype(T)


def total_power(P):
    with np.errstate(all="ignore"):
        return _sum(np.asarray(P))


def voltage_unbalance(x):
    """std::transform_reduce with std::max from T(0) as a left fold (:233-239)"""
    x = np.asarray(x)
    T = x.dtype.type
    with np.errstate(all="ignore"):
        avg = _sum(x) / T(x.shape[0])
        m = np.zeros_like(avg)
        for row in x:
            d = np.abs(row - avg)
            m = np.where(m < d, d, m)
    return _percent(m, avg)


def current_unbalance(x):
    """std::max_element with the comparator |a - avg| < |b - avg|, then |best - avg| (:242-247)"""
    x = np.asarray(x)
    T = x.dtype.type
    with np.errstate(all="ignore"):
        avg = _sum(x) / T(x.shape[0])
        best = x[0].copy()
        for row in x[1:]:
            best = np.where(np.abs(best - avg) < np.abs(row - avg), row, best)
        dmax = np.abs(best - avg)
    return _percent(dmax, avg)


def system_unbalance(U, I, P):
    """(P_total, U_unbalance, I_unbalance)"""
    return total_power(P), voltage_unbalance(U), current_unbalance(I)


def same_bits(a, b):
    """bit for bit, two NaNs equal whatever their payload"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.dtype(f"u{a.dtype.itemsize}")
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def ulp_distance(a, b):
    """ordered-integer distance in units in the last place (0 where both are NaN, inf where one is), exact for float64 too"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.dtype.kind == "f"
    it = np.dtype(f"i{a.dtype.itemsize}")

    def ordered(v):
        i = v.view(it).astype(np.int64)
        return np.where(i < 0, np.int64(np.iinfo(it).min) - i, i)
    oa, ob = ordered(a), ordered(b)
    hi, lo = np.maximum(oa, ob), np.minimum(oa, ob)
    d = (hi.view(np.uint64) - lo.view(np.uint64)).astype(np.float64)
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    return np.where(np.isnan(a) ^ np.isnan(b), np.inf, d)


def phase_inputs(dtype):
    """(P, S) whose quotients cover acos' domain: linspace(-1, 1), the five values either side of +-1, +-0, subnormals, clamped cases (|P| > |S|) and the 14 x 14 grid"""
    T = np.dtype(dtype).type
    fi = np.finfo(dtype)
    c = [np.linspace(-1, 1, 201).astype(dtype)]
    for edge in (T(1), T(-1)):
        lo = hi = edge
        for _ in range(5):
            lo, hi = np.nextafter(lo, T(-np.inf)), np.nextafter(hi, T(np.inf))
            c.append(np.array([lo, hi], dtype))
    c.append(np.array([0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, -fi.tiny / 2, fi.tiny, 1.0, -1.0, 3.0, -5.0, 1e30, -1e30], dtype))
    c = np.concatenate(c)
    P = [c, (c * T(2300)).astype(dtype), np.array([3, -5, 2300, -2301, 1, -0.0, 1, np.inf], dtype)]
    S = [np.ones_like(c), np.full_like(c, 2300), np.array([2, 2, -2299, 2300, fi.smallest_subnormal, 1, np.inf, np.inf], dtype)]
    g = grid(dtype, 2)
    return np.concatenate(P + [g[0]]), np.concatenate(S + [g[1]])


def wide_random(rng, shape, dtype, signed=False):
    """seeded magnitudes over 1e-30 ... 1e30 (for float32 as far as its range goes)"""
    x = 10.0 ** rng.uniform(-30, 30, shape)
    if signed:
        x = x * rng.choice([-1.0, 1.0], shape)
    with np.errstate(over="ignore", under="ignore"):
        return x.astype(dtype)


def graph_inputs(dtype, rng, n_random=200):
    """{P, S, U, I}, each [3, n]: what the graph tests feed.  P / S cover acos' domain (phase_inputs) in every row, U / I the 14^3 grid; all padded with wide-range
    random values to one length"""
    p, s = phase_inputs(dtype)
    g = grid(dtype, 3)
    n = max(p.size, g.shape[1]) + n_random

    def pad(rows, signed):
        return np.stack([np.concatenate([r, wide_random(rng, n - r.size, dtype, signed)]) for r in rows])
    perm = [np.arange(p.size), rng.permutation(p.size), rng.permutation(p.size)]
    P, S = pad([p[k] for k in perm], True), pad([s[k] for k in perm], False)
    U, I = pad(list(g), False), pad(list(g[::-1]), False)
    near = rng.uniform(0.9, 1.1, (3, n_random))  # realistic phases: a few percent apart
    U[:, -n_random:] = (230.0 * near).astype(dtype)
    I[:, -n_random // 2:] = (10.0 * near[:, :n_random // 2]).astype(dtype)
    return {"P": P, "S": S, "U": U, "I": I}
