"""The SignalGenerator oracle (tests/signal_generator_oracle.py) against the reference's own SignalGeneratorCore<T> -- tests/golden/signal_generator_reference.npz,
200 000 samples of four sample types and eleven signal types at the parameters of tests/golden/make_signal_fixture.py -- and the segment table of the time base
against plain sequential addition.  No device."""
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as O
import signal_generator_oracle as SG

N = 200_000
CASES = {"f32": (1.5, 0.25), "f64": (1.5, 0.25), "i16": (30000.0, 9000.0), "c32": (1.5, 0.25)}
EXACT = (SG.CONST, SG.SQUARE, SG.SAW, SG.TRIANGLE, SG.UNIFORM, SG.TRIANGULAR)
# Sin, Cos, Gaussian: the bounds tests/test_host_cpp.py::test_signal_generator_is_the_reference_core keeps for this fixture
BOUND = {"f32": 4e-6, "c32": 4e-6, "f64": 1e-12, "i16": 1}
# FastSin, FastCos: the closed-form model against the reference's recurrence over these 200 000 samples, twice the deviation measured for the model (1.2e-4 for
# complex<float>, 6.3e-12 for double: the recurrence's own rounding walk); the margin covers another libm.  float and int16 are rounded from the double value.
BOUND_FAST = {"c32": 2.5e-4, "f64": 1.3e-11, "f32": 4e-6, "i16": 1}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(O.ROOT, "tests", "golden", "signal_generator_reference.npz"))


def fixture_generator(dtype, t, **kw):
    amp, off = CASES[dtype]
    return SG.Generator(dtype, signal_type=t, sample_rate=1000.0, frequency=37.5, amplitude=amp, offset=off, phase=0.3, seed=12345, **kw)


def bound_for(dtype, t):
    return BOUND_FAST[dtype] if t in (SG.FAST_SIN, SG.FAST_COS) else BOUND[dtype]


@pytest.mark.parametrize("dtype", list(CASES))
@pytest.mark.parametrize("t", range(11))
def test_oracle_reproduces_the_reference_fixture(fx, dtype, t):
    got = fixture_generator(dtype, t).generate(N)
    assert got.dtype == SG.NP_DTYPE[dtype] and got.shape == (N,)
    idx = fx["index"]
    err = np.abs(got[idx].astype(np.complex128) - fx[f"{dtype}_{t}"].astype(np.complex128)).max()
    print(f"{dtype} {SG.TYPES[t]}: max |oracle - reference| at the fixture's positions {err:.3e}")
    if t in EXACT:
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(fx[f"{dtype}_{t}_sha256"]), (dtype, t, err)
    else:
        assert err <= bound_for(dtype, t), (dtype, t, err)


@pytest.mark.parametrize("F,tick,steps", [(np.float32, np.float32(1) / np.float32(1000), 3_000_000), (np.float32, np.float32(1) / np.float32(48000), 3_000_000),
                                          (np.float32, np.float32(0.25), 3_000_000), (np.float32, np.float32(0.375 * 2.0 ** -10), 3_000_000),
                                          (np.float64, 1.0 / 1000.0, 400_000)])
def test_segment_table_is_sequential_addition(F, tick, steps):
    tab = SG.time_table(F, tick, n_end=steps + 1)
    want = SG.sequential_time(F, tick, 0, steps)
    got = SG.time_at(tab, np.arange(steps + 1)).astype(F)
    assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])
    print(f"tick {float(tick):.6g} ({np.dtype(F).name}): {len(tab)} segments for {steps} steps")


def test_segment_table_at_every_boundary_up_to_the_stall():
    """F = float, tick 1 / 1000: 1000 steps on either side of every segment boundary up to n = 2^25 -- the stall near 2^24 included -- walked sequentially from the
    table's own value"""
    F, tick = np.float32, np.float32(1) / np.float32(1000)
    tab = SG.time_table(F, tick)
    assert tab[-1][2] == 0 and tab[-1][0] < 1 << 25, tab[-1]  # the last segment is the stall, and it starts below 2^25
    bounds = [s[0] for s in tab if s[0] <= 1 << 25] + [1 << 25]
    for nb in bounds:
        lo = max(nb - 1000, 0)
        t0 = F(SG.time_at(tab, [lo])[0])
        want = SG.sequential_time(F, tick, t0, nb + 1000 - lo)
        got = SG.time_at(tab, np.arange(lo, nb + 1001)).astype(F)
        assert np.array_equal(got, want), (nb, int(np.nonzero(got != want)[0][0]))
    stall = tab[-1][0]
    ts = SG.time_at(tab, [stall, stall + 1, 1 << 40]).astype(F)
    assert ts[0] == ts[1] == ts[2] and F(ts[0] + tick) == ts[0]
    print(f"{len(tab)} segments; the time stalls at n = {stall}, t = {float(ts[0])!r}")


def test_table_time_generator_is_the_sequential_one():
    for dtype in ("c32", "f64"):
        a = fixture_generator(dtype, SG.SAW).generate(70_000)
        b = fixture_generator(dtype, SG.SAW, table_time=True).generate(70_000)
        assert np.array_equal(a, b)


def test_draws_and_jump_are_stepping():
    st = SG.seed_state(12345)
    s = list(st)
    seq = np.array([SG.step(s) for _ in range(5000)], dtype=np.uint64)
    assert np.array_equal(SG.draws(st, 5000, lanes=64), seq) and np.array_equal(SG.draws(st, 4999, lanes=7), seq[:4999])
    assert SG.jump(st, 5000) == s and SG.jump(st, 0) == st
    assert np.array_equal(O.xoshiro_draws(12345, 100), seq[:100])
