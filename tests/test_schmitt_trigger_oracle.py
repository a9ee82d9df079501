"""The plain-Python restatement of gr::trigger::SchmittTrigger (tests/schmitt_trigger_oracle.py) pinned on the reference's own QA: the signals and expected
(kind, index) lists of algorithm/test/qa_SchmittTrigger.cpp:74-160 and of its integer suite (:203-230), fed in the QA's order -- the one case without reset()
between two signals included (:107-109) -- with the QA's tolerance of 0.1 on sample + edge_idx + edge_offset (:43, :59).  The LINEAR cases run on the block's
window of 32 (Trigger.hpp:45); none of the QA's signals accumulates more than 12 samples, so the expectations of its window of 12 hold."""
import numpy as np
import pytest

import schmitt_trigger_oracle as ST

R, F = ST.RISING, ST.FALLING
NO, BASIC, LINEAR = ST.NO_INTERPOLATION, ST.BASIC_LINEAR_INTERPOLATION, ST.LINEAR_INTERPOLATION

SLOW_RISING = [0.3, 0.4, 0.45, 0.5, 0.55, 0.6, 1.0, 1.0, 0.0]
SLOW_FALLING = [1.0, 0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6, 0.55, 0.5, 0.45, 0.4, 0.35, 0.3]
FAST = [0.0, 0.8, 1.2, 0.9, 0.4, -0.2, -1.1, -0.5, 0.0, 1.1, 1.1, 1.0, 0.0, 0.0]
DIRAC = [0.0, 1.0, 0.0]
INTERPOLATED = [  # (reset in front, signal, expected): :100-116, the same lists at :122-139
    (True, SLOW_RISING, [(R, 3), (F, 7.5)]),
    (True, SLOW_FALLING, [(R, -0.5), (F, 9.0)]),
    (False, FAST, [(R, 0.625), (F, 3.8), (R, 8.45455), (F, 11.5)]),  # (:107-109: BASIC has no reset() here)
    (True, DIRAC, [(R, 0.5), (F, 1.5)]),
]
# threshold 0.1, offset 0.5 (:75, :98, :120)
FLOAT_CASES = {
    NO: [(True, SLOW_RISING, [(R, 5), (F, 8)]), (True, SLOW_FALLING, [(R, 0), (F, 11)]), (True, FAST, [(R, 1), (F, 4), (R, 9), (F, 12)]),
         (True, DIRAC, [(R, 1), (F, 2)])],
    BASIC: INTERPOLATED,
    LINEAR: [(True, s, e) for _, s, e in INTERPOLATED],  # (:126-136: reset() in front of every signal)
}
# threshold 1, offset 5 (:207, :220)
INT_CASES = {
    NO: [(True, [0, 1, 5, 7, 7, 7, 8, 0, 0], [(R, 3), (F, 7)]), (True, [0, 10, 0, 7], [(R, 1), (F, 2), (R, 3)])],
    BASIC: [(True, [0, 1, 5, 7, 7, 7, 8, 0, 0], [(R, 2), (F, 6.375)]), (True, [0, 10, 0, 8], [(R, 0.5), (F, 1.5), (R, 2.625)])],
}


def _run_cases(trigger, cases, dtype):
    for k, (reset, signal, expected) in enumerate(cases):
        if reset and k:
            trigger.reset()
        e = trigger.process(np.array(signal, np.float64).astype(dtype))
        assert e["count"] == len(expected), (k, e)
        assert list(e["kind"]) == [kind for kind, _ in expected], (k, e)
        assert np.all(e["flags"] == 0)
        assert np.allclose(ST.positions(e), [p for _, p in expected], rtol=0, atol=0.1), (k, ST.positions(e), expected)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", [NO, BASIC, LINEAR])
def test_reference_qa_float(method, dtype):
    _run_cases(ST.SchmittTrigger(0.5, 0.1, method, dtype), FLOAT_CASES[method], dtype)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("method", [NO, BASIC])
def test_reference_qa_integer(method, dtype):
    _run_cases(ST.SchmittTrigger(5, 1, method, dtype), INT_CASES[method], dtype)


def _stream(n, seed, dtype=np.float32, scale=1.0):
    rng = np.random.default_rng(seed)
    x = scale * (np.sin(2 * np.pi * np.arange(n) / 37.3) + 0.05 * rng.standard_normal(n))
    return x.astype(dtype)


def _same(a, b):
    return a["count"] == b["count"] and all(np.array_equal(a[k].view(np.int32) if k == "edge_offset" else a[k], b[k].view(np.int32) if k == "edge_offset" else b[k])
                                            for k in ("sample", "kind", "edge_idx", "edge_offset", "n_fit", "flags"))


def _join(parts, starts):
    out = {"count": sum(p["count"] for p in parts)}
    for k in ("sample", "kind", "edge_idx", "edge_offset", "n_fit", "flags"):
        out[k] = np.concatenate([p[k] + s if k == "sample" else p[k] for p, s in zip(parts, starts)])
    return out


@pytest.mark.parametrize("dtype,scale,offset,threshold", [(np.float32, 1.0, 0.1, 0.2), (np.float64, 1.0, 0.1, 0.2), (np.int16, 1000.0, 100, 200)])
@pytest.mark.parametrize("method", [NO, BASIC, LINEAR])
def test_split_calls_give_the_same_edges(method, dtype, scale, offset, threshold):
    x = _stream(3000, 5, dtype, scale)
    whole = ST.SchmittTrigger(offset, threshold, method, dtype).process(x)
    assert whole["count"] > 100
    t = ST.SchmittTrigger(offset, threshold, method, dtype)
    cuts = [0, 1, 18, 19, 50, 1000, 1007, 2999, 3000]  # chunks shorter than the history, an empty one, cuts inside open zones
    parts = [t.process(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert _same(whole, _join(parts, cuts[:-1]))


def test_linear_needs_a_zone_entry_first():
    """the quirk of :177-190: an edge needs a preceding zone entry (yPrev <= lower && yCurr > lower), so a stream that starts inside the band -- here the band
    holds the primed history's zeros -- gives no edge until it has left the band on the far side once.  NO_INTERPOLATION sees every edge."""
    x = np.array([0.0, 0.0, 0.2, 0.4, 0.0, -0.4, 0.0, 0.4, 0.0, -0.4], np.float32)  # band -0.1 ... 0.1
    e0 = ST.SchmittTrigger(0.0, 0.1, NO, np.float32).process(x)
    assert list(e0["sample"]) == [2, 5, 7, 9] and list(e0["kind"]) == [R, F, R, F]
    # [2], [3] reach upper with no zone open: no edge, _lastState stays low, so -0.4 at [5] is no FALLING either; -0.4 -> 0 at [6] enters, 0.4 at [7] is the
    # first RISING; 0.4 -> 0 at [8] enters from above and -0.4 at [9] is the FALLING
    e2 = ST.SchmittTrigger(0.0, 0.1, LINEAR, np.float32).process(x)
    assert list(e2["sample"]) == [7, 9] and list(e2["kind"]) == [R, F] and list(e2["n_fit"]) == [2, 2]


def test_linear_integer_crossing_is_truncated():
    """relativeIndex is value_t (:198): for an integer type the crossing index is truncated and the offset is 0, where float keeps the fraction"""
    sig = [0, 0, 4, 5, 7, 12]  # offset 5, threshold 2: zone entered at [2] (0 <= 3 < 4), upper 7 reached at [4], n = 3 over (4, 5, 7)
    ei = ST.SchmittTrigger(5, 2, LINEAR, np.int16).process(np.array(sig, np.int16))
    ef = ST.SchmittTrigger(5, 2, LINEAR, np.float32).process(np.array(sig, np.float32))
    assert list(ei["sample"]) == [4] and list(ef["sample"]) == [4] and list(ei["n_fit"]) == list(ef["n_fit"]) == [3]
    # slope 1.5, intercept 23/6: the line crosses 5 at 7/9 in fit coordinates, relative 7/9 - 2: float rounds to -1 with offset -2/9; the integer
    # truncates 7/9 to 0: -2
    assert list(ef["edge_idx"]) == [-1] and abs(float(ef["edge_offset"][0]) + 2 / 9) < 1e-6
    assert list(ei["edge_idx"]) == [-2] and float(ei["edge_offset"][0]) == 0.0 and list(ei["flags"]) == [0]


def test_zero_slope_is_degenerate_and_flips_the_state():
    t = ST.SchmittTrigger(0.0, 1.0, LINEAR, np.float32)
    e = t.process(ST.ZERO_SLOPE[:5])
    assert list(e["sample"]) == [4] and list(e["kind"]) == [R] and list(e["flags"]) == [ST.DEGENERATE]
    assert e["edge_idx"][0] == 0 and e["edge_offset"][0] == 0.0 and e["n_fit"][0] == 4
    assert t.last is True and t.acc == 0  # the state flips as in the reference (:209-210)
    e = t.process(ST.ZERO_SLOPE[5:])
    assert list(e["sample"]) == [1] and list(e["kind"]) == [F] and list(e["flags"]) == [0] and list(e["n_fit"]) == [2]


def test_nan_holds_the_state():
    x = np.array([0.0, np.nan, 2.0, np.nan, np.nan, -2.0, np.nan], np.float32)
    for method in (NO, BASIC):
        e = ST.SchmittTrigger(0.0, 1.0, method, np.float32).process(x)
        assert list(e["sample"]) == [2, 5] and list(e["kind"]) == [R, F]
    e = ST.SchmittTrigger(0.0, 1.0, BASIC, np.float32).process(x)
    assert list(e["flags"]) == [ST.DEGENERATE, ST.DEGENERATE]  # yPrev is NaN: the reference's round(NaN) -> int32 is undefined


def test_integer_range_and_fractions_are_refused():
    for args in ((32000, 1000), (-32000, 1000), (0.5, 1), (0, 1.5), (40000, 0)):
        with pytest.raises(ValueError):
            ST.SchmittTrigger(*args, NO, np.int16)
    ST.SchmittTrigger(32000, 767, NO, np.int16)
    for args in ((0, -1), (float("nan"), 1), (0, float("inf"))):
        with pytest.raises(ValueError):
            ST.SchmittTrigger(*args, NO, np.float32)
