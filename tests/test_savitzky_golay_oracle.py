"""The Savitzky-Golay oracle (tests/savitzky_golay_oracle.py) against the reference's own test facts (algorithm/test/qa_SavitzkyGolay.cpp) and against exact rational
least squares.  No GPU and no library: numpy and fractions only."""
import numpy as np
import pytest

import savitzky_golay_oracle as SG

# every (W, p, d, alignment) the other Savitzky-Golay tests design with; the float64 rule drops nothing in any of them (asserted below)
SETTINGS = [(1, 0, 0), (2, 1, 0), (4, 2, 1), (5, 2, 0), (5, 4, 4), (7, 3, 0), (11, 4, 0), (11, 4, 1), (11, 4, 2), (21, 3, 0), (21, 10, 0), (25, 4, 2), (31, 6, 0),
            (32, 3, 1), (33, 3, 0), (51, 4, 0), (64, 3, 0), (64, 3, 1), (101, 4, 0), (101, 6, 1), (128, 3, 1), (255, 4, 0)]


@pytest.mark.parametrize("W", [5, 7, 11, 21])
def test_smoothing_coefficients_are_symmetric_and_sum_to_one(W):
    """qa_SavitzkyGolay.cpp:18-32"""
    for dtype, tol in ((np.float32, 1e-5), (np.float64, 1e-12)):
        c, info = SG.design(dtype, W, 3)
        assert c.dtype == dtype and len(c) == W and info["rank"] == 4
        assert abs(float(c.astype(np.float64).sum()) - 1.0) < tol
        assert np.max(np.abs(c - c[::-1])) < tol


def test_derivative_coefficients_sum_to_zero_and_order_zero_is_the_mean():
    for dtype, tol in ((np.float32, 1e-5), (np.float64, 1e-12)):
        for W in (5, 11, 21):
            for alignment in ("Centred", "Causal"):
                c, _ = SG.design(dtype, W, 3, 1, 1.0, alignment)
                assert abs(float(c.astype(np.float64).sum())) < tol * 10
                c0, _ = SG.design(dtype, W, 0, 0, 1.0, alignment)
                assert np.max(np.abs(c0.astype(np.float64) - 1.0 / W)) < tol


def test_clamps():
    """SavitzkyGolay.hpp:95-98"""
    assert SG.clamp(0, 4, 0) == (1, 0, 0)
    assert SG.clamp(5, 10, 10) == (5, 4, 4)
    assert SG.clamp(11, 4, 7) == (11, 4, 4)
    c, info = SG.design(np.float32, 5, 10, 10)
    c2, _ = SG.design(np.float32, 5, 4, 4)
    assert np.array_equal(c, c2) and (info["W"], info["p"], info["d"]) == (5, 4, 4)
    c, _ = SG.design(np.float64, 0, 3, 2)
    assert np.array_equal(c, [1.0])
    # delta <= 0 is clamped to eps_T, not refused: the scale is d! / eps^d
    for dtype in (np.float32, np.float64):
        eps = np.finfo(dtype).eps
        assert SG.scale(dtype, 1, 0.0) == dtype(1) / eps and SG.scale(dtype, 1, -5.0) == dtype(1) / eps
        assert SG.scale(dtype, 0, -5.0) == 1 and SG.scale(dtype, 3, 1.0) == 6
        a, _ = SG.design(dtype, 7, 2, 1, 0.0)
        b, _ = SG.design(dtype, 7, 2, 1, float(eps))
        assert np.array_equal(a, b)
    assert SG.centre(11) == 5 and SG.centre(10) == 4 and SG.centre(11, "Causal") == 10 and SG.centre(11, "Sideways") == 5


def test_index_tables_hold_literally():
    """qa_SavitzkyGolay.cpp:67-84: reflectIndex / replicateIndex on N = 5"""
    assert [SG.reflect_index(i, 5) for i in range(-5, 0)] == [4, 3, 2, 1, 0]
    assert [SG.reflect_index(i, 5) for i in range(0, 5)] == [0, 1, 2, 3, 4]
    assert [SG.reflect_index(i, 5) for i in range(5, 10)] == [4, 3, 2, 1, 0]
    assert SG.reflect_index(-1, 5) == 0 and SG.reflect_index(-2, 5) == 1 and SG.reflect_index(5, 5) == 4 and SG.reflect_index(6, 5) == 3
    assert SG.reflect_index(10, 5) == 0 and SG.reflect_index(-11, 5) == 0 and SG.reflect_index(23, 2) == 0  # several wraps
    assert [SG.replicate_index(i, 5) for i in (-100, -1, 0, 2, 4, 5, 100)] == [0, 0, 0, 2, 4, 4, 4]
    assert SG.reflect_index(3, 0) == 0 and SG.replicate_index(3, 0) == 0
    for N in (1, 2, 3, 7):
        for policy, fn in (("Reflect", SG.reflect_index), ("Replicate", SG.replicate_index)):
            assert list(SG._index_table(-20, 25, N, policy)) == [fn(i, N) for i in range(-20, 25)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_cubic_passes_a_cubic_filter_unchanged(dtype):
    n = np.arange(200, dtype=np.float64)
    x = (1e-5 * (n - 90) ** 3 - 2e-3 * n ** 2 + 0.5 * n - 3).astype(dtype)
    tol = 64 * float(np.finfo(dtype).eps) * float(np.max(np.abs(x)))
    for W, p in ((7, 3), (11, 4), (21, 3)):
        c, info = SG.design(dtype, W, p)
        assert info["rank"] == p + 1
        y, _ = SG.streaming(c, x)
        D = (W - 1) // 2
        assert np.max(np.abs(y[W - 1:].astype(np.float64) - x[W - 1 - D:len(x) - D].astype(np.float64))) <= tol  # the centred filter delays by D
        for policy in ("Reflect", "Replicate"):
            z, _ = SG.zero_phase(c, x, policy)
            assert np.max(np.abs(z[W:-W].astype(np.float64) - x[W:-W].astype(np.float64))) <= tol


@pytest.mark.parametrize("W", [1, 2, 4, 5, 8, 11])
def test_two_pass_form_is_the_literal_reverse_apply_reverse(W):
    """the semantics the device kernel implements against SavitzkyGolay.hpp:177-193 word for word; N < W wraps reflectIndex several times"""
    rng = np.random.default_rng(W)
    c = rng.standard_normal(W)
    for N in (1, 2, 3, W, W + 1, 3 * W + 2):
        x = rng.standard_normal(N) + 0.3 * np.arange(N)
        for policy in ("Reflect", "Replicate"):
            got, _ = SG.zero_phase(c, x, policy)
            assert np.max(np.abs(got - SG.zero_phase_literal(c, x, policy))) <= 8 * np.finfo(np.float64).eps * np.abs(c).sum() ** 2 * np.abs(x).max()
    assert len(SG.zero_phase(c, np.zeros(0), "Reflect")[0]) == 0


def test_float64_svd_agrees_with_exact_rational_least_squares(capsys):
    """where the rule drops nothing the design is plain least squares, which fractions.Fraction solves exactly: the worst deviation of numpy's float64 SVD from it,
    relative to the largest coefficient, is what tests/test_savitzky_golay_host.py sizes the library's bar by (printed with pytest -s)"""
    worst = 0.0
    for W, p, d in SETTINGS:
        for alignment in ("Centred", "Causal"):
            row, info = SG.pinv_row(np.float64, W, p, d, alignment)
            assert info["rank"] == info["p"] + 1, (W, p, d, alignment)
            exact = np.array([float(v) for v in SG.exact_row(W, p, d, alignment)])
            dev = float(np.max(np.abs(row - exact)) / np.max(np.abs(exact)))
            cond = info["sigma_max"] / info["sigma_min_kept"]
            print(f"W {W:3d} p {p:2d} d {d:2d} {alignment:8s} cond {cond:9.3g}  numpy-vs-exact {dev:.3g}")
            assert dev <= 64 * np.finfo(np.float64).eps * cond, (W, p, d, alignment)  # a backward-stable SVD: eps * cond, with room
            worst = max(worst, dev / cond)
    print(f"worst deviation / cond: {worst:.3g}")


def test_the_float_rule_truncates_at_ordinary_settings():
    """the fact the whole contract hangs on: with float's epsilon the rule drops singular values at W = 51, p = 4 and at W = 31, p = 6, and the truncated
    coefficients differ from least squares by far more than rounding"""
    for W, p, kept in ((51, 4, 4), (31, 6, 4), (101, 4, 3), (21, 10, 5), (11, 4, 5)):
        row, info = SG.pinv_row(np.float32, W, p, 0)
        assert info["rank"] == kept, (W, p, info["rank"])
    row, info = SG.pinv_row(np.float32, 51, 4, 0)
    exact = np.array([float(v) for v in SG.exact_row(51, 4, 0)])
    assert np.max(np.abs(row - exact)) / np.max(np.abs(exact)) > 1e-3
    assert SG.pinv_row(np.float32, 31, 6, 0)[1]["ambiguous"] and not SG.pinv_row(np.float32, 11, 4, 0)[1]["ambiguous"]
