"""The cross-spectrum correlator's definition (tests/cross_spectrum_oracle.py) against the plain complex128 sum and against itself.  No GPU, no library needed."""
import numpy as np
import pytest

import cross_spectrum_oracle as XO

SHAPES = [(2, 8, 1), (3, 8, 63), (5, 16, 65), (4, 8, 130), (17, 4, 70)]  # (S, N, A)


@pytest.mark.parametrize("S,N,A", SHAPES)
def test_ordered_stays_within_the_chain_bound_of_the_exact_sum(S, N, A):
    """a float32 fma chain of at most 2 B terms per leaf, the leaves in float64, one rounding to float32: per component within (2 B + 2) 2^-24 sum_m |X_i| |X_j|"""
    X = XO.streams(S, 2 * A + 3, N, 100 + S)
    got, want = XO.cross_ordered(X, A), XO.cross_exact(X, A)
    assert got.shape == want.shape == (2 + 3 // A, S * (S + 1) // 2, N)
    bound = (2 * XO.LEAF + 2) * 2.0 ** -24 * XO.abs_bound(X, A)
    worst = max(float(np.max(np.abs(got.real - want.real) / bound)), float(np.max(np.abs(got.imag - want.imag) / bound)))
    print(f"S={S} N={N} A={A}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_the_diagonal_is_real_with_a_positive_zero():
    X = XO.streams(4, 70, 8, 7)
    V = XO.cross_ordered(X, 70)
    for i in range(4):
        d = V[:, XO.baseline(i, i)]
        assert np.all(d.imag.view(np.uint32) == 0) and np.all(d.real > 0)
    assert np.any(V[:, XO.baseline(1, 0)].imag != 0)


def test_one_frame_is_the_conjugate_product_to_float_rounding():
    X = XO.streams(3, 5, 16, 8)
    V = XO.cross_ordered(X, 1)
    assert V.shape == (5, 6, 16)
    for i in range(3):
        for j in range(i + 1):
            want = X[i].astype(np.complex128) * np.conj(X[j].astype(np.complex128))
            scale = np.abs(X[i]).astype(np.float64) * np.abs(X[j]).astype(np.float64)
            got = V[:, XO.baseline(i, j)]
            # two fma per component, then exact conversions: two roundings of at most 2^-24 of |X_i| |X_j| each
            assert np.all(np.abs(got.real - want.real) <= 2.0 ** -23 * scale) and np.all(np.abs(got.imag - want.imag) <= 2.0 ** -23 * scale)


@pytest.mark.parametrize("cut", [1, 63, 64, 65, 129, 140])
def test_an_integration_does_not_depend_on_the_frames_around_it(cut):
    """output q is a function of frames [q A, (q + 1) A) alone: a stream cut at any frame, with the partial integration carried, gives what the uncut one gives --
    the oracle states that as: the matrices of a prefix are a prefix of the matrices, and those of a suffix starting at an integration's first frame are a suffix"""
    A = 70
    X = XO.streams(3, 3 * A, 8, 9)
    whole = XO.cross_ordered(X, A)
    head = XO.cross_ordered(X[:, :cut], A)
    assert np.array_equal(head.view(np.uint32), whole[:cut // A].view(np.uint32))
    tail = XO.cross_ordered(X[:, (cut // A + 1) * A:], A)
    assert np.array_equal(tail.view(np.uint32), whole[cut // A + 1:].view(np.uint32))


def test_mean_is_the_sum_divided_once():
    """mean = (float)(acc / A) from the float64 accumulator -- one rounding, so within half an ulp of sum / A in exact arithmetic, and not always (float)sum / A"""
    A = 130
    X = XO.streams(4, A, 8, 10)
    s, m = XO.cross_ordered(X, A), XO.cross_ordered(X, A, mean=True)
    for part in ("real", "imag"):
        sv, mv = getattr(s, part).astype(np.float64), getattr(m, part).astype(np.float64)
        # sum is (float)acc: |acc - sum| <= 2^-24 |acc|, so |acc / A - sum / A| <= 2^-24 |acc| / A, plus the mean's own rounding
        assert np.all(np.abs(mv - sv / A) <= 2.0 ** -23 * np.abs(sv) / A + 1e-45)
    assert np.all(m.imag[:, [XO.baseline(i, i) for i in range(4)]].view(np.uint32) == 0)
    B = 64  # a power of two: the division is exact, mean == sum / A bit for bit
    s, m = XO.cross_ordered(X[:, :B], B), XO.cross_ordered(X[:, :B], B, mean=True)
    for part in ("real", "imag"):
        assert np.array_equal((getattr(s, part) / np.float32(B)).view(np.uint32), np.ascontiguousarray(getattr(m, part)).view(np.uint32))


def test_coherence_of_a_stream_with_itself_and_of_the_swapped_pair():
    X = XO.streams(3, 40, 8, 11)
    V = XO.cross_ordered(X, 20)
    msc, h1 = XO.coherence(V, 3, 1, 1)
    assert np.all(msc == 1) and np.all(h1 == 1)
    a, ha = XO.coherence(V, 3, 2, 0)
    b, hb = XO.coherence(V, 3, 0, 2)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.all((a > 0) & (a <= 1.0 + 1e-6))
    assert np.all(np.abs(ha * hb - a) <= 1e-6)  # H1_ij H1_ji = V_ij conj(V_ij) / (V_jj V_ii)
