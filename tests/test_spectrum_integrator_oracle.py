"""The spectrum integrator's oracle against itself (tests/spectrum_integrator_oracle.py): the error of the defined order of additions, its identities and where
its leaves lie.  No GPU needed."""
import numpy as np
import pytest

import pfb_oracle as PO
import spectrum_integrator_oracle as SO

ORDER_TOL = 1e-6  # the parity contract's 1e-5 (include/gr4hip.h) with a decade in hand; measured 3e-8 .. 2.7e-7


def power(N, frames, seed):
    """exact |X|^2 of the tests' signal (float64), and the same rounded to float32: what an integrator is given"""
    x = SO.signal(N * frames, seed).astype(np.complex128).reshape(frames, N)
    p = np.abs(np.fft.fft(x, axis=1)) ** 2
    return p, p.astype(np.float32)


@pytest.mark.parametrize("N,A", [(8, 3), (64, 33), (256, 1000), (1024, 67), (8192, 32)])
@pytest.mark.parametrize("mean", [False, True])
def test_the_order_is_far_inside_the_contract(N, A, mean):
    p, m = power(N, 2 * A + 3, N + A)
    e = PO.rel(SO.integrate_ordered(m, A, mean), SO.integrate(p, A, mean))
    print(f"N {N} A {A} mean {mean}: ordered float32/float64 sums against float64 {e:.2e}")
    assert e <= ORDER_TOL


def test_trailing_frames_are_dropped():
    _, m = power(16, 2 * 5 + 3, 1)
    assert SO.integrate_ordered(m, 5).shape == (2, 16) and SO.integrate(m, 5).shape == (2, 16)
    assert SO.integrate_ordered(m[:4], 5).shape == (0, 16)


@pytest.mark.parametrize("mean", [False, True])
def test_one_frame_per_integration_is_the_identity(mean):
    _, m = power(64, 7, 2)
    assert np.array_equal(SO.integrate_ordered(m, 1, mean), m)


def test_leaves_are_aligned_to_the_integration():
    """values whose float32 sum depends on the grouping: 2^24 + 1 + 1 is 2^24 when the ones are added to it one by one, 2^24 + 2 when they meet first"""
    big = 2.0 ** 24
    m = np.zeros((66, 2), np.float32)
    m[33], m[64], m[65] = big, 1.0, 1.0
    # A = 33: integration 1 is frames 33 .. 65, its leaves are [33, 65) and [65, 66): frame 64 is lost in the first leaf (2^24 + 1 -> 2^24), frame 65 is a leaf of
    # its own, and the float64 sum 2^24 + 1 rounds to 2^24.  Leaves aligned to the stream ([32, 64), [64, 96)) would have given 2^24 + (1 + 1).
    y33 = SO.integrate_ordered(m, 33)
    assert float(y33[0, 0]) == 0.0 and float(y33[1, 0]) == big
    # A = 64: integration 0 is frames 0 .. 63 = leaves [0, 32), [32, 64); A = 66: one more leaf [64, 66), where the ones meet
    assert float(SO.integrate_ordered(m, 64)[0, 0]) == big
    assert float(SO.integrate_ordered(m, 66)[0, 0]) == big + 2
    # and the same three values with the large one LAST in its leaf: A = 33 keeps the ones (leaf [33, 65) = 1 + 1 + 2^24 exactly)
    m2 = np.zeros((66, 2), np.float32)
    m2[33], m2[34], m2[64] = 1.0, 1.0, big
    assert float(SO.integrate_ordered(m2, 33)[1, 0]) == big + 2
    assert float(SO.integrate_ordered(m2, 64)[0, 0]) == 2.0  # (frames 33, 34 alone: frame 64 belongs to the next integration)


def test_a_nan_frame_reaches_only_its_own_integration():
    _, m = power(32, 4 * 33, 3)
    clean = SO.integrate_ordered(m, 33)
    bad = m.copy()
    bad[40, 5] = np.nan
    bad[70, 6] = np.inf
    got = SO.integrate_ordered(bad, 33)
    assert np.isnan(got[1, 5]) and np.isinf(got[2, 6])
    keep = np.ones_like(clean, bool)
    keep[1, 5] = keep[2, 6] = False
    assert np.array_equal(got[keep], clean[keep])
