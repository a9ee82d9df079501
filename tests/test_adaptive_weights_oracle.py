"""The adaptive weights' definition (tests/adaptive_weights_oracle.py): the ordered float64 routine against the long-double one under the bound, the
distortionless property, the Capon power against a direct solve, and the failure rule.  No GPU, no library needed."""
import numpy as np
import pytest

import adaptive_weights_oracle as AO
import cross_spectrum_oracle as XO

CASES = [(2, 1, 8, 64, 0.0), (3, 5, 16, 19, 1e-3), (8, 4, 8, 64, 0.0), (17, 3, 8, 40, 1e-2), (32, 32, 4, 64, 0.0), (32, 2, 4, 33, 0.0), (8, 2, 8, 8, 0.0)]  # (S, B, N, A, loading)
_cache = {}


def case(S, B, N, A, loading):
    """(V, a, the ordered result, the exact result, cond2): computed once, shared and left unchanged"""
    key = (S, B, N, A, loading)
    if key not in _cache:
        V = XO.cross_ordered(XO.streams(S, A, N, 7 * S + B), A, mean=True)
        a = AO.steering(B, S, N, 100 * S + B)
        _cache[key] = (V, a, AO.mvdr_ordered(V, a, loading), AO.mvdr_exact(V, a, loading), AO.kappa(V, S, loading))
    return _cache[key]


@pytest.mark.parametrize("S,B,N,A,loading", CASES)
def test_ordered_stays_within_the_bound_of_the_long_double_result(S, B, N, A, loading):
    V, a, (W, P, failed), (Wx, Px, fx), kap = case(S, B, N, A, loading)
    assert W.shape == (1, B, S, N) and W.dtype == np.complex64 and P.shape == (1, B, N) and P.dtype == np.float32
    assert not failed.any() and not fx.any()
    rw, rp = AO.ratios(W, P, Wx, Px, kap, S)
    print(f"S={S} B={B} N={N} A={A} loading={loading}: cond2 <= {kap.max():.3g}, worst error / bound: W {rw:.3f}, P {rp:.3f}")
    assert rw <= 1.0 and rp <= 1.0


@pytest.mark.parametrize("S,B,N,A,loading", CASES)
def test_the_weights_are_distortionless(S, B, N, A, loading):
    V, a, (W, P, _), _, _ = case(S, B, N, A, loading)
    resp = (W[0].astype(np.complex128) * a.astype(np.complex128)).sum(axis=1)  # sum_s W_s a_s, [B, N]
    dev = float(np.max(np.abs(resp - 1)))
    print(f"S={S} B={B}: |sum_s W_s a_s - 1| <= {dev:.3g}")
    assert dev <= 1e-6


@pytest.mark.parametrize("S,B,N,A,loading", CASES)
def test_the_power_is_the_capon_estimate_of_a_direct_solve(S, B, N, A, loading):
    V, a, (W, P, _), _, kap = case(S, B, N, A, loading)
    R = AO.loaded_matrix(V, S, loading)[:, :, 0]  # [S, S, N]
    for c in range(N):
        for b in range(B):
            ab = a[b, :, c].astype(np.complex128)
            want = 1.0 / np.real(np.conj(ab) @ np.linalg.solve(R[:, :, c], ab))
            assert abs(float(P[0, b, c]) - want) <= (2.0 ** -23 + 4 * (8 + S) * kap[0, c] * 2.0 ** -53) * want  # both sides carry the solve's error


@pytest.mark.parametrize("solve", [AO.mvdr_ordered, AO.mvdr_exact])
def test_a_failed_pivot_gives_nan_in_exactly_its_bin(solve):
    S, B, N = 4, 3, 6
    V, bad = AO.hand_made(S, N)
    a = AO.steering(B, S, N, 9)
    W, P, failed = solve(V, a, 0.0)
    want = np.zeros((4, N), bool)
    for q, c in bad:
        want[q, c] = True
    assert np.array_equal(failed, want)
    assert np.array_equal(np.isnan(W.real) & np.isnan(W.imag), np.broadcast_to(want[:, None, None, :], W.shape))
    assert np.array_equal(np.isnan(P), np.broadcast_to(want[:, None, :], P.shape))
    assert np.all(np.isfinite(W[~np.broadcast_to(want[:, None, None, :], W.shape)]))
    clean = XO.cross_ordered(XO.streams(S, 4 * 16, N, 5), 16, mean=True)
    W0, P0, f0 = solve(clean, a, 0.0)
    keep = ~np.broadcast_to(want[:, None, None, :], W.shape)
    assert not f0.any() and np.array_equal(W[keep], W0[keep])  # neighbouring bins and matrices are untouched


def test_a_nan_in_a_steering_vector_reaches_only_its_beam_and_bin():
    S, B, N = 4, 3, 6
    V = XO.cross_ordered(XO.streams(S, 16, N, 5), 16, mean=True)
    a = np.array(AO.steering(B, S, N, 9))
    W0, P0, _ = AO.mvdr_ordered(V, a)
    a[1, 2, 3] = np.nan
    W, P, failed = AO.mvdr_ordered(V, a)
    hit = np.zeros(W.shape, bool)
    hit[:, 1, :, 3] = True
    assert not failed.any() and np.all(np.isnan(W[hit])) and np.all(np.isnan(P[:, 1, 3]))
    assert np.array_equal(W[~hit].view(np.uint32), W0[~hit].view(np.uint32))
