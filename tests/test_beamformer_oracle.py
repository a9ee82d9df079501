"""The beamformer's definition (tests/beamformer_oracle.py) against the plain complex128 sum and against the spectrum integrator's oracle.  No GPU, no library
needed."""
import numpy as np
import pytest

import beamformer_oracle as BO
import cross_spectrum_oracle as XO
import spectrum_integrator_oracle as SI
from pfb_oracle import _fma32

SHAPES = [(1, 1, 8, 5), (2, 1, 8, 5), (3, 5, 16, 19), (8, 4, 8, 17), (9, 17, 8, 17), (32, 32, 4, 18)]  # (S, B, N, F)


def case(S, B, N, F):
    return BO.weights(B, S, N, 7 * S + B + 1), XO.streams(S, F, N, 7 * S + B)


@pytest.mark.parametrize("S,B,N,F", SHAPES)
def test_ordered_stays_within_the_chain_bound_of_the_exact_sum(S, B, N, F):
    """each component is a float32 fma chain of 2 S terms: within (2 S + 1) 2^-24 sum_s |W| |X| of the exact sum"""
    W, X = case(S, B, N, F)
    got, want = BO.beams_ordered(W, X), BO.beams_exact(W, X)
    assert got.shape == want.shape == (B, F, N)
    bound = (2 * S + 1) * 2.0 ** -24 * BO.abs_bound(W, X)
    worst = max(float(np.max(np.abs(got.real - want.real) / bound)), float(np.max(np.abs(got.imag - want.imag) / bound)))
    print(f"S={S} B={B} N={N} F={F}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_no_accumulator_of_these_inputs_is_a_negative_zero():
    W, X = case(3, 5, 16, 19)
    Y = BO.beams_ordered(W, X)
    assert not np.any((Y.real == 0) & np.signbit(Y.real)) and not np.any((Y.imag == 0) & np.signbit(Y.imag))


def test_the_short_weight_form_is_the_same_weight_in_every_bin():
    W, X = case(3, 5, 16, 7)
    short = np.ascontiguousarray(W[:, :, 0])
    a = BO.beams_ordered(short, X)
    b = BO.beams_ordered(np.repeat(short[:, :, None], 16, axis=2), X)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("A,mean", [(1, False), (5, False), (32, True), (33, False), (70, True)])
def test_integrated_power_is_the_integrator_applied_to_the_detected_power(A, mean):
    S, B, N, F = 3, 5, 16, 2 * 70 + 3
    W, X = case(S, B, N, F)
    Y = BO.beams_ordered(W, X)
    yr, yi = np.ascontiguousarray(Y.real), np.ascontiguousarray(Y.imag)
    p = _fma32(yr, yr, yi * yi)  # [B, F, N]
    frames = np.ascontiguousarray(p.transpose(1, 0, 2)).reshape(F, B * N)
    want = SI.integrate_ordered(frames, A, mean).reshape(F // A, B, N)
    got = BO.power_integrated_ordered(W, X, A, mean)
    assert got.shape == want.shape == (F // A, B, N) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if A == 1:  # A = 1 is the per-frame power itself
        assert np.array_equal(got.view(np.uint32), frames.reshape(F, B, N).view(np.uint32))


def test_a_nan_reaches_every_beam_in_its_own_frame_and_bin_only():
    S, B, N, F = 4, 3, 8, 6
    W, X = case(S, B, N, F)
    W = np.array(W)
    W[1, 2] = 0  # beam 1 ignores stream 2 -- but 0 NaN = NaN
    X = np.array(X)
    clean = BO.beams_ordered(W, X)
    X[2, 4, 5] = np.nan
    Y = BO.beams_ordered(W, X)
    hit = np.zeros(Y.shape, bool)
    hit[:, 4, 5] = True
    assert np.all(np.isnan(Y.real[hit])) and np.all(np.isnan(Y.imag[hit]))
    assert np.array_equal(Y[~hit].view(np.uint32), clean[~hit].view(np.uint32))
