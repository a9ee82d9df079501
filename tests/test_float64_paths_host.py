"""no GPU: the plans of tests/test_gpu_float64_paths.py are what they say they are -- the kernel each call states is the one the dispatch rule picks, the records they
assert cover both FIR kernels with every R and K-loop, both ways of writing the next history, both FFT kernels and the 128 KiB LDS case, no plan but the rotator's
long span goes beyond 2.7e5 samples, the delta frames of the FFT flag tests are well conditioned, and the numpy truths are the oracle's.  The two test hooks are
exported and declared nowhere."""
import os
import re

import pytest

pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ["gr4hip_internal_fir64_last_path", "gr4hip_internal_fft64_last_path"]


def test_float64_plans():
    import test_gpu_float64_paths as T
    T.test_plans_reach_every_path_and_state_the_dispatch_rule()
    T.test_delta_frames_are_well_conditioned()
    sizes = T.plan_sizes()
    assert len(sizes) > 200 and all(n <= T.MAX_SPAN for _, n in sizes), [s for s in sizes if s[1] > T.MAX_SPAN]
    assert T.ROT_LONG > 1 << 24


def test_float64_plans_state_the_records_of_the_issue():
    """R = 4, 4, 2, 2, 1, 1 for D = 1, 8, 9, 16, 17, 32; the K-loops by tap count; the capacity that only grows"""
    import test_gpu_float64_paths as T
    assert [T._R(D) for D in (1, 8, 9, 16, 17, 32)] == [4, 4, 2, 2, 1, 1]
    assert [T._FirModel(K, 1).want(40000, T.MATRIX)[1:3] for K in (17, 64, 65, 128, 129, 256, 257, 320, 321, 1985, 2048)] == \
        [(20, 64)] * 2 + [(36, 128)] * 2 + [(68, 256)] * 2 + [(0, 320)] * 2 + [(0, 384)] + [(0, 2048)] * 2
    m = T._FirModel(100, 1)
    assert m.hcap == 128 and not m.set_taps(20) and m.hcap == 128 and not m.set_taps(100) and m.set_taps(129) and m.hcap == 256
    assert T._FirModel(2048, 8).want(8, T.DIRECT)[4] == 98240 and T._fft_want(8192, 3, T.RADIX2) == (1, 3, 1, 131072)
    assert T._fft_want(16, 513, T.STOCKHAM) == (2, 2, 512, 65536) and T._fft_want(4096, 3, T.STOCKHAM) == (2, 2, 2, 65536)


@pytest.mark.parametrize("shape,n", [((4, 2), 3000), ((1, 8), 2000), ((8, 1), 1000)])
def test_float64_iir_truth_is_the_oracle(shape, n):
    import test_gpu_float64_paths as T
    T.test_iir_truth_is_the_oracle(shape, n)


@pytest.mark.parametrize("inc,phase0,n", [(1e-3, 0.25, 4096), (0.37, 0.0, 1000), (-2.5, 1.5, 2000)])
def test_float64_rotator_truth_is_the_oracle(inc, phase0, n):
    import numpy as np
    import test_gpu_float64_paths as T
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("the truth needs a long double of 64 bits of mantissa")
    T.test_rotator_truth_is_the_oracle(inc, phase0, n)


@pytest.mark.parametrize("N,window", [(8, "None"), (64, "Hann"), (256, "BlackmanHarris")])
def test_float64_fft_truth_is_the_oracle(N, window):
    import test_gpu_float64_paths as T
    T.test_fft_truth_is_the_oracle(N, window)


def test_float64_hooks_are_exported_and_not_declared():
    from gnuradio4_amd import capi
    import ctypes
    raw = ctypes.CDLL(capi.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "gr4hip.h")).read()
    for s in HOOKS:
        assert hasattr(raw, s) and not re.search(rf"\b{s}\b", text) and s not in capi.SIGNATURES
