"""The oracle of the overlapped FFT frames (tests/stft_oracle.py) against itself and against the library's host-only entry (no GPU): the frames by the definition
through oracle_lib.fft_block_truth / dft64, and the k / off rule against a sample-by-sample walk over random cuts.

test_rule_equals_brute_force, test_frames_by_the_definition and test_skipping_stride_drops_samples pin the oracle against itself (they need no library);
test_library_rule_is_the_oracle_rule and test_create_refusals_need_no_device exercise the library, as does every test of tests/test_gpu_stft.py and
tests/test_stft_host.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import stft_oracle as SO

RULE_SHAPES = [(8, 1), (8, 3), (8, 4), (8, 8), (8, 11), (8, 29), (64, 32), (64, 63), (64, 65), (256, 128), (256, 255), (256, 257)]


def cuts(N, S, seed):
    """call sizes: the edge sizes in random order, mixed with random ones"""
    rng = np.random.default_rng(seed)
    edge = [0, 1, max(S - 1, 0), S, N - 1, N, N + 1, 0, 1]
    rnd = [int(v) for v in rng.integers(0, 3 * max(N, S), 40)]
    sizes = edge + rnd
    rng.shuffle(sizes)
    return [int(v) for v in sizes]


@pytest.mark.parametrize("N,S", RULE_SHAPES)
def test_rule_equals_brute_force(N, S):
    for seed in range(5):
        sizes = cuts(N, S, 100 * N + S + seed)
        rule, off = SO.cut(sizes, N, S)
        brute = SO.starts_brute(sizes, N, S)
        pos, m = 0, 0
        for (k, o), got, n in zip(rule, brute, sizes):
            assert k == len(got), (sizes, pos)
            assert [pos + o + i * S for i in range(k)] == got  # the frames start where the rule says, relative to the call
            assert got == [(m + i) * S for i in range(k)]      # and those are the stream's m S
            pos += n
            m += k
        assert m == SO.n_frames_total(sum(sizes), N, S)  # nothing lost, nothing extra, whatever the cut


def test_frames_by_the_definition():
    N, S = 64, 24
    x = O.signal_c32(7, 5 * S + N + S - 1)
    f = SO.frames(x, N, S)
    assert f.shape == (6, N)  # the tail of S - 1 samples yields no frame
    for m in range(6):
        assert np.array_equal(f[m], x[m * S:m * S + N])
    assert SO.frames(x[:N - 1], N, S).shape == (0, N)
    # the spectrum: the block's float32 window, then oracle_lib.dft64; numpy's float64 transform (the large sizes) agrees with it to float64 rounding
    w = O.window(3, N, np.float32).astype(np.float64)
    t = SO.spectrum(x, N, S)
    for m in range(6):
        assert np.array_equal(t[m], O.dft64(x[m * S:m * S + N].astype(np.complex128) * w))
    assert np.max(np.abs(np.fft.fft(f.astype(np.complex128) * w, axis=1) - t)) <= 1e-12 * np.max(np.abs(t))
    # the block's signals per frame: re / im of fft_block_truth are the spectrum's
    mag, ph, re, im = SO.block_truth(x, N, S)
    assert mag.shape == (6, N) and np.allclose(re + 1j * im, t, rtol=0, atol=1e-9 * np.max(np.abs(t)))
    # real frames: N / 2 values per signal
    xr = O.signal_f32(7, 3 * S + N)
    assert SO.block_truth(xr, N, S)[0].shape == (4, N // 2)


def test_skipping_stride_drops_samples():
    N, S = 8, 11
    x = np.arange(40, dtype=np.float32)
    f = SO.frames(x, N, S)
    assert f.shape == (3, N) and list(f[:, 0]) == [0, 11, 22]  # 33 + 8 > 40: no fourth frame


@pytest.mark.parametrize("N,S", RULE_SHAPES)
def test_library_rule_is_the_oracle_rule(N, S):
    """the library's frame count (csrc/stft.hip stft_rule, what gr4hip_stft_pending and every call use) through its handle-free test hook: host arithmetic, no device"""
    from gnuradio4_amd import capi
    fn = capi.lib().gr4hip_internal_stft_count  # (test hook, not in include/gr4hip.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_size_t, C.c_size_t, C.c_longlong, C.c_size_t, C.POINTER(C.c_size_t)]
    k = C.c_size_t(99)
    for seed in range(3):
        sizes = cuts(N, S, 7 * N + S + seed)
        rule, _ = SO.cut(sizes, N, S)
        brute = SO.starts_brute(sizes, N, S)
        for (want, off), got, n in zip(rule, brute, sizes):
            assert fn(N, S, off, n, C.byref(k)) == 0 and k.value == want == len(got)
    assert fn(N, S, -N, 1, C.byref(k)) == capi.INVALID_ARGUMENT  # off below -(N - 1) cannot happen
    assert fn(N, 0, 0, 1, C.byref(k)) == capi.INVALID_ARGUMENT and fn(N, S, 0, 1, None) == capi.INVALID_ARGUMENT


def test_create_refusals_need_no_device():
    from gnuradio4_amd import capi
    L = capi.lib()
    h = C.c_void_p()
    assert L.gr4hip_stft_create(None, capi.C32, 256, 128, 3, 0) == capi.INVALID_ARGUMENT
    assert L.gr4hip_stft_create(C.byref(h), capi.F64, 256, 128, 3, 0) == capi.INVALID_ARGUMENT
    assert L.gr4hip_stft_create(C.byref(h), capi.C32, 1, 1, 3, 0) == capi.INVALID_ARGUMENT
    assert L.gr4hip_stft_create(C.byref(h), capi.C32, 256, (1 << 20) + 1, 3, 0) == capi.UNSUPPORTED and b"stride" in L.gr4hip_last_error()
    assert L.gr4hip_stft_reset(None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_stft_pending(None, 1, None) == capi.INVALID_ARGUMENT
    n = C.c_size_t(5)
    assert L.gr4hip_stft_spectrum(None, None, 0, None, C.byref(n), None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_stft_destroy(None) == 0
