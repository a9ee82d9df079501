"""GPU parity tests (run with -m gpu on an MI355X): the HIP path through the C-ABI (ctypes -> libgr4hip.so) against the
CPU oracle on identical seeded inputs.  Bar (the parity contract of include/gr4hip.h, "Conventions"; `_rel` below IS that formula): bit-exact for
integer / byte / copy work; for float32 FIR / IIR / FFT  max_k |gpu_k - truth_k| / max(|truth_k|, rms(truth)) <= 1e-5  against the float64 oracle
(BASELINE.json north_star: "<= 1e-5 rel"; relative above the rms level of the output, rms-normalised below it: point-wise relative error is
meaningless near spectral zeros)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5


def _rel(got, truth):
    """THE parity metric (include/gr4hip.h, "PARITY CONTRACT"): max_k |got_k - truth_k| / max(|truth_k|, rms(truth)) -- relative error for values above the
    rms level, rms-normalised absolute error below it (an all-rms normalisation would demand better than float32 epsilon on a dominant tone bin of
    a quadratic output: peak/rms ~ sqrt(N))."""
    got = np.asarray(got).astype(np.complex128 if np.iscomplexobj(got) else np.float64).ravel()
    truth = np.asarray(truth).ravel()
    rms = np.sqrt(np.mean(np.abs(truth) ** 2))
    return float(np.max(np.abs(got - truth) / np.maximum(np.abs(truth), rms if rms > 0 else 1.0)))


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ref32_err(b, x, truth, sl, decim=1):
    """the parity contract's second clause (include/gr4hip.h): the error of the REFERENCE's own float32 arithmetic on the same input -- the oracle's restatement of
    time_domain_filter.hpp:44-47 / 190-204 evaluated in float32, in order (oracle/gr4_oracle.c gr4o_fir_f32 / gr4o_fir_c32) -- against the float64 evaluation,
    with the contract's formula.  The bound for a device result where float32 cannot meet 1e-5 is this number, factor ONE."""
    r32 = O.fir(b, x, acc64=False)[0][::decim]
    return _rel(r32[sl], truth[sl])


@pytest.fixture
def devsw(G):
    """developer switches of the library (gr4hip_developer_switch: which of two kernels serves a call), restored when the test ends"""
    used = set()

    def set_(name, value=1):
        used.add(name)
        G.capi.developer_switch(name, value)
    yield set_
    for name in used:
        G.capi.developer_switch(name, 0)


# ------------------------------------------------------------------ plumbing
def test_host_ring_is_double_mapped_and_page_locked(G):
    """gr4hip_host_ring_create: `bytes` of page-locked host storage mapped twice back to back (the reference's double-mapped CircularBuffer, CircularBuffer.hpp:75-172, on the
    host side of the link): base[i] and base[i + bytes] are the same byte, a span across the physical end is one contiguous source for the copy engine"""
    import ctypes as C
    L = G.capi.lib()
    nbytes = 1 << 20
    base = C.c_void_p()
    G.capi.check(L.gr4hip_host_ring_create(C.byref(base), nbytes), "host_ring_create")
    try:
        a = np.ctypeslib.as_array((C.c_uint32 * (2 * nbytes // 4)).from_address(base.value))
        a[: nbytes // 4] = (np.arange(nbytes // 4, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
        assert np.array_equal(a[: nbytes // 4], a[nbytes // 4:])          # the second mapping IS the first
        a[nbytes // 4 + 7] = 42
        assert a[7] == 42
        d = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
        start = nbytes // 4 - 1000                                         # a span that wraps the physical end, read in place by the copy engine
        G.capi.check(L.gr4hip_memcpy_h2d(d.data_ptr(), base.value + 4 * start, nbytes, None), "h2d")
        G.capi.check(L.gr4hip_stream_synchronize(None), "sync")
        assert np.array_equal(d.cpu().numpy().view(np.uint32), a[start:start + nbytes // 4])
        with pytest.raises(G.capi.Gr4HipError):
            G.capi.check(L.gr4hip_host_ring_create(C.byref(C.c_void_p()), 1000), "not a whole number of pages")
    finally:
        G.capi.check(L.gr4hip_host_ring_destroy(base, nbytes), "host_ring_destroy")


def test_caller_supplied_output_tensors_are_checked(G):
    """an undersized, host-side, strided or wrongly typed `out` handed to a kernel is an out-of-bounds device write -- every entry point of the host layer
    that takes one refuses it (INVALID_ARGUMENT) before anything is launched"""
    x = G.synth_f32(4096, seed=1)
    b = O.design_taps_hamming_lowpass(31, 0.1)
    f = G.fir_filter(b, torch.float32, decimate=4)
    good = torch.empty(1024, dtype=torch.float32, device="cuda")
    assert f.process_bulk(x, good) is good
    for bad in (torch.empty(1023, dtype=torch.float32, device="cuda"), torch.empty(1024, dtype=torch.float32), torch.empty(1024, dtype=torch.float64, device="cuda"),
                torch.empty(2048, dtype=torch.float32, device="cuda")[::2]):
        with pytest.raises(G.capi.Gr4HipError):
            f.process_bulk(x, bad)
        with pytest.raises(G.capi.Gr4HipError):
            G.Merged(torch.float32, [("Add", 1.0)]).decimate(x, 4, bad)
    with pytest.raises(G.capi.Gr4HipError):
        G.Merged(torch.float32, [("Add", 1.0)]).process_bulk(x, torch.empty(4095, dtype=torch.float32, device="cuda"))
    with pytest.raises(G.capi.Gr4HipError):
        G.FFT(256, "None").mag2(G.synth_c32(1024), torch.empty(1023, dtype=torch.float32, device="cuda"))
    fb, xb = G.FirBatched(np.ones((2, 8), np.float32)), torch.zeros((2, 1000), dtype=torch.float32, device="cuda")
    good = torch.empty((2, 1008), dtype=torch.float32, device="cuda")
    assert fb.process_bulk(xb, good).data_ptr() == good.data_ptr()
    assert fb.process_bulk(xb, torch.empty((2, 2016), dtype=torch.float32, device="cuda")[:, :1000]).shape == (2, 1000)  # a row-strided view with unit inner stride is legal
    for bad in (torch.empty((2, 999), dtype=torch.float32, device="cuda"), torch.empty((3, 1000), dtype=torch.float32, device="cuda"), torch.empty(2000, dtype=torch.float32, device="cuda"),
                torch.empty((2, 1000), dtype=torch.float32), torch.empty((2, 1000), dtype=torch.float64, device="cuda"), torch.empty((2, 2000), dtype=torch.float32, device="cuda")[:, ::2],
                torch.empty((1000, 2), dtype=torch.float32, device="cuda").t()):
        with pytest.raises(G.capi.Gr4HipError) as e:
            fb.process_bulk(xb, bad)
        assert e.value.status == G.capi.INVALID_ARGUMENT


def test_native_library_is_loaded_and_shares_torch_runtime(G):
    L = G.capi.lib()
    n = C.c_int(0)
    assert L.gr4hip_device_count(C.byref(n)) == 0 and n.value >= 1
    buf = C.create_string_buffer(256)
    assert L.gr4hip_device_name(0, buf, 256) == 0
    assert b"gfx950" in buf.value, buf.value
    # a torch-allocated tensor is a valid device pointer for the library (same HIP runtime instance)
    x = torch.arange(1024, dtype=torch.int32, device="cuda")
    y = G.math_const("Add", x, 5)
    assert torch.equal(y, x + 5)
    maps = open("/proc/self/maps").read()
    assert "libgr4hip.so" in maps


def test_ring_is_double_mapped(G):
    L = G.capi.lib()
    ring = C.c_void_p()
    assert L.gr4hip_ring_create(C.byref(ring), 1 << 20) == 0, L.gr4hip_last_error()
    base, size = C.c_void_p(), C.c_size_t()
    L.gr4hip_ring_base(ring, C.byref(base))
    L.gr4hip_ring_size(ring, C.byref(size))
    n = size.value // 4
    host = np.arange(n, dtype=np.int32)
    assert L.gr4hip_memcpy_h2d(base, host.ctypes.data, size.value, None) == 0
    back = np.empty(n, np.int32)
    assert L.gr4hip_memcpy_d2h(back.ctypes.data, C.c_void_p(base.value + size.value), size.value, None) == 0  # second mapping
    L.gr4hip_stream_synchronize(None)
    assert np.array_equal(back, host)
    # a span that straddles the wrap point is contiguous: run a kernel across it
    span = np.empty(1024, np.int32)
    start = base.value + size.value - 512 * 4
    one = np.array([1], np.int32)
    out = torch.empty(1024, dtype=torch.int32, device="cuda")
    assert L.gr4hip_math_const(0, 6, C.c_void_p(start), out.data_ptr(), 1024, one.ctypes.data, None) == 0
    L.gr4hip_memcpy_d2h(span.ctypes.data, out.data_ptr(), 4096, None)
    L.gr4hip_stream_synchronize(None)
    assert np.array_equal(span, np.concatenate([host[-512:], host[:512]]) + 1)
    assert L.gr4hip_ring_destroy(ring) == 0


# ------------------------------------------------------------------ FIR (a1, a2, a5, a6)
@pytest.mark.parametrize("ntaps", [1, 2, 10, 64, 91, 256, 1024])
@pytest.mark.parametrize("cplx", [False, True])
def test_fir_parity(G, ntaps, cplx):
    rng = np.random.default_rng(ntaps)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    n = 50_000 + 37
    x = O.signal_c32(42, n) if cplx else O.signal_f32(42, n)
    truth, _ = O.fir(b, x)
    f = G.fir_filter(b, torch.complex64 if cplx else torch.float32)
    y = f.process_bulk(dev(x)).cpu().numpy()
    assert _rel(y, truth) <= TOL
    # not worse than the reference-faithful float CPU path by more than 1e-6 of rms
    cpu32, _ = O.fir(b, x, acc64=False)
    assert _rel(y, truth) <= _rel(cpu32, truth) + 1e-6


@pytest.mark.parametrize("cplx", [False, True])
def test_fir_history_across_calls(G, cplx):
    rng = np.random.default_rng(3)
    b = rng.standard_normal(64).astype(np.float32)
    x = O.signal_c32(7, 30_000) if cplx else O.signal_f32(7, 30_000)
    truth, _ = O.fir(b, x)
    f = G.fir_filter(b, torch.complex64 if cplx else torch.float32)
    cuts = [0, 1, 2, 33, 63, 64, 65, 4096, 4097, 20_000, 30_000]  # spans shorter and longer than the history
    parts = [f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert _rel(np.concatenate(parts), truth) <= TOL
    f.reset()
    again = f.process_bulk(dev(x[:1000])).cpu().numpy()
    assert _rel(again, truth[:1000]) <= TOL
    assert f.process_bulk(dev(x[:0])).numel() == 0  # empty span


@pytest.mark.parametrize("ntaps", [33, 64, 100, 128, 200, 256])
def test_fir_real_long_input_mfma(G, ntaps):
    """float, 33..256 taps, >= 2^16 samples: the block-Toeplitz MFMA kernel; history crosses the VALU / MFMA boundaries"""
    rng = np.random.default_rng(ntaps)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    cuts = [0, 1000, 1000 + 70_001, 1000 + 70_001 + 17, 1000 + 70_001 + 17 + 65_536]
    x = O.signal_f32(11, cuts[-1])
    truth, _ = O.fir(b, x)
    f = G.fir_filter(b, torch.float32)
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _rel(y, truth) <= TOL
    cpu32, _ = O.fir(b, x, acc64=False)
    assert _rel(y, truth) <= _rel(cpu32, truth) + 1e-6


@pytest.mark.parametrize("scale", [1e-25, 1e25])
def test_fir_float_bf16_three_term_kernel_keeps_its_accuracy_across_the_exponent_range(G, scale):
    """the three bf16 terms share float32's exponent range: a stream 25 decades above or below unity loses nothing (no scaling step, no fp16-style range limit)"""
    ntaps, n = 200, 120_000
    b = O.design_taps_hamming_lowpass(ntaps, 0.1)
    x = (O.signal_f32(97, n) * np.float32(scale)).astype(np.float32)
    truth, _ = O.fir(b, x)
    xin = torch.empty(n + 4, dtype=torch.float32, device="cuda")[4:]
    xin.copy_(torch.from_numpy(x))
    y = G.fir_filter(b, torch.float32).process_bulk(xin).cpu().numpy()
    assert np.all(np.isfinite(y)) and _rel(y, truth) <= TOL


@pytest.mark.parametrize("ntaps", [257, 384, 512, 1000, 1024, 2048])
def test_fir_float_more_than_256_taps_in_slices(G, ntaps):
    """fir_filter<float>, 384 .. 1024 taps, long aligned spans (257 and 2048 taps: the register-window kernel, same contract): slices of 256 taps, each a pass of the three-term bf16 kernel over the input delayed by 256 p
    samples that adds to the output; history deeper than one slice, ragged calls alternating with the register-window kernel"""
    rng = np.random.default_rng(ntaps)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    n = 200_000
    x = O.signal_f32(95, n)
    truth, _ = O.fir(b, x)
    f = G.fir_filter(b, torch.float32)
    cuts = [0, 60_000, 60_004, 63_000, 150_000, n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        xin = torch.empty(hi - lo + 4, dtype=torch.float32, device="cuda")[4:]  # 16-byte aligned start
        xin.copy_(torch.from_numpy(x[lo:hi]))
        parts.append(f.process_bulk(xin).cpu().numpy())
    assert _rel(np.concatenate(parts), truth) <= TOL


@pytest.mark.parametrize("ntaps", [65, 81, 113, 146, 200, 256])
def test_fir_float_bf16_three_term_kernel(G, ntaps, devsw):
    """fir_filter<float>, 65 .. 256 taps, long aligned spans: samples and taps as three bf16 terms each on the bf16 matrix pipe (fir_bf16.hip) -- float32
    accuracy: against the float64 oracle at the same bar as the f32 MFMA kernel, also when the filter removes a tone 30 dB above what passes (the error is
    relative to the products, like float32's own rounding, so the bar is checked relative to the OUTPUT), across ragged calls, and against the f32 kernel"""
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    n = 300_000
    x = (O.signal_f32(91, n, tone_frel=0.31, tone_amp=30.0)).astype(np.float32)
    truth, _ = O.fir(b, x)
    f = G.fir_filter(b, torch.float32)
    f.set_algo(G.capi.FIR_TIME_DOMAIN_BF16X3)  # (the default takes the two-term f16 kernel since round 4: test_fir_float_f16_two_term_kernel)
    cuts = [0, 120_000, 120_004, 121_000, n]

    def run(flt):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            xin = torch.empty(hi - lo + 4, dtype=torch.float32, device="cuda")[4:]  # 16-byte aligned start
            xin.copy_(torch.from_numpy(x[lo:hi]))
            parts.append(flt.process_bulk(xin).cpu().numpy())
        return np.concatenate(parts)
    y = run(f)
    assert _rel(y, truth) <= TOL
    devsw("GR4HIP_FIR_NO_BF16X3", 1)
    y32 = run(G.fir_filter(b, torch.float32))
    devsw("GR4HIP_FIR_NO_BF16X3", 0)
    assert _rel(y32, truth) <= TOL
    assert _rel(y, truth) <= 3 * _rel(y32, truth) + 1e-7  # as accurate as the float32 kernel, to a small factor
    # white noise through a random filter: no structure for the dropped 2^-24 terms to hide behind
    rng = np.random.default_rng(ntaps)
    br = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    xr = O.signal_f32(92, 100_000, tone_amp=0.0)
    tr, _ = O.fir(br, xr)
    xin = torch.empty(100_004, dtype=torch.float32, device="cuda")[4:]
    xin.copy_(torch.from_numpy(xr))
    fbf = G.fir_filter(br, torch.float32)
    fbf.set_algo(G.capi.FIR_TIME_DOMAIN_BF16X3)
    e_bf = _rel(fbf.process_bulk(xin).cpu().numpy(), tr)
    devsw("GR4HIP_FIR_NO_BF16X3", 1)
    e_32 = _rel(G.fir_filter(br, torch.float32).process_bulk(xin).cpu().numpy(), tr)
    devsw("GR4HIP_FIR_NO_BF16X3", 0)
    assert e_bf <= 3e-6 and e_bf <= 3 * e_32 + 1e-7, (e_bf, e_32)


def _dev16(x):
    t = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")[4:]  # 16-byte aligned start
    t.copy_(torch.from_numpy(x))
    return t


@pytest.mark.parametrize("ntaps", [33, 65, 81, 113, 146, 200, 256, 400, 1024])
def test_fir_float_f16_two_term_kernel(G, ntaps, devsw):
    """fir_filter<float>, 33 .. 256 taps (and the 256-tap slices of 384 .. 1024), long aligned spans -- the default since round 4: samples and taps as two f16
    terms each under a per-segment block exponent, three products per tap on the f16 matrix pipe (fir_f16.hip).  Against the float64 oracle at the same bar as
    every float32 path, also when the filter removes a tone 30 dB above what passes and across ragged calls; on white noise through a random filter no
    worse than twice the three-term bf16 kernel; and whatever the level of the stream (1e-30 .. 1e30: the block exponent)."""
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    n = 300_000
    x = (O.signal_f32(91, n, tone_frel=0.31, tone_amp=30.0)).astype(np.float32)
    truth, _ = O.fir(b, x)
    cuts = [0, 120_000, 120_004, 121_000, n]

    def run(flt, xx):
        return np.concatenate([flt.process_bulk(_dev16(xx[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    y = run(G.fir_filter(b, torch.float32), x)
    assert _rel(y, truth) <= TOL
    def unguarded():  # (under the guard both kernels hand this stream's segments to the second evaluation: the same float64 sums)
        f = G.fir_filter(b, torch.float32)
        f.set_guard_mode(G.capi.GUARD_OFF)
        return run(f, x)
    yhf = unguarded()
    devsw("GR4HIP_FIR_NO_F16X2", 1)
    ybf = unguarded()
    devsw("GR4HIP_FIR_NO_F16X2", 0)
    assert not np.array_equal(yhf, ybf)  # (two different kernels did run)
    for scale in (1e-30, 1e30):  # a power-of-ten level far from 1: every segment finds its own exponent
        xs_ = (x.astype(np.float64) * scale).astype(np.float32)
        ts, _ = O.fir(b, xs_)
        assert _rel(run(G.fir_filter(b, torch.float32), xs_), ts) <= TOL
    rng = np.random.default_rng(ntaps)
    br = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    xr = O.signal_f32(92, 100_000, tone_amp=0.0)
    tr, _ = O.fir(br, xr)
    e_hf = _rel(G.fir_filter(br, torch.float32).process_bulk(_dev16(xr)).cpu().numpy(), tr)
    fbf = G.fir_filter(br, torch.float32)
    fbf.set_algo(G.capi.FIR_TIME_DOMAIN_BF16X3)
    e_bf = _rel(fbf.process_bulk(_dev16(xr)).cpu().numpy(), tr)
    assert e_hf <= 3e-6 and e_hf <= 2 * e_bf + 1e-7, (e_hf, e_bf)


@pytest.mark.parametrize("ntaps", [257, 300, 383, 384, 777, 1024, 1100, 2048, 3000, 3840])
def test_fir_f16_slices_of_a_long_filter_are_judged_on_their_sum(G, ntaps):
    """fir_filter<float> with 384 .. 1024 taps runs as 256-tap slices that add into y; a slice sees partial sums, so until round 5 these ran unjudged (2e-4 of the
    output under a tone 50 dB above it: worse than the reference's float32 sum).  The LAST slice judges the sums it leaves in y -- the whole filter's outputs -- and marked
    segments are evaluated again with all the taps on the FP64 matrix pipe: below the reference's float32 error (the oracle's sum), factor one; ordinary segments untouched"""
    n = 1 << 18
    b = O.design_taps_hamming_lowpass(ntaps, 0.05)
    x = (O.signal_f32(7, n, tone_amp=0.0) * 0.05).astype(np.float32)
    x[: n // 2] += (316.0 * np.cos(2 * np.pi * 0.31 * np.arange(n // 2))).astype(np.float32)
    truth, _ = O.fir(b, x)
    half = slice(ntaps, n // 2 - 8192), slice(n // 2 + 8192, n)
    y = G.fir_filter(b, torch.float32).process_bulk(_dev16(x)).cpu().numpy()
    off = G.fir_filter(b, torch.float32)
    off.set_guard_mode(G.capi.GUARD_OFF)
    yo = off.process_bulk(_dev16(x)).cpu().numpy()
    e, e_off, e_ref = _rel(y[half[0]], truth[half[0]]), _rel(yo[half[0]], truth[half[0]]), _ref32_err(b, x, truth, half[0])
    assert e_off > 3e-5 and e <= max(TOL, e_ref) and e <= 1e-6, (e, e_off, e_ref)
    assert _rel(y[half[1]], truth[half[1]]) <= TOL and np.array_equal(y[half[1]], yo[half[1]])


@pytest.mark.parametrize("ntaps", [64, 200, 256])
def test_fir_f16_kernel_judges_its_own_segments(G, ntaps):
    """a rejected tone 50 dB above the noise that passes: the error of ANY split-product form is relative to the products and shows against the output (the
    three-term bf16 kernel: ~1e-4, the two-term f16 products by themselves: ~2e-4; the reference's own float32 sum: ~3e-5).  The f16 kernel compares every
    segment's output power with its input power and marks a segment that rejects more than 36 dB of it; the marked segments are evaluated again on the FP64 matrix
    pipe behind the launch (fir_exact.hip) -- the default stays BELOW the reference's float32 error, measured here with the oracle's float32 sum
    (include/gr4hip.h, PARITY CONTRACT); gr4hip_fir_set_guard_mode(GUARD_OFF) shows what it would be without.  Segments of ordinary
    input inside the same stream are not redone (the verdict is per segment): the stream's second half is plain noise and stays on the matrix pipe."""
    n = 1 << 18
    b = O.design_taps_hamming_lowpass(ntaps, 0.1)
    x = (O.signal_f32(7, n, tone_amp=0.0) * 0.05).astype(np.float32)
    t = np.arange(n // 2)
    x[: n // 2] += (316.0 * np.cos(2 * np.pi * 0.31 * t)).astype(np.float32)
    truth, _ = O.fir(b, x)
    half = slice(ntaps, n // 2 - 4096), slice(n // 2 + 8192, n)

    def err(y, sl):
        return _rel(y[sl], truth[sl])
    y = G.fir_filter(b, torch.float32).process_bulk(_dev16(x)).cpu().numpy()
    off = G.fir_filter(b, torch.float32)
    off.set_guard_mode(G.capi.GUARD_OFF)
    yo = off.process_bulk(_dev16(x)).cpu().numpy()
    e_ref = _ref32_err(b, x, truth, half[0])            # the reference's own float32 sum on this input
    assert err(yo, half[0]) > 3e-5                       # the products by themselves, under the interferer
    assert err(y, half[0]) <= max(TOL, e_ref), (err(y, half[0]), e_ref)  # marked and evaluated again (fir_exact.hip): the contract's bound, factor one
    assert err(y, half[0]) <= 1e-6                       # (in fact the float64 sums rounded once)
    assert err(y, half[1]) <= TOL and np.array_equal(y[half[1]], yo[half[1]])  # ordinary segments: the matrix-pipe result, untouched


def test_fir_f16_kernel_outliers_and_non_finite_samples(G):
    """the block exponent's blind spot, closed: a finite glitch of 1e30 (and one of 3.4e38, an Inf, a NaN) among unit-power samples would push a whole segment's
    ordinary samples below the f16 planes' floor -- the kernel sees the spread (largest magnitude against the smallest per-lane maximum) and gives such a
    segment to the float32 path: the classes and the reach of the non-finite values are the reference's (exactly ntaps outputs), and every other output of the
    stream is inside the parity bar"""
    n, ntaps = 300_000, 200
    b = O.design_taps_hamming_lowpass(ntaps, 0.1)
    x = O.signal_f32(7, n)
    pos = {"glitch": 30_001, "inf": 90_003, "nan": 150_005, "big": 210_007}
    x[pos["glitch"]] = 1e30
    x[pos["inf"]] = -np.inf
    x[pos["nan"]] = np.nan
    x[pos["big"]] = 3.4e38
    truth, _ = O.fir(b, x)
    with np.errstate(over="ignore", invalid="ignore"):
        t32 = truth.astype(np.float32)
    xc = x.copy()
    xc[list(pos.values())] = 0
    rms = float(np.sqrt(np.mean(O.fir(b, xc)[0] ** 2)))
    y = G.fir_filter(b, torch.float32).process_bulk(_dev16(x)).cpu().numpy()
    assert np.array_equal(np.isnan(y), np.isnan(t32)) and np.array_equal(np.isposinf(y), np.isposinf(t32)) and np.array_equal(np.isneginf(y), np.isneginf(t32))
    ok = np.isfinite(t32)
    near = np.zeros(n, bool)
    for m in (pos["glitch"], pos["big"]):
        near[m: m + ntaps] = True
    assert float(np.max(np.abs(y[ok & ~near] - truth[ok & ~near]) / np.maximum(np.abs(truth[ok & ~near]), rms))) <= TOL  # the ordinary outputs, at THEIR level
    assert float(np.max(np.abs(y[ok & near] - truth[ok & near]) / np.maximum(np.abs(truth[ok & near]), 1e-3 * np.abs(truth[ok & near]).max()))) <= TOL  # under the glitches: relative to them


def _dev16c(x):
    t = torch.empty(x.size + 2, dtype=torch.complex64, device="cuda")[2:]  # 16-byte aligned start
    t.copy_(torch.from_numpy(x))
    return t


@pytest.mark.parametrize("ntaps", [33, 64, 97, 200, 256])
def test_fir_complex_f16_two_term_kernel(G, ntaps, devsw):
    """fir_filter<complex<float>>, 33 .. 256 taps, the direct form on long aligned spans (GR4HIP_FIR_TIME_DOMAIN; the default up to 96 taps) -- since round 4 the
    two-term f16 kernel on both components under one block exponent (fir_f16.hip): the float64 oracle's bar with a rejected tone 30 dB above what passes, across
    ragged calls, at any level of the stream; a rejected tone 50 dB above the noise is judged per segment and redone with float32 products (the error of the
    float32 kernel, where the products by themselves -- guard off -- are an order of magnitude above it)"""
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    n = 200_000
    x = O.signal_c32(91, n, tone_frel=0.31, tone_amp=30.0)
    truth, _ = O.fir(b, x)
    cuts = [0, 90_000, 90_002, 91_000, n]

    def make(algo=None, guard=None):
        f = G.fir_filter(b, torch.complex64)
        f.set_algo(G.capi.FIR_TIME_DOMAIN if algo is None else algo)
        if guard is not None:
            f.set_guard_mode(guard)
        return f

    def run(flt, xx):
        return np.concatenate([flt.process_bulk(_dev16c(xx[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    y = run(make(), x)
    assert _rel(y, truth) <= TOL
    ybf = run(make(G.capi.FIR_TIME_DOMAIN_BF16X3), x)
    assert _rel(ybf, truth) <= TOL
    # (under the guard both kernels hand this stream's segments to the same second evaluation; with the guard off each shows its own products)
    assert not np.array_equal(run(make(guard=G.capi.GUARD_OFF), x), run(make(G.capi.FIR_TIME_DOMAIN_BF16X3, G.capi.GUARD_OFF), x))  # (two different kernels did run)
    for scale in (1e-30, 1e30):
        xs_ = (x.astype(np.complex128) * scale).astype(np.complex64)
        ts, _ = O.fir(b, xs_)
        assert _rel(run(make(), xs_), ts) <= TOL
    # a rejected tone 50 dB above the noise
    bw = O.design_taps_hamming_lowpass(ntaps, 0.1)
    xi = (O.signal_c32(7, n, tone_amp=0.0) * 0.05).astype(np.complex64)
    xi += (316.0 * np.exp(2j * np.pi * 0.31 * np.arange(n))).astype(np.complex64)
    ti, _ = O.fir(bw, xi)
    sl = slice(ntaps, n)

    def go(algo=None, guard=None):
        f = G.fir_filter(bw, torch.complex64)
        f.set_algo(G.capi.FIR_TIME_DOMAIN if algo is None else algo)
        if guard is not None:
            f.set_guard_mode(guard)
        return _rel(f.process_bulk(_dev16c(xi)).cpu().numpy()[sl], ti[sl])
    e_def, e_off, e_ref = go(), go(guard=G.capi.GUARD_OFF), _ref32_err(bw, xi, ti, sl)
    assert e_off > 3e-5 and e_def <= max(TOL, e_ref) and e_def <= 1e-6, (e_def, e_off, e_ref)  # the contract's bound (the reference's float32 sum), factor one


@pytest.mark.parametrize("ntaps", [257, 300, 480, 496, 512, 777, 1000, 1024, 1500, 1792])
def test_fir_complex_long_filters_as_slices_on_the_f16_kernel(G, ntaps):
    """round 5: fir_filter<complex<float>> with 257 .. 1024 taps on long aligned spans = slices of 256 taps on the two-term f16 kernel, each a pass over the input delayed by 256 p
    samples that adds to y (until then: the f32 matrix pipe at its peak, 36 Gsamples/s at 512 taps); the last slice judges the SUMS against the whole filter's threshold and the marked
    segments are evaluated again with all the taps in float64.  Ragged calls (short ones take the other kernels: the history is one), any level of the stream, a rejected tone 30 dB
    above what passes, and one 50 dB above the noise against the reference's float32 sum (factor one).  480 / 496 taps: a last slice of 224 / 240 taps is the 8-K-step shape,
    which runs the 9-step kernel on zero-padded taps."""
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    n = 400_000
    x = O.signal_c32(91, n, tone_frel=0.31, tone_amp=30.0)
    truth, _ = O.fir(b, x)
    cuts = [0, 150_000, 150_002, 151_000, n]

    def run(flt, xx):
        return np.concatenate([flt.process_bulk(_dev16c(xx[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _rel(run(G.fir_filter(b, torch.complex64), x), truth) <= TOL
    for scale in (1e-30, 1e30):
        xs_ = (x.astype(np.complex128) * scale).astype(np.complex64)
        ts, _ = O.fir(b, xs_)
        assert _rel(run(G.fir_filter(b, torch.complex64), xs_), ts) <= TOL
    bw = O.design_taps_hamming_lowpass(ntaps, 0.1)
    xi = (O.signal_c32(7, n, tone_amp=0.0) * 0.05).astype(np.complex64)
    xi += (316.0 * np.exp(2j * np.pi * 0.31 * np.arange(n))).astype(np.complex64)
    ti, _ = O.fir(bw, xi)
    sl = slice(ntaps, n)
    f = G.fir_filter(bw, torch.complex64)
    e_def = _rel(f.process_bulk(_dev16c(xi)).cpu().numpy()[sl], ti[sl])
    assert e_def <= max(TOL, _ref32_err(bw, xi, ti, sl)) and e_def <= 2e-6, e_def
    xn = x.copy(); xn[250_000] = np.nan + 0j; xn[300_000] = np.inf  # non-finite samples: the segments that hold one are evaluated again as plain sums
    got = G.fir_filter(b, torch.complex64).process_bulk(_dev16c(xn)).cpu().numpy()
    tn, _ = O.fir(b, xn)
    fin = np.isfinite(tn)
    assert np.array_equal(np.isfinite(got), fin) and _rel(got[fin], tn[fin]) <= TOL


@pytest.mark.parametrize("decim,ntaps", [(8, 1024), (2, 64), (3, 600), (4, 100), (10, 1000), (5, 91), (16, 4096), (16, 512), (16, 33), (32, 1024), (32, 7), (64, 2048), (64, 100), (64, 1),
                                         (11, 352), (12, 384), (20, 333), (24, 100), (25, 800), (48, 1536), (100, 1000), (96, 1536),
                                         (2, 256), (2, 258), (2, 17), (3, 243), (4, 228), (5, 213), (7, 100), (9, 152), (9, 153), (6, 1)])
def test_fir_decimating_long_input_mfma(G, decim, ntaps):
    """float polyphase decimator, >= 16 taps per phase, >= 2^14 outputs per span: phase products summed on the MFMA units; decimation by 2 .. 9 with short branches:
    the band form with three-term bf16 products; decimation by 10 .. 128: the band form (samples in stream order, the decimation in the A operand, the four waves of a tile splitting the K-steps)"""
    rng = np.random.default_rng(ntaps + decim)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    cuts = [0, 40 * decim, (40 + 20_003) * decim, (40 + 20_003 + 7) * decim, (40 + 20_003 + 7 + 16_384) * decim]
    x = O.signal_f32(13, cuts[-1])
    truth, _ = O.fir_decim(b, x, decim)
    f = G.fir_filter(b, torch.float32, decimate=decim)
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _rel(y, truth) <= TOL


@pytest.mark.parametrize("decim,ntaps", [(8, 64), (8, 87), (8, 88), (8, 256), (8, 520), (2, 16), (2, 130), (2, 1), (3, 100), (4, 128), (4, 33), (5, 91), (7, 33), (10, 80), (12, 200),
                                         (16, 64), (16, 256), (16, 460), (16, 1), (16, 600), (17, 64), (16, 33), (16, 449), (16, 450), (32, 64), (32, 256), (32, 321), (32, 322)])
def test_fir_complex_decimating_long_input_matrix_pipe(G, decim, ntaps):
    """complex<float> samples x real taps, decimate by 2 .. 16, >= 2^14 outputs per span: the float decimator's band-form kernels (three-term bf16 products) on the
    interleaved stream read as floats -- the rows of a tile alternate between the re and im phases of the window; shapes beyond their windows (and decimation 17)
    stay on the register-window kernel.  Since late round 4 decimation 16 / 32 (33 .. 449 / 321 taps) and 8 (64 .. 513 taps) take the f16 band-form kernel of
    fir_decim_f16.hip the same way (the interleaving in its tap table).  Against the float64 oracle, across calls that switch kernels"""
    rng = np.random.default_rng(1000 * ntaps + decim)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    cuts = [0, 40 * decim, (40 + 20_003) * decim, (40 + 20_003 + 7) * decim, (40 + 20_003 + 7 + 16_384) * decim, (40 + 20_003 + 7 + 16_384 + 33_000) * decim]
    x = O.signal_c32(17, cuts[-1])
    truth = O.fir(b, x, acc64=True)[0][::decim]
    f = G.fir_filter(b, torch.complex64, decimate=decim)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        xin = torch.empty(hi - lo + 2, dtype=torch.complex64, device="cuda")[2:]  # 16-byte aligned start
        xin.copy_(torch.from_numpy(x[lo:hi]))
        parts.append(f.process_bulk(xin).cpu().numpy())
    y = np.concatenate(parts)
    assert y.shape == truth.shape and _rel(y, truth) <= TOL



@pytest.mark.parametrize("cplx,D,ntaps", [(True, 100, 40), (True, 128, 1000), (False, 200, 500), (False, 1000, 3), (True, 1000, 1), (False, 129, 4000)])
def test_fir_shapes_beyond_every_tiling(G, cplx, D, ntaps):
    """BasicDecimatingFilter takes any `decimate` a user types (time_domain_filter.hpp:190-204): decimation x taps beyond every LDS tiling of the tiled kernels
    (complex data decimated by 100, float by more than 128) -- until round 5 GR4HIP_UNSUPPORTED -- runs on the one-output-per-lane kernel, the reference's sum term for
    term; ragged calls carry the history"""
    rng = np.random.default_rng(D + ntaps)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    n = D * 3000
    x = O.signal_c32(3, n) if cplx else O.signal_f32(3, n)
    truth = O.fir(b, x)[0][::D]
    f = G.fir_filter(b, torch.complex64 if cplx else torch.float32, decimate=D)
    cuts = [0, D * 7, D * 1000, n]
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert y.shape == truth.shape and _rel(y, truth) <= TOL


@pytest.mark.parametrize("cplx,D,ntaps,algo,short", [
    (True, 2, 300, "FIR_AUTO", False),            # the register-window kernel (fir_poly_kernel): the phase-by-phase float32 sum measured 12 x the reference's order on this shape
    (True, 2, 256, "FIR_EXACT_F32", False),
    (False, 3, 64, "FIR_AUTO", True),             # spans below the matrix-pipe kernels' sizes: the register-window kernel at every shape
    (False, 1, 32, "FIR_AUTO", False),
    (True, 1, 48, "FIR_AUTO", True),
    (False, 10, 256, "FIR_AUTO", False),          # float32 matrix-pipe forms (fir_decim_band_kernel / fir_mfma_decim_kernel): fir_judge_kernel + fir_exact_kernel behind them
    (False, 10, 100, "FIR_AUTO", False),
    (True, 10, 64, "FIR_AUTO", False),
    (False, 12, 300, "FIR_AUTO", False),
    (False, 1, 200, "FIR_TIME_DOMAIN_F32", False),   # the float32 / three-term bf16 direct forms a caller names
    (False, 1, 200, "FIR_TIME_DOMAIN_BF16X3", False),
    (True, 1, 200, "FIR_TIME_DOMAIN_F32", False),
    (True, 1, 128, "FIR_TIME_DOMAIN_BF16X3", False),
    (False, 1, 700, "FIR_TIME_DOMAIN_BF16X3", False),
    (False, 5, 300, "FIR_AUTO", False), (True, 4, 256, "FIR_AUTO", False), (True, 5, 256, "FIR_AUTO", False),  # three-term bf16 band forms (judged inside the kernel)
])
def test_fir_every_kernel_answers_to_the_guard(G, cplx, D, ntaps, algo, short):
    """the parity contract's second clause for EVERY kernel gr4hip_fir_process can take, not only the split-product ones: a rejected tone 36 .. 70 dB above what passes.
    Each kernel judges its segments (or fir_judge_kernel does behind it) and the marked ones are evaluated again with float64 products and sums (fir_exact.hip; inside the
    workgroup for the register-window kernel): the result is within the float64 oracle's bar, or -- where even that is out of float32's reach -- within the error of the
    reference's own float32 sum in the reference's order (oracle: gr4o_fir_f32 / _c32), factor ONE"""
    rng = np.random.default_rng(ntaps + D)
    n = (D * 4 * 1_000) if short else (D * 4 * 40_000 if D > 1 else 1 << 18)
    b = O.design_taps_hamming_lowpass(ntaps, 0.4 / D if D > 1 else 0.05)
    for amp, fq in ((3.0, 0.27), (300.0, 0.44), (30.0, 0.31)):
        ph = 2 * np.pi * fq * np.arange(n)
        x = 0.05 * (rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)) + amp * (np.exp(1j * ph) if cplx else np.cos(ph))
        x = x.astype(np.complex64 if cplx else np.float32)
        truth = O.fir(b, x)[0][::D]
        f = G.fir_filter(b, torch.complex64 if cplx else torch.float32, decimate=D)
        f.set_algo(getattr(G.capi, algo))
        cuts = [0, (n // D // 3) * D, n]  # two calls: the second starts from a carried history
        y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
        sl = slice(ntaps // D + 1, None)
        e, e_ref = _rel(y[sl], truth[sl]), _ref32_err(b, x, truth, sl, D)
        assert e <= max(TOL, e_ref), (amp, fq, e, e_ref)


@pytest.mark.parametrize("D,ntaps", [(8, 97), (8, 169), (8, 257), (8, 258), (8, 513), (8, 514), (8, 769), (8, 770), (8, 1024), (8, 1025),
                                     (16, 33), (16, 129), (16, 130), (16, 385), (16, 386), (16, 897), (32, 64), (32, 129), (32, 130), (32, 641),
                                     (4, 33), (4, 64), (4, 321), (4, 322), (4, 577), (4, 578), (4, 1025)])  # (round 5: decimate by 4 on the same kernel, eight tile rows per column)
def test_fir_decimate_by_8_16_32_f16_band_kernel(G, D, ntaps, devsw):
    """BasicDecimatingFilter<float>, decimate by 8 (97 .. 1025 taps), 16 (33 .. 897) and 32 (33 .. 641), long aligned spans -- the default since late round 4: the band form on the f16 matrix pipe
    (fir_decim_f16.hip; the window sizes 3 / 5 / 7 / 9 K-steps per wave at their edges).  The float64 oracle's bar across ragged calls and at any level of the stream
    (the per-segment block exponent); a glitch of 1e30 and an Inf among ordinary samples (such segments are evaluated as float32 sums: the reference's classes on exactly
    the outputs whose window holds the sample, every other output at its own level); a rejected tone 50 dB above the output: judged per segment, the marked segments evaluated again on the FP64
    matrix pipe (fir_exact.hip) -- below the error of the reference's own float32 sum (the oracle's, the contract's factor ONE), where the two-term products alone (guard off)
    are several times above it"""
    rng = np.random.default_rng(ntaps)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    U = D * 4 * max(1, 8 // D)  # (decimate by 4: twice as many outputs, so that every call still is >= 2^17 samples)
    n = U * 15_000
    cuts = [0, U * 5_001, U * 5_001 + U * 4_250, n]  # (calls of >= 2^17 samples, 16-byte aligned)
    x = O.signal_f32(31, n)

    def run(xx, taps=b, guard=None):
        f = G.fir_filter(taps, torch.float32, decimate=D)
        if guard is not None:
            f.set_guard_mode(guard)
        return np.concatenate([f.process_bulk(dev(xx[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    truth, _ = O.fir_decim(b, x, D)
    y = run(x)
    assert y.shape == truth.shape and _rel(y, truth) <= TOL
    devsw("GR4HIP_FIR_NO_DECIM_F16", 1)
    assert not np.array_equal(y, run(x))  # (another kernel without it)
    devsw("GR4HIP_FIR_NO_DECIM_F16", 0)
    for scale in (1e-30, 1e30):
        xs_ = (x.astype(np.float64) * scale).astype(np.float32)
        ts, _ = O.fir_decim(b, xs_, D)
        assert _rel(run(xs_), ts) <= TOL
    # outliers and a non-finite sample
    xo = x.copy()
    xo[100_003], xo[300_005] = 1e30, np.inf
    to, _ = O.fir_decim(b, xo, D)
    with np.errstate(over="ignore", invalid="ignore"):
        t32 = to.astype(np.float32)
    yo = run(xo)
    assert np.array_equal(np.isnan(yo), np.isnan(t32)) and np.array_equal(np.isposinf(yo), np.isposinf(t32)) and np.array_equal(np.isneginf(yo), np.isneginf(t32))
    ok = np.isfinite(t32)
    near = np.zeros(len(to), bool)
    near[100_003 // D: (100_003 + ntaps) // D + 1] = True
    rms = float(np.sqrt(np.mean(truth ** 2)))
    assert float(np.max(np.abs(yo[ok & ~near] - to[ok & ~near]) / np.maximum(np.abs(to[ok & ~near]), rms))) <= TOL
    assert float(np.max(np.abs(yo[ok & near] - to[ok & near]) / np.maximum(np.abs(to[ok & near]), 1e-3 * np.abs(to[ok & near]).max()))) <= TOL
    # a rejected tone 50 dB above the noise through an anti-alias low-pass
    bl = O.design_taps_hamming_lowpass(ntaps, 0.4 / D)
    xi = (O.signal_f32(7, n, tone_amp=0.0) * 0.05 + 316.0 * np.cos(2 * np.pi * 0.31 * np.arange(n))).astype(np.float32)
    ti, _ = O.fir_decim(bl, xi, D)
    sl = slice(ntaps // D + 1, None)
    e_def, e_off = _rel(run(xi, bl)[sl], ti[sl]), _rel(run(xi, bl, G.capi.GUARD_OFF)[sl], ti[sl])
    e_ref = _ref32_err(bl, xi, ti, sl, D)  # the reference's own float32 sum (BasicDecimatingFilter::processBulk keeps every D-th of it)
    assert e_off > 1.5 * e_def and e_def <= max(TOL, e_ref) and e_def <= 1e-6, (e_def, e_off, e_ref)  # the contract's bound, factor one


@pytest.mark.parametrize("D,ntaps", [(8, 64), (8, 97), (8, 256), (8, 513), (16, 33), (16, 200), (16, 449), (32, 64), (32, 321), (4, 33), (4, 161), (4, 162), (4, 289), (4, 513)])
def test_fir_complex_decimate_f16_band_kernel_levels_outliers_and_rejected_tone(G, D, ntaps, devsw):
    """BasicDecimatingFilter<complex<float>> with real taps on the f16 band-form kernel (the interleaved stream read as floats, the interleaving in the tap table): the float64
    oracle's bar at any level of the stream; a glitch of 1e30 in a re and an Inf in an im component -- the reference's classes on exactly the outputs (and the components) whose
    window holds the sample, the other component of the same outputs finite and at its own level (real taps never mix the two); a rejected tone 50 dB above the output
    evaluated again inside the kernel"""
    rng = np.random.default_rng(ntaps + D)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    U = D * 4 * max(1, 8 // D)
    n = U * 12_000
    cuts = [0, U * 4_001, U * 4_001 + U * 4_250, n]
    x = O.signal_c32(37, n)

    def oracle(taps, xx):  # (real taps never mix the components: the float oracle on each)
        xx = xx.astype(np.complex128)
        re, im = O.fir_decim(taps, xx.real.astype(np.float32), D)[0], O.fir_decim(taps, xx.imag.astype(np.float32), D)[0]
        out = np.empty(len(re), np.complex128)  # (not re + 1j * im: 0 x Inf)
        out.real, out.imag = re, im
        return out

    def run(xx, taps=b, guard=None):
        f = G.fir_filter(taps, torch.complex64, decimate=D)
        if guard is not None:
            f.set_guard_mode(guard)
        return np.concatenate([f.process_bulk(dev(xx[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    truth = oracle(b, x)
    y = run(x)
    assert y.shape == truth.shape and _rel(y, truth) <= TOL
    devsw("GR4HIP_FIR_NO_DECIM_F16", 1)
    assert not np.array_equal(y, run(x))  # (another kernel without it)
    devsw("GR4HIP_FIR_NO_DECIM_F16", 0)
    for scale in (1e-30, 1e30):
        xs_ = (x.astype(np.complex128) * scale).astype(np.complex64)
        ts = oracle(b, xs_)
        assert _rel(run(xs_), ts) <= TOL
    xo = x.copy()
    xo[100_003] = complex(1e30, xo[100_003].imag)
    xo[300_005] = complex(xo[300_005].real, np.inf)
    to = oracle(b, xo)
    yo = run(xo)
    rms = float(np.sqrt(np.mean(np.abs(truth) ** 2)))
    for part in (np.real, np.imag):
        with np.errstate(over="ignore", invalid="ignore"):
            t32 = part(to).astype(np.float32)
        yp, tp = part(yo), part(to)
        assert np.array_equal(np.isnan(yp), np.isnan(t32)) and np.array_equal(np.isposinf(yp), np.isposinf(t32)) and np.array_equal(np.isneginf(yp), np.isneginf(t32))
        ok = np.isfinite(t32)
        near = np.zeros(len(to), bool)
        if part is np.real:
            near[100_003 // D: (100_003 + ntaps) // D + 1] = True
        assert float(np.max(np.abs(yp[ok & ~near] - tp[ok & ~near]) / np.maximum(np.abs(tp[ok & ~near]), rms))) <= TOL
        if near.any():
            assert float(np.max(np.abs(yp[ok & near] - tp[ok & near]) / np.maximum(np.abs(tp[ok & near]), 1e-3 * np.abs(tp[ok & near]).max()))) <= TOL
    assert np.isfinite(np.imag(yo)[100_003 // D: (100_003 + ntaps) // D + 1]).all() and np.isfinite(np.real(yo)[300_005 // D: (300_005 + ntaps) // D + 1]).all()
    bl = O.design_taps_hamming_lowpass(ntaps, 0.4 / D)
    xi = (O.signal_c32(7, n, tone_amp=0.0) * 0.05 + 316.0 * np.exp(2j * np.pi * 0.31 * np.arange(n))).astype(np.complex64)
    ti = oracle(bl, xi)
    sl = slice(ntaps // D + 1, None)
    e_def, e_off = _rel(run(xi, bl)[sl], ti[sl]), _rel(run(xi, bl, G.capi.GUARD_OFF)[sl], ti[sl])
    e_ref = _ref32_err(bl, xi, ti, sl, D)  # the reference's own float32 sum on both components
    assert e_off > 1.5 * e_def and e_def <= max(TOL, e_ref) and e_def <= 1e-6, (e_def, e_off, e_ref)  # the contract's bound, factor one


@pytest.mark.parametrize("ntaps", [1024, 1000, 513, 129, 8, 1])
def test_fir_decimate_by_8_frequency_domain(G, ntaps, devsw):
    """BASELINE configs[2]'s filter: decimate by 8, <= 1024 taps, spans of >= 64 blocks of 7168 samples take the overlap-save kernel (csrc/fir_decim_fd.hip:
    4096-point complex transform, one table product, 1024-point inverse per block); against the float64 oracle, across calls (history from the handle, then
    from the previous span), with ragged remainders going to the polyphase kernels, and against the polyphase path on the same input"""
    rng = np.random.default_rng(ntaps)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32) if ntaps > 1 else np.array([0.7], np.float32)
    blk = 7168
    cuts = [0, 64 * blk + 8 * 37, 64 * blk + 8 * 37 + 8 * 5, 2 * (64 * blk) + 8 * 100, 2 * (64 * blk) + 8 * 100 + 70 * blk]
    x = O.signal_f32(31, cuts[-1])
    truth, _ = O.fir_decim(b, x, 8)
    def run():
        f = G.fir_filter(b, torch.float32, decimate=8)
        return np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    y16 = run()  # the default since late round 4: 97 .. 1025 taps on the f16 band-form kernel (fir_decim_f16.hip), the rest as below
    assert y16.shape == truth.shape and _rel(y16, truth) <= TOL
    devsw("GR4HIP_FIR_NO_DECIM_F16", 1)  # the frequency-domain kernel
    y = run()
    assert y.shape == truth.shape and _rel(y, truth) <= TOL
    assert (ntaps < 97) == np.array_equal(y, y16)  # (two different kernels did run where the f16 one applies)
    devsw("GR4HIP_FIR_NO_DECIM_FD", 1)  # developer switch: the polyphase (MFMA / VALU) kernels on the same stream
    y2 = run()
    devsw("GR4HIP_FIR_NO_DECIM_FD", 0)
    devsw("GR4HIP_FIR_NO_DECIM_F16", 0)
    assert _rel(y2, truth) <= TOL
    assert _rel(y, truth) <= _rel(y2, truth) + 2e-6  # as accurate as the direct form, to 1/5 of the tolerance
    assert _rel(y16, truth) <= _rel(y2, truth) + 2e-6


@pytest.mark.parametrize("kind", ["float", "complex", "decim"])
def test_fir_random_span_sizes_switch_kernels(G, kind):
    """one stream cut into random spans: every call picks its kernel by size (register-window VALU / MFMA / frequency-domain), the
    history has to survive every switch"""
    rng = np.random.default_rng({"float": 1, "complex": 2, "decim": 3}[kind])
    if kind == "float":
        b, decim, total, big = (rng.standard_normal(100) / 10).astype(np.float32), 1, 1_200_000, 200_000
        x = O.signal_f32(21, total)
        truth, _ = O.fir(b, x)
        f = G.fir_filter(b, torch.float32)
    elif kind == "complex":
        b, decim, total, big = (rng.standard_normal(91) / 9).astype(np.float32), 1, 2_200_000, 700_000
        x = O.signal_c32(22, total)
        truth, _ = O.fir(b, x)
        f = G.fir_filter(b, torch.complex64)
    else:
        b, decim, total, big = (rng.standard_normal(1024) / 32).astype(np.float32), 8, 1_600_000, 400_000
        x = O.signal_f32(23, total)
        truth, _ = O.fir_decim(b, x, decim)
        f = G.fir_filter(b, torch.float32, decimate=decim)
    cuts, pos = [0], 0
    while pos < total:
        step = int(rng.choice([rng.integers(1, 300), rng.integers(1000, 70_000), rng.integers(70_000, big)]))
        step = max(decim, step - step % decim)
        pos = min(total, pos + step)
        cuts.append(pos)
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert len(y) == total // decim and _rel(y, truth) <= TOL


@pytest.mark.parametrize("ntaps", [256, 129, 97, 91, 65, 33, 2])
def test_fir_complex_long_input_fast_convolution(G, ntaps, devsw):
    """complex<float>, 97 .. 256 taps, >= 64 frames of 8192: whole frames take the frequency-domain kernel, the rest the direct form;
    history crosses both boundaries (<= 96 taps: the same spans stay on the direct form, which is faster there).  Since round 4 the default for 16-byte-aligned spans
    is the direct form on the f16 matrix pipe at every tap count (as fast, error relative to the output): the fast convolution serves the spans that kernel does not
    take -- the 8-byte-aligned one below -- and is run on the aligned spans here through the developer switch"""
    rng = np.random.default_rng(ntaps)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    n = 3000 + (70 * 8192 + 77) + 5 + 64 * 8192
    x = O.signal_c32(5, n)
    truth, _ = O.fir(b, x)
    cuts = [0, 3000, 3000 + 70 * 8192 + 77, 3000 + 70 * 8192 + 77 + 5, n]  # direct | FD + remainder | direct | FD exactly 64 frames
    ys = []
    for no_f16 in (1, 0):
        devsw("GR4HIP_FIR_NO_F16X2", no_f16)
        f = G.fir_filter(b, torch.complex64)
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            xin = torch.empty(hi - lo + 2, dtype=torch.complex64, device="cuda")[2:]  # 16-byte aligned start
            xin.copy_(torch.from_numpy(x[lo:hi]))
            parts.append(f.process_bulk(xin).cpu().numpy())
        ys.append(np.concatenate(parts))
        assert _rel(ys[-1], truth) <= TOL
    assert ntaps <= 32 or not np.array_equal(ys[0], ys[1])  # (the fast convolution / the bf16 direct form, then the f16 direct form; <= 32 taps: the register-window kernel both times)
    # an input span that is only 8-byte aligned (e.g. an odd ring-buffer position) gives the same answer
    f2 = G.fir_filter(b, torch.complex64)
    xin = torch.empty(n + 1, dtype=torch.complex64, device="cuda")[1:]
    xin.copy_(torch.from_numpy(x))
    assert _rel(f2.process_bulk(xin).cpu().numpy(), truth) <= TOL


@pytest.mark.parametrize("ntaps", [256, 129, 64, 40, 33])
def test_fir_complex_time_domain_on_the_matrix_pipe(G, ntaps):
    """complex<float> direct form (GR4HIP_FIR_TIME_DOMAIN: the regime the dynamic-range guard moves a stream to), 33 .. 256 taps, spans >= 2^15 samples: the
    re and im planes as a block-Toeplitz product on the matrix pipe (bf16 three-term products on 16-byte-aligned spans, the f32 MFMA otherwise); ragged spans, history across the kernel switches, an output that is only 8-byte
    aligned (-> the VALU kernel) gives the same stream"""
    rng = np.random.default_rng(ntaps)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    cuts = [0, 50_001, 50_001 + 300_003, 50_001 + 300_003 + 700, 50_001 + 300_003 + 700 + 40_000, 50_001 + 300_003 + 700 + 40_000 + 150_000]
    x = O.signal_c32(6, cuts[-1])
    truth, _ = O.fir(b, x)
    f = G.fir_filter(b, torch.complex64)
    f.set_algo(G.capi.FIR_TIME_DOMAIN)
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _rel(y, truth) <= TOL
    f2 = G.fir_filter(b, torch.complex64)
    f2.set_algo(G.capi.FIR_TIME_DOMAIN)
    out = torch.empty(cuts[-1] + 1, dtype=torch.complex64, device="cuda")[1:]
    f2.process_bulk(dev(x), out)
    assert _rel(out.cpu().numpy(), truth) <= TOL
    assert float(np.abs(out.cpu().numpy() - y).max()) <= TOL * float(np.sqrt(np.mean(np.abs(truth) ** 2)))  # two float32 summation orders


def test_fir_boxcar_step_golden(G, golden):
    g = golden["fir_iir_step"]
    x = np.ones(g["n_steps"], np.float32)
    x[0] = 0
    y = G.fir_filter(np.full(g["boxcar_taps"], g["boxcar_value"], np.float32)).process_bulk(dev(x)).cpu().numpy()
    np.testing.assert_allclose(y[:11], [0, .1, .2, .3, .4, .5, .6, .7, .8, .9, 1.0], atol=1e-6)
    assert abs(y[-1] - 1.0) < 1e-6


def test_fir_settings_changed_keeps_history(G):
    rng = np.random.default_rng(4)
    x = O.signal_f32(9, 4000)
    b1, b2 = rng.standard_normal(20).astype(np.float32), rng.standard_normal(30).astype(np.float32)
    f = G.fir_filter(b1)
    y1 = f.process_bulk(dev(x[:2000])).cpu().numpy()
    f.settings_changed(b2)  # 30 <= capacity 32: history survives (time_domain_filter.hpp:38-42)
    y2 = f.process_bulk(dev(x[2000:])).cpu().numpy()
    t1, _ = O.fir(b1, x[:2000])
    t2, _ = O.fir(b2, x)  # continuing with full history == filtering the whole stream with b2
    assert _rel(y1, t1) <= TOL and _rel(y2, t2[2000:]) <= TOL


def test_f16_kernels_follow_a_settings_change_in_mid_stream(G):
    """settingsChanged (time_domain_filter.hpp:38-42) between two long calls: the f16 matrix-pipe kernels rebuild their tap tables (fragments, block exponent of the taps,
    guard threshold, the float taps of their float32 paths) and keep the history -- float FIR, complex FIR, decimate-by-8"""
    rng = np.random.default_rng(11)
    n = 8 * 40_000
    for cplx, decim, k1, k2 in ((False, 1, 200, 256), (True, 1, 100, 128), (False, 8, 900, 1024)):
        x = (O.signal_c32 if cplx else O.signal_f32)(9, n)
        b1, b2 = (rng.standard_normal(k1) / np.sqrt(k1)).astype(np.float32), (rng.standard_normal(k2) / np.sqrt(k2)).astype(np.float32)
        f = G.fir_filter(b1, torch.complex64 if cplx else torch.float32, decimate=decim)
        if cplx:
            f.set_algo(G.capi.FIR_TIME_DOMAIN)
        h = n // 2
        y1 = f.process_bulk(dev(x[:h])).cpu().numpy()
        f.settings_changed(b2)  # k2 <= bit_ceil(k1): history survives
        y2 = f.process_bulk(dev(x[h:])).cpu().numpy()
        fd = (lambda bb, xx: O.fir_decim(bb, xx, decim)[0]) if decim > 1 else (lambda bb, xx: O.fir(bb, xx)[0])
        t1, t2 = fd(b1, x[:h]), fd(b2, x)
        assert _rel(y1, t1) <= TOL and _rel(y2, t2[h // decim:]) <= TOL, (cplx, decim)


@pytest.mark.parametrize("decim,ntaps", [(2, 33), (5, 91), (8, 1024), (10, 64), (64, 512)])
def test_decimating_fir_parity(G, decim, ntaps):
    rng = np.random.default_rng(decim)
    b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    n = decim * 6000
    x = O.signal_f32(42, n)
    truth, _ = O.fir_decim(b, x, decim)
    f = G.fir_filter(b, torch.float32, decimate=decim)
    half = decim * 2500
    y = np.concatenate([f.process_bulk(dev(x[:half])).cpu().numpy(), f.process_bulk(dev(x[half:])).cpu().numpy()])
    assert len(y) == n // decim and _rel(y, truth) <= TOL
    with pytest.raises(G.capi.Gr4HipError):
        f.process_bulk(dev(x[: decim + 1]))  # spans must be whole input chunks


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("interp,ntaps", [(2, 33), (3, 91), (8, 1024), (2, 256), (4, 64), (5, 100), (6, 7), (8, 33), (7, 50), (16, 256), (3, 1), (1, 45)])
def test_interpolating_fir_parity(G, interp, ntaps, cplx):
    """north_star "interpolating FIR" (no reference block: SURVEY.md Appendix A definition, own float64 oracle = literal zero-stuffing + the a1 sum, gain L):
    polyphase kernels for L in {2,3,4,5,6,8}, the generic kernel otherwise; ragged calls carry ceil(K/L) - 1 input samples of history"""
    n = 30_011
    b = O.design_taps_hamming_lowpass(ntaps, 0.4 / interp) if ntaps > 1 else np.array([0.75], np.float32)
    x = O.signal_c32(21, n) if cplx else O.signal_f32(21, n)
    truth, _ = O.fir_interp(b, x, interp)
    f = G.fir_interpolator(b, interp, torch.complex64 if cplx else torch.float32)
    cuts = [0, 1, 2, 500, 501, 7000, 7000, 20_001, n]  # incl. an empty call, one-sample calls, spans shorter than the history
    got = np.concatenate([f.process_bulk(dev(x[a:c])).cpu().numpy() for a, c in zip(cuts[:-1], cuts[1:])])
    assert got.shape == truth.shape and _rel(got, truth) <= TOL
    # the same stream in one call, after a reset; and new taps on the live block keep the history (like fir_filter::settingsChanged)
    f.reset()
    assert _rel(f.process_bulk(dev(x)).cpu().numpy(), truth) <= TOL
    if ntaps > 1:
        f.reset()
        y1 = f.process_bulk(dev(x[:5000])).cpu().numpy()
        b2 = (0.5 * b).astype(np.float32)
        f.settings_changed(b2)
        y2 = f.process_bulk(dev(x[5000:9000])).cpu().numpy()
        t1, h = O.fir_interp(b, x[:5000], interp)
        t2, _ = O.fir_interp(b2, x[5000:9000], interp, h)
        assert _rel(np.concatenate([y1, y2]), np.concatenate([t1, t2])) <= TOL
    with pytest.raises(G.capi.Gr4HipError):
        G.fir_interpolator(b, 0)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("interp,ntaps", [(2, 64), (2, 530), (4, 256), (4, 37), (8, 256), (8, 1024), (8, 2168), (16, 256), (16, 5), (7, 128), (12, 100), (20, 333), (48, 96), (100, 1000), (9, 2400)])
def test_interpolating_fir_matrix_pipe_long_streams(G, interp, ntaps, cplx):
    """spans of >= 32768 outputs at L in {2, 4, 8, 16} (G = 16 / L input positions per 16-row tile) and at any other L except 3, 5, 6 (one input
    position per tile, rows = 16 phases at a time): the block-Toeplitz contraction on the f32 matrix pipe (fir_interp_mfma_kernel) -- many segments
    per call, ragged ends, history handed between the matrix-pipe and the register-window / generic kernel"""
    n = 150_003 if interp <= 16 else 40_003
    b = O.design_taps_hamming_lowpass(ntaps, 0.4 / interp)
    x = O.signal_c32(33, n) if cplx else O.signal_f32(33, n)
    truth, _ = O.fir_interp(b, x, interp)
    f = G.fir_interpolator(b, interp, torch.complex64 if cplx else torch.float32)
    assert _rel(f.process_bulk(dev(x)).cpu().numpy(), truth) <= TOL
    hook, rec = G.capi.lib().gr4hip_internal_fir_interp_last_path, (C.c_int * 8)()  # (test hook, not in include/gr4hip.h; tests/test_gpu_fir_interp_paths.py)
    hook.restype, hook.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int)]
    assert hook(f._h, rec) == 0 and rec[0] == 3, tuple(rec)  # the whole-stream call took the matrix-pipe kernel
    f.reset()
    cuts = [0, 70_001, 70_004, 74_100, 140_000, 140_900, n] if interp <= 16 else [0, 20_001, 20_004, 21_000, n]  # long spans (matrix pipe), short ones in between
    got = np.concatenate([f.process_bulk(dev(x[a:c])).cpu().numpy() for a, c in zip(cuts[:-1], cuts[1:])])
    assert got.shape == truth.shape and _rel(got, truth) <= TOL


def test_interpolating_fir_matrix_pipe_many_workgroups(G):
    """a device-generated stream long enough that every workgroup takes 4 segments: against the register-window kernel's definition through the
    polyphase identity -- branch p of the output is an ordinary FIR of the input with taps L b[p::L] (fir_filter, itself oracle-checked)"""
    L, ntaps, n = 8, 256, 1 << 25
    b = O.design_taps_hamming_lowpass(ntaps, 0.4 / L)
    x = G.synth_f32(n, seed=5)
    y = G.fir_interpolator(b, L).process_bulk(x)
    for p in (0, 5):
        ref = G.fir_filter((L * b[p::L]).astype(np.float32)).process_bulk(x)
        d = (y[p::L] - ref).abs().max() / ref.abs().max()
        assert float(d) <= 2e-6


def test_interpolating_fir_random_configurations(G):
    """seeded random draws over the interpolator's parameter space (factor, tap count, real / complex, call lengths on both sides of the matrix-pipe
    threshold): every one against the zero-stuffing oracle"""
    rng = np.random.default_rng(4242)
    for case in range(24):
        L = int(rng.choice([2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 24, 33]))
        ntaps = int(rng.integers(1, min(40 * L, 700)))
        cplx = bool(rng.integers(0, 2))
        n = int(rng.integers(1, 120_000 if L <= 8 else 30_000))
        b = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        x = O.signal_c32(200 + case, n) if cplx else O.signal_f32(200 + case, n)
        truth, _ = O.fir_interp(b, x, L)
        f = G.fir_interpolator(b, L, torch.complex64 if cplx else torch.float32)
        cuts = sorted(set([0, n] + [int(c) for c in rng.integers(0, n + 1, size=3)]))
        got = np.concatenate([f.process_bulk(dev(x[a:c])).cpu().numpy() for a, c in zip(cuts[:-1], cuts[1:])])
        assert got.shape == truth.shape and _rel(got, truth) <= TOL, (case, L, ntaps, cplx, n, cuts)


def test_interpolating_fir_is_the_gain_L_inverse_of_decimation(G):
    """size-independent property at a long device-generated stream: interpolate by L with a 1/L-band low-pass, keep every L-th output of the
    branch-0 phase -> the input delayed by the filter's group delay, to the filter's pass-band ripple"""
    L, ntaps, n = 4, 255, 1 << 20
    b = O.design_taps_hamming_lowpass(ntaps, 0.5 / L)
    x = G.synth_f32(n, seed=3, tone_frel=0.01, noise_amp=0.0)  # a slow tone: well inside the pass band
    y = G.fir_interpolator(b, L).process_bulk(x)
    d = (ntaps - 1) // 2
    back = y[d::L][: n - 1000]  # output sample m L + d is x[m] through the centre tap's phase (unit DC gain after the gain L)
    assert float((back - x[: n - 1000]).abs().max()) <= 2e-3


@pytest.mark.parametrize("dtype_id", range(12))
def test_decimator_bit_exact(G, dtype_id, golden):
    g = golden["decimator"]
    rng = np.random.default_rng(dtype_id)
    raw = rng.integers(0, 256, size=1003 * O.lib().gr4o_dtype_size(dtype_id), dtype=np.uint8)
    x = raw.view(O.NP_DTYPES[dtype_id])
    if dtype_id in (8, 9, 10, 11):
        x = np.nan_to_num(x, nan=1.0, posinf=2.0, neginf=-2.0)
    for decim in (1, 3, g["decim"]):
        y = G.Decimator(decim).process_bulk(dev(x)).cpu().numpy()
        assert np.array_equal(y.view(np.uint8), np.ascontiguousarray(x[::decim]).view(np.uint8))
    assert G.Decimator(g["decim"]).process_bulk(dev(np.arange(g["n_in"], dtype=np.float32))).numel() == g["n_out"]


@pytest.mark.parametrize("nch,ntaps", [(64, 256), (3, 33), (8, 100), (1, 1)])
def test_batched_fir_mfma_parity(G, nch, ntaps):
    """BASELINE.json configs[3]: many-channel FIR on the f32 MFMA units == nch independent fir_filter<float> instances."""
    rng = np.random.default_rng(nch * 1000 + ntaps)
    b = (rng.standard_normal((nch, ntaps)) / np.sqrt(ntaps)).astype(np.float32)
    n = 9000 + 37
    x = np.stack([O.signal_f32(42 + c, n) for c in range(nch)])
    f = G.FirBatched(b)
    cut = 4100  # spans that are not multiples of the 4096-sample segment, history carried per channel
    y = np.concatenate([f.process_bulk(dev(x[:, :cut])).cpu().numpy(), f.process_bulk(dev(x[:, cut:])).cpu().numpy()], axis=1)
    for c in range(nch):
        truth, _ = O.fir(b[c], x[c])
        assert _rel(y[c], truth) <= TOL, c
    f.reset()
    y0 = f.process_bulk(dev(x[:, :100])).cpu().numpy()
    t0, _ = O.fir(b[0], x[0, :100])
    assert _rel(y0[0], t0) <= TOL


def _batched_paths(G, f):
    """bits of the batched dispatcher's path record (test hook of csrc/fir_batched.hip): 1 the f16 kernel, 2 the bf16 one, 3 the f32 MFMA one; 0: a second evaluation behind it"""
    fn = G.capi.lib().gr4hip_internal_fir_batched_last_paths
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint)]
    m = C.c_uint(0xFFFFFFFF)
    assert fn(f._h, C.byref(m)) == 0
    return tuple(k for k in range(32) if m.value >> k & 1)


@pytest.mark.parametrize("switch", [None, "GR4HIP_FIR_NO_F16X2"], ids=["f16", "bf16"])
@pytest.mark.parametrize("nch,ntaps", [(5, 256), (3, 65), (2, 130), (4, 33), (3, 48), (2, 64)])
def test_batched_fir_long_spans_take_the_f16_or_the_bf16_kernel(G, devsw, nch, ntaps, switch):
    """configs[3] at spans of >= 32768 samples per channel and more than 32 taps: per-channel taps as two f16 planes each (fir_f16.hip; the default) or, with
    GR4HIP_FIR_NO_F16X2, as three bf16 planes (fir_bf16.hip), the channels in grid.y; ragged ends, per-channel history handed between that kernel (long spans) and
    the f32 kernel (short ones).  Each call asserts the kernel that served it."""
    rng = np.random.default_rng(nch * 1000 + ntaps)
    b = (rng.standard_normal((nch, ntaps)) / np.sqrt(ntaps)).astype(np.float32)
    n = 90_000 + 36
    x = np.stack([O.signal_f32(142 + c, n) for c in range(nch)])
    f = G.FirBatched(b)
    if switch:
        devsw(switch)
    long_path = (0, 2) if switch else (0, 1)
    cuts = [0, 40_004, 41_000, n]
    ys = []
    for lo, hi, want in zip(cuts[:-1], cuts[1:], (long_path, (3,), long_path)):
        ys.append(f.process_bulk(dev(np.ascontiguousarray(x[:, lo:hi]))).cpu().numpy())
        assert _batched_paths(G, f) == want, (lo, hi)
    y = np.concatenate(ys, axis=1)
    for c in range(nch):
        truth, _ = O.fir(b[c], x[c])
        assert _rel(y[c], truth) <= TOL, c


# ------------------------------------------------------------------ IIR (a3, a4)
def test_iir_forms_golden(G, golden):
    g = golden["fir_iir_step"]
    x = np.ones(g["n_steps"], np.float32)
    x[0] = 0
    truth = O.iir_cascade(O.make_sections([(g["biquad_b"], g["biquad_a"])]), x, O.DF_I)
    for form in range(4):
        y = G.iir_filter(g["biquad_b"], g["biquad_a"], form).process_bulk(dev(x)).cpu().numpy()
        np.testing.assert_allclose(y, truth, atol=g["forms_tolerance"])


def test_iir_ill_conditioned_cascade_takes_the_sequential_form(G):
    """profiles/r03_fuzz_summary.txt: an order-16 / fc = 0.016 Butterworth cascade came out at 7.8e-2 from the parallel-in-time kernels where a float32 CPU cascade
    gets 7.0e-3 -- float32 cannot carry that state through the scan.  GR4HIP_IIR_AUTO measures this at create (three tiles of noise against float64 and against
    the sequential float32 form) and runs such a cascade on GR4HIP_IIR_SEQUENTIAL_F32: the reference's own arithmetic, as close to float64 as the host block.
    A well-conditioned cascade stays on the parallel kernels; the sequential kernel evaluates each of the four forms as the reference writes it"""
    import gnuradio4_amd.blocks as B
    sig = pytest.importorskip("scipy.signal")
    n = 150_000 + 7
    x = O.signal_f32(77, n)
    cuts = [0, 5, 8192, 100_000, n]
    taken = 0
    for sos in (sig.cheby1(16, 1.0, 2 * 0.016, output="sos"), sig.butter(16, 2 * 0.016, output="sos"), sig.cheby1(12, 1.0, 2 * 0.012, output="sos")):  # (the fuzzer's designs)
        b, a = sos[:, :3].astype(np.float32), sos[:, 3:].astype(np.float32)
        secs = [(bb, aa) for bb, aa in zip(b, a)]
        truth = O.iir_cascade(O.make_sections(secs), x, 3, f64=True)  # float64, direct form II transposed (the least state noise)
        cpu32 = O.iir_cascade(O.make_sections(secs), x, O.DF_II, f64=False)
        f = G.iir_filter(b, a)
        algo, e_par, e_seq = f.algo_in_use
        y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
        e_dev, e_cpu = _rel(y, truth), _rel(cpu32, truth)
        if algo == G.capi.IIR_SEQUENTIAL_F32:
            taken += 1
            assert e_par > 1e-5 and e_par > 10 * e_seq > 0, (e_par, e_seq)
            assert e_dev <= 1.5 * e_cpu + 1e-6, (e_dev, e_cpu)   # the reference's float32 arithmetic, no worse
            f.set_algo(G.capi.IIR_PARALLEL)  # on request the scan runs anyway -- and shows what the self-test saw
            assert _rel(f.process_bulk(dev(x)).cpu().numpy(), truth) > 3 * e_dev
        else:  # the scan carries this one: inside the bar, or no worse than ten times the float32 form
            assert e_dev <= max(TOL, 10 * e_cpu), (e_dev, e_cpu)
    assert taken >= 1  # at least one of these cascades is beyond what float32 carries through the scan
    # a well-conditioned cascade: AUTO keeps the parallel kernels
    b8, a8 = B.design_iir(0, 8, 0.05, float("nan"), 1.0, G.capi.BUTTERWORTH)
    f8 = G.iir_filter(b8, a8)
    assert f8.algo_in_use[0] == G.capi.IIR_PARALLEL and 0 <= f8.algo_in_use[1] <= 1e-5
    # the four forms, each in its own arithmetic (the oracle's float32 cascade of the same form), streamed in ragged calls
    secs8 = O.make_sections([(bb, aa) for bb, aa in zip(b8, a8)])
    t8 = O.iir_cascade(secs8, x, 1, f64=True)
    for form in range(4):
        fs = G.iir_filter(b8, a8, form)
        fs.set_algo(G.capi.IIR_SEQUENTIAL_F32)
        assert fs.algo_in_use[0] == G.capi.IIR_SEQUENTIAL_F32
        ys = np.concatenate([fs.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
        want = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b8, a8)]), x, form, f64=False)
        assert _rel(ys, want.astype(np.float64)) <= 2e-6, form   # the same float32 operations up to the order of two- and three-term sums
        assert _rel(ys, t8) <= TOL, form


@pytest.mark.parametrize("order,design", [(1, 0), (2, 0), (8, 0), (4, 2), (5, 3), (6, 1)])
def test_iir_cascade_parity(G, order, design):
    import gnuradio4_amd.blocks as B
    b, a = B.design_iir(0, order, 0.05, float("nan"), 1.0, design)
    n = 300_000 + 11
    x = O.signal_f32(42, n)
    truth = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b, a)]), x, O.DF_II, f64=True)
    f = G.iir_filter(b, a)
    cuts = [0, 5, 8192, 8193, 100_000, n]
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _rel(y, truth) <= TOL
    cpu32 = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b, a)]), x, O.DF_II, f64=False)
    assert _rel(y, truth) <= 2 * _rel(cpu32, truth) + 2e-6


def test_iir_span_beyond_the_memory_side_cache(G):
    """round 5: a span whose input + output exceed 192 MB takes the tiles' loads and stores with streaming (nt) hints (IirSeqArgs::nt, profiles/r05_streaming_hints.txt): the same
    arithmetic -- the whole 2^25-sample span against the float64 oracle, and its state handed to a second call of ragged length"""
    import gnuradio4_amd.blocks as B
    b, a = B.design_iir(0, 8, 0.05, float("nan"), 1.0, G.capi.BUTTERWORTH)
    n1, n2 = (1 << 25) + 4096 * 3 + 7, 70_001
    x = O.signal_f32(7, n1 + n2)
    truth = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b, a)]), x, O.DF_II, f64=True)
    f = G.iir_filter(b, a)
    y = np.concatenate([f.process_bulk(dev(x[:n1])).cpu().numpy(), f.process_bulk(dev(x[n1:])).cpu().numpy()])
    assert _rel(y, truth) <= TOL
    f.status()


def test_iir_status_is_clean_after_long_streams(G):
    """gr4hip_iir_status: where a caller synchronises anyway; a look-back time-out (never observed) would surface here instead of on the next call"""
    bi, ai = G.blocks.design_iir(G.capi.LOWPASS, 8, 0.05, float("nan"), 1.0, G.capi.BUTTERWORTH)
    f = G.iir_filter(bi, ai)
    x = G.synth_f32(1 << 24, seed=2)
    for _ in range(3):
        f.process_bulk(x)
    f.status()
    f.reset()


def _iir_record(G, f, part=0):
    """what the last gr4hip_iir_process call enqueued for (a part of) the handle: (kernel, ORD, padded NSEC, warm_tiles, warm_chunks, tiles_per_wg, grid, nt), kernel
    1 = segment-sequential runs, 2 = look-back single pass, 3 = three-pass, 4 = sequential float32 (the library's test hook; tests/test_gpu_iir_paths.py)"""
    fn = G.capi.lib().gr4hip_internal_iir_last_path
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    rec = (C.c_int * 8)()
    assert fn(f._h, part, rec) == 0
    return tuple(rec)


@pytest.mark.parametrize("mode", ["runs", "three_pass"])
def test_iir_long_stream_crosses_block_scan_groups(G, mode, devsw):
    """2^24 + 2^22 + 5 samples = 2561 blocks, odd tail, against the float64 oracle.  "three_pass" (GR4HIP_IIR_THREE_PASS): more than one 2048-block group of the
    block-level scan iir_pass_b; "runs": what such a span takes by default, the segment-sequential kernel with runs of several tiles per workgroup"""
    import gnuradio4_amd.blocks as B
    b, a = B.design_iir(0, 8, 0.05, float("nan"), 1.0, 0)  # Butterworth order 8 -> 4 biquads (BASELINE configs[2])
    n = (1 << 24) + (1 << 22) + 5
    x = O.signal_f32(7, n)
    truth = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b, a)]), x, O.DF_II, f64=True)
    if mode == "three_pass":
        devsw("GR4HIP_IIR_THREE_PASS", 1)
    blocks = -(-n // 8192)
    f = G.iir_filter(b, a)
    y = f.process_bulk(dev(x)).cpu().numpy()
    rec = _iir_record(G, f)
    if mode == "three_pass":
        assert rec == (3, 2, 4, 0, 0, 1, blocks, 0) and blocks > 2048
    else:
        assert rec[:3] == (1, 2, 4) and rec[3] >= 1 and rec[5] == max(rec[3], -(-blocks // (4 * torch.cuda.get_device_properties(0).multi_processor_count))) and rec[6] == -(-blocks // rec[5])
    assert _rel(y, truth) <= TOL
    f2 = G.iir_filter(b, a)  # the same stream in two calls: state carried across
    y2 = np.concatenate([f2.process_bulk(dev(x[:n // 3])).cpu().numpy(), f2.process_bulk(dev(x[n // 3:])).cpu().numpy()])
    assert _iir_record(G, f2)[0] == rec[0]
    assert _rel(y2, truth) <= TOL


@pytest.mark.parametrize("kind", ["biquad4", "pole1", "order4"])
def test_iir_single_pass_equals_three_pass(G, kind, devsw):
    """the single-pass kernel (decoupled look-back over block states, "one": GR4HIP_IIR_LOOKBACK -- all three filters fade fast and would take the segment-
    sequential runs otherwise), the three-pass kernels and the default route ("runs") are three evaluations of the same scan: they must agree far inside the parity
    tolerance on a span long enough for multi-window look-backs (> 64 blocks of 8192 samples), ragged, in two calls"""
    n = (1 << 21) + 12345
    x = G.synth_f32(n, seed=21)
    if kind == "biquad4":
        b, a = G.blocks.design_iir(G.capi.LOWPASS, 8, 0.05, float("nan"), 1.0, G.capi.BUTTERWORTH)
    elif kind == "pole1":
        b, a = np.array([[0.3]], np.float32), np.array([[1.0, -0.7]], np.float32)
    else:
        b, a = np.array([[0.1, 0.2, 0.3, 0.2, 0.1]], np.float32), np.array([[1.0, -0.9, 0.5, -0.1, 0.02]], np.float32)
    out = {}
    inst = {"biquad4": (2, 4), "pole1": (2, 2), "order4": (4, 1)}[kind]
    for mode in ("runs", "one", "three"):
        devsw("GR4HIP_IIR_LOOKBACK", int(mode == "one"))
        devsw("GR4HIP_IIR_THREE_PASS", int(mode == "three"))
        f = G.iir_filter(b, a)
        y = torch.empty_like(x)
        cut = 700001
        for lo, hi in ((0, cut), (cut, n)):
            f.process_bulk(x[lo:hi], y[lo:hi])
            rec = _iir_record(G, f)
            assert rec[:3] == ({"runs": 1, "one": 2, "three": 3}[mode],) + inst, (mode, rec)
            assert mode == "runs" or rec[3:] == (0, 0, 1, -(-(hi - lo) // 8192), 0), (mode, rec)
        out[mode] = y.double()
    rms = float(out["three"].pow(2).mean().sqrt())
    assert float((out["one"] - out["three"]).abs().max()) <= 2e-5 * rms
    assert float((out["runs"] - out["three"]).abs().max()) <= 2e-5 * rms


@pytest.mark.parametrize("pole", [0.7, 0.998, 0.999, 0.99999])
def test_iir_segment_sequential_runs_match_the_lookback_and_the_oracle(G, pole, devsw):
    """every span takes the segment-sequential kernel when the filter's memory fades inside 1, 2 or 4 tiles (poles 0.7 / 0.998 / 0.999 here, asserted from
    the path record; 0.99999 does not and stays on the look-back): same answers as the look-back kernel and the float64 oracle, in two calls so that run 0 of
    the second call starts from the carried state and not from a warm-up"""
    n = (1 << 22) + (1 << 20) + 4321
    x = O.signal_f32(31, n)
    b, a = np.array([[1.0 - pole, 0.0, 0.0], [0.2, 0.3, 0.2]], np.float32), np.array([[1.0, -pole, 0.0], [1.0, -0.4, 0.2]], np.float32)
    truth = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b, a)]), x, O.DF_II, f64=True)
    out = {}
    for mode in ("runs", "lookback"):
        if mode == "lookback":
            devsw("GR4HIP_IIR_LOOKBACK", 1)
        f = G.iir_filter(b, a)
        cut = (1 << 21) + 777  # both calls are hundreds of tiles: each run as long as its warm-up (more tiles per run: tests/test_gpu_iir_paths.py)
        ys = []
        for lo, hi in ((0, cut), (cut, n)):
            ys.append(f.process_bulk(dev(x[lo:hi])).cpu().numpy())
            rec = _iir_record(G, f)
            warm = {0.7: 1, 0.998: 2, 0.999: 4, 0.99999: 0}[pole]
            if mode == "runs" and warm:
                assert rec[:4] == (1, 2, 2, warm) and rec[4] == (32 if pole == 0.7 else 256) and rec[6] == -(-(-(-(hi - lo) // 8192)) // rec[5]), (pole, rec)
            else:
                assert rec == (2, 2, 2, 0, 0, 1, -(-(hi - lo) // 8192), 0), (pole, mode, rec)
        out[mode] = np.concatenate(ys)
        f.status()
        assert _rel(out[mode], truth) <= TOL, mode
    rms = float(np.sqrt(np.mean(truth ** 2)))
    assert float(np.abs(out["runs"].astype(np.float64) - out["lookback"]).max()) <= 2e-5 * rms


def test_basic_filter_bands(G, golden):
    g = golden["basic_filter_lowpass"]
    fs, n = g["sample_rate"], g["num_samples"]
    for ftype in ("FIR", "IIR"):
        for decim in (1, g["decimation"]):
            for f_hz, ok in ((g["pass_hz"], lambda m: m >= g["pass_min"]), (g["stop_hz"], lambda m: m <= g["stop_max"])):
                flt = G.BasicFilter(filter_type=ftype, filter_response=0, filter_order=g["filter_order"], f_low=g["f_low"], sample_rate=fs,
                                    decimate=decim, iir_design_method=G.capi.CHEBYSHEV1, fir_design_method="Hamming")
                assert flt.input_chunk_size == decim
                x = np.sin(2 * np.pi * f_hz / fs * np.arange(1, 2 * n + 1)).astype(np.float32)
                y = flt.process_bulk(dev(x)).cpu().numpy()
                assert len(y) == 2 * n // decim
                assert ok(np.max(np.abs(y[n // decim:]))), (ftype, decim, f_hz)


# ------------------------------------------------------------------ FFT block (a7-a10)
@pytest.mark.parametrize("N", [2, 4, 8, 16, 64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_fft_spectrum_parity(G, N):
    frames = 5
    x = O.signal_c32(N, frames * N)
    got = G.FFT(N, "None").spectrum(dev(x)).cpu().numpy()
    for f in range(frames):
        truth = O.dft64(x[f * N:(f + 1) * N])
        assert _rel(got[f], truth) <= TOL


@pytest.mark.parametrize("N,window", [(8192, "None"), (8192, "Hann"), (8192, "Kaiser"), (1024, "Hann")])
def test_fft_mag2_frame_pipeline(G, N, window, devsw):
    """|X|^2 of >= 256 frames of 8192 complex samples runs on the fused chain kernel's frame pipeline (no filter): same numbers as the FFT block kernel
    to float rounding, and the float64 oracle's on sampled frames (1024: the block kernel in both cases -- a pipeline variant for the smaller
    sizes measured slower than two block-kernel workgroups per CU and was dropped)"""
    frames = 300 * (8192 // N) + (3 if N < 8192 else 0)
    x = G.synth_c32(frames * N, seed=17)
    F = G.FFT(N, window)
    got = F.mag2(x)
    devsw("GR4HIP_FFT_NO_PIPELINE", 1)
    ref = G.FFT(N, window).mag2(x)
    devsw("GR4HIP_FFT_NO_PIPELINE", 0)
    floor = ref.pow(2).mean(dim=1, keepdim=True).sqrt()
    assert float(((got - ref).abs() / torch.maximum(ref.abs(), floor)).max()) <= TOL
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    xs = x.cpu().numpy()
    for f in (0, 1, 255, 256, frames - 1):
        fr = xs[f * N:(f + 1) * N].astype(np.complex128)
        if wid > 1:
            fr = fr * O.window(wid, N, np.float32).astype(np.float64)  # the block multiplies by its float32 window (fft.hpp:150-157)
        truth = np.abs(O.dft64(fr)) ** 2
        assert _rel(got[f].cpu().numpy(), truth) <= TOL, f


@pytest.mark.parametrize("window", ["None", "Hann"])
def test_fft_spectrum_frame_pipeline(G, window, devsw):
    """the raw spectrum of >= 256 frames of 8192 complex samples takes the same frame pipeline (complex output): same numbers as the FFT block
    kernel to float rounding, and the float64 oracle's on sampled frames; 255 frames stay on the block kernel"""
    N, frames = 8192, 301
    x = G.synth_c32(frames * N, seed=23)
    got = G.FFT(N, window).spectrum(x)
    devsw("GR4HIP_FFT_NO_PIPELINE", 1)
    ref = G.FFT(N, window).spectrum(x)
    devsw("GR4HIP_FFT_NO_PIPELINE", 0)
    floor = ref.abs().pow(2).mean(dim=1, keepdim=True).sqrt()
    assert float(((got - ref).abs() / torch.maximum(ref.abs(), floor)).max()) <= TOL
    few = G.FFT(N, window).spectrum(x[: 255 * N])
    assert torch.equal(few, ref[:255])
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    xs = x.cpu().numpy()
    for f in (0, 255, 256, frames - 1):
        fr = xs[f * N:(f + 1) * N].astype(np.complex128)
        if wid > 1:
            fr = fr * O.window(wid, N, np.float32).astype(np.float64)
        assert _rel(got[f].cpu().numpy(), O.dft64(fr)) <= TOL, f


@pytest.mark.parametrize("N", [3, 5, 12, 100, 131, 257, 521, 1000, 1009, 2039, 3000, 4095])
def test_fft_any_size_bluestein(G, N):
    """sizes that are not a power of two (the reference's Bluestein branch, algorithm/.../fourier/fft.hpp:353-381), <= 4096.  Round 5: chirp lengths M = 256 .. 4096 run the two
    M-point transforms on the compile-time 16 x 16 x R3 plan, register to register (bluestein_fast_kernel); the run-time radix-8 form stays behind a developer switch"""
    frames = 7 if N > 64 else 3  # (not a whole number of workgroups' frames)
    x = O.signal_c32(N, frames * N)
    F = G.FFT(N, "Hann")
    w = O.window(3, N)
    got = F.spectrum(dev(x)).cpu().numpy()
    for f in range(frames):
        truth = O.dft64(x[f * N:(f + 1) * N].astype(np.complex128) * w)
        assert _rel(got[f], truth) <= TOL
    out = F.process_bulk(dev(x))
    mag, ph, re, im = O.fft_block_truth(x[:N], 3)
    assert _rel(out["magnitude"][0].cpu().numpy(), mag) <= TOL and _rel(out["re"][0].cpu().numpy(), re) <= TOL
    if N in (131, 257, 521, 1009, 2039):  # (M = 512 .. 4096: the same spectra from the generic form, from another kernel)
        G.capi.developer_switch("GR4HIP_FFT_BLUESTEIN_GENERIC", 1)
        old = G.FFT(N, "Hann").spectrum(dev(x)).cpu().numpy()
        G.capi.developer_switch("GR4HIP_FFT_BLUESTEIN_GENERIC", 0)
        assert not np.array_equal(old, got) and _rel(old, got.astype(np.complex128)) <= TOL


@pytest.mark.parametrize("N", [6, 12, 15, 45, 100, 243, 360, 1000, 1536, 1920, 3000, 3125, 3750, 4000, 6000, 6561, 7680, 7776, 8000])
def test_fft_smooth_sizes_mixed_radix(G, N):
    """{2,3,5}-smooth sizes that are not powers of two -- the sizes SimdFFT::canProcessSize takes with radix-3 / radix-5 passes (SimdFFT.hpp:348-375, the
    reference benchmark sweeps one: bm_fft.cpp:44-58) -- run as mixed-radix Stockham passes in ONE launch (fft_smooth.hpp: radices 2 .. 16, prime-factor 6 / 10 /
    12 / 15), every output of the block, complex and real input, odd sizes included; truth: the float64 DFT"""
    frames = 7
    x = O.signal_c32(N, frames * N + 3)
    F = G.FFT(N, "Hann")
    w = O.window(3, N)
    got = F.spectrum(dev(x)).cpu().numpy()
    assert got.shape == (frames, N)
    for f in range(frames):
        truth = O.dft64(x[f * N:(f + 1) * N].astype(np.complex128) * w)
        assert _rel(got[f], truth) <= TOL, f
    out = F.process_bulk(dev(x))
    mag, ph, re, im = O.fft_block_truth(x[:N], 3)
    assert _rel(out["magnitude"][0].cpu().numpy(), mag) <= TOL and _rel(out["re"][0].cpu().numpy(), re) <= TOL and _rel(out["im"][0].cpu().numpy(), im) <= TOL
    m2 = F.mag2(dev(x[: frames * N])).cpu().numpy()
    assert _rel(m2, np.abs(got.astype(np.complex128)) ** 2) <= TOL
    if N % 2 == 0:  # real input (computeHalfSpectrum): first N / 2 bins of magnitude / phase
        xr = O.signal_f32(N + 1, frames * N)
        Fr = G.FFT(N, "Hamming", dtype=torch.float32)
        o2 = Fr.process_bulk(dev(xr))
        tm = np.abs(O.dft64(xr[:N].astype(np.complex128) * O.window(2, N)))[: N // 2] * 2.0 / N
        assert _rel(o2["magnitude"][0].cpu().numpy(), tm) <= TOL


def test_fft_every_smooth_size_up_to_8192(G):
    """all 153 {2,3,5}-smooth sizes up to 8192 that are not powers of two (144 on compile-time plans, the single-pass ones on the run-time kernel): two frames each
    against numpy's float64 FFT"""
    sizes = sorted({2 ** a * 3 ** b * 5 ** c for a in range(14) for b in range(9) for c in range(6)} - {2 ** a for a in range(14)})
    sizes = [n for n in sizes if 2 <= n <= 8192]
    assert len(sizes) == 153
    rng = np.random.default_rng(5)
    for N in sizes:
        x = (rng.standard_normal(2 * N) + 1j * rng.standard_normal(2 * N)).astype(np.complex64)
        got = G.FFT(N, "None").spectrum(dev(x)).cpu().numpy()
        want = np.fft.fft(x.astype(np.complex128).reshape(2, N), axis=1)
        assert _rel(got, want) <= TOL, N


@pytest.mark.parametrize("N", [360, 500, 1000, 1200, 1536, 2000, 3000, 3072, 4800, 5000, 6144, 7680, 8000])
def test_fft_smooth_compile_time_plans_match_the_run_time_kernel(G, N, devsw):
    """the common {2,3,5}-smooth sizes have compile-time plans (fft_smooth.hpp: first pass from global memory, last pass emits from registers); the run-time
    mixed-radix kernel computes the same passes -- both against the float64 DFT, and against each other to float32 rounding"""
    frames = 11
    x = O.signal_c32(3 * N + 1, frames * N)
    w = O.window(7, N)  # Blackman-Harris
    outs = {}
    for which in ("compile_time", "run_time"):
        devsw("GR4HIP_FFT_SMOOTH_RUNTIME", 1 if which == "run_time" else 0)
        outs[which] = G.FFT(N, "BlackmanHarris").spectrum(dev(x)).cpu().numpy()
    for f in (0, frames // 2, frames - 1):
        truth = O.dft64(x[f * N:(f + 1) * N].astype(np.complex128) * w)
        assert _rel(outs["compile_time"][f], truth) <= TOL and _rel(outs["run_time"][f], truth) <= TOL, f
    assert _rel(outs["compile_time"], outs["run_time"].astype(np.complex128)) <= 5e-6  # (the two plans take their radices in different orders)


@pytest.mark.parametrize("N", [6000, 10000, 30000, 48000, 65535, 100003, 3 ** 7 * 5 ** 3, 1 << 19])
def test_fft_any_size_beyond_one_workgroup(G, N):
    """sizes SimdFFT takes with radix-3/5 passes (SimdFFT.hpp:348-375: 6000, 10000, 30000, 48000, 3^7 5^3) and sizes the reference sends to Bluestein
    (primes, 2^16 - 1), up to 2^19: chirp convolution over the four-step power-of-two transforms (M up to 2^20); truth: numpy's float64 FFT"""
    frames = 2
    x = O.signal_c32(N, frames * N + 5)
    if N == 1 << 19:
        N -= 1  # the largest size of this path: 2^19 - 1 (M = 2^20); 2^19 itself is a power of two
        x = x[:frames * N + 5]
    F = G.FFT(N, "Hann")
    w = O.window(3, N)
    got = F.spectrum(dev(x)).cpu().numpy()
    assert got.shape == (frames, N)
    # three float32 transforms of M = bit_ceil(2N - 1) points and two chirp products per spectrum.  On white noise the worst bin of every size up to
    # 2^19 - 1 is within 2e-6 of the spectrum's rms (tools/fft_accuracy.py); this test signal is tone-dominated (peaks ~ sqrt(N) above the rms) and the
    # chirp convolution spreads the rounding of the peaks over all bins: 1.3e-5 / 2.0e-5 at N = 273375 / 2^19 - 1 (M = 2^20).  The bar there is 3e-5,
    # 1e-5 for every shorter convolution length
    tol = TOL if 2 * N - 1 <= 1 << 19 else 3e-5
    for f in range(frames):
        assert _rel(got[f], np.fft.fft(x[f * N:(f + 1) * N].astype(np.complex128) * w)) <= tol
    xr = np.ascontiguousarray(x.real[:N & ~1])  # real input, even size: the first N/2 bins of the block's outputs
    if N % 2 == 0:
        out = G.FFT(N, "None", dtype=torch.float32).process_bulk(dev(xr))
        truth = np.fft.fft(xr.astype(np.float64))
        assert _rel(out["magnitude"][0].cpu().numpy(), np.abs(truth[:N // 2]) * 2 / N) <= TOL


def test_fft_multi_kernel_paths_run_in_batches(G):
    """the multi-kernel paths bound their scratch buffers (2^25 complex values each): more frames than one batch holds come out the same"""
    N, frames = 30000, 600  # M = 65536: 512 frames per batch
    x = G.synth_c32(N * frames, seed=3)
    got = G.FFT(N, "None").spectrum(x)
    for f in (0, 511, 512, 599):
        truth = np.fft.fft(x[f * N:(f + 1) * N].cpu().numpy().astype(np.complex128))
        assert _rel(got[f].cpu().numpy(), truth) <= TOL
    N, frames = 1 << 17, 300  # four-step with N1 = 32: 256 frames per batch
    x = G.synth_c32(N * frames, seed=4)
    got = G.FFT(N, "None").mag2(x)
    for f in (0, 255, 256, 299):
        truth = np.abs(np.fft.fft(x[f * N:(f + 1) * N].cpu().numpy().astype(np.complex128))) ** 2
        assert _rel(got[f].cpu().numpy(), truth) <= TOL


@pytest.mark.parametrize("N", [16384, 32768, 65536, 1 << 17, 1 << 18, 1 << 20])
def test_fft_large_power_of_two(G, N):
    """N1 x 4096 four-step pipeline (N1 <= 16: column transforms in registers; 32 .. 256: as frames of the block kernels between two tiled transpositions);
    truth: numpy's float64 FFT (the O(N^2) oracle DFT is checked against it at N = 16384 once)"""
    frames = 2
    x = O.signal_c32(N + 1, frames * N)
    got = G.FFT(N, "None").spectrum(dev(x)).cpu().numpy()
    # the test signal's tone stands sqrt(N) above the noise bins: at 2^20 points one float32 ulp of the peak (6e-8 x 8e5) is already 3.3e-5 of the
    # spectrum's rms, which is what the off-peak bins are measured against.  The bar for 2^20-point transforms is 3e-5 (measured 2.2e-5; on white noise
    # the worst bin is at 1.3e-6, tools/fft_accuracy.py), 1e-5 for every shorter one
    tol = TOL if N < 1 << 20 else 3e-5
    for f in range(frames):
        truth = np.fft.fft(x[f * N:(f + 1) * N].astype(np.complex128))
        assert _rel(got[f], truth) <= tol
    if N == 16384:
        assert _rel(O.dft64(x[:N]), np.fft.fft(x[:N].astype(np.complex128))) <= 1e-9
    if N == 65536:  # round 5: 256 x 256 in two kernels (32 B of HBM traffic per point); the three-kernel four-step pipeline behind the developer switch gives the same spectra
        G.capi.developer_switch("GR4HIP_FFT_FOUR_STEP_64K", 1)
        old = G.FFT(N, "None").spectrum(dev(x)).cpu().numpy()
        G.capi.developer_switch("GR4HIP_FFT_FOUR_STEP_64K", 0)
        assert not np.array_equal(old, got) and _rel(old[0], np.fft.fft(x[:N].astype(np.complex128))) <= tol  # (two different kernels did run)
        xr = O.signal_f32(5, 3 * N)  # real input, Hamming window, the DataSet outputs through the same two kernels: the same values as the four-step pipeline's to rounding
        new_out = G.FFT(N, "Hamming", dtype=torch.float32).process_bulk(dev(xr), ranges=False)
        G.capi.developer_switch("GR4HIP_FFT_FOUR_STEP_64K", 1)
        old_out = G.FFT(N, "Hamming", dtype=torch.float32).process_bulk(dev(xr), ranges=False)
        G.capi.developer_switch("GR4HIP_FFT_FOUR_STEP_64K", 0)
        for key in ("magnitude", "re", "im"):
            a_, b_ = new_out[key].cpu().numpy(), old_out[key].cpu().numpy()
            assert a_.shape == b_.shape and _rel(a_, b_.astype(np.float64)) <= TOL, key
    m2 = G.FFT(N, "Hann").mag2(dev(x)).cpu().numpy()
    w = O.window(3, N)
    t2 = np.abs(np.fft.fft(x[:N].astype(np.complex128) * w)) ** 2
    assert _rel(m2[0], t2) <= TOL
    if N in (16384, 1 << 17):  # float frames through both column-transform variants: the block's real-input outputs
        xr = np.ascontiguousarray(x.real[:2 * N])
        out = G.FFT(N, "Hann", dtype=torch.float32).process_bulk(dev(xr))
        X = np.fft.fft(xr.reshape(2, N).astype(np.float64) * w, axis=1)
        assert _rel(out["magnitude"].cpu().numpy(), np.abs(X[:, :N // 2]) * 2 / N) <= TOL and _rel(out["re"].cpu().numpy(), X[:, N // 2:].real) <= TOL


def test_fft_n16_patterns_golden(G, golden):
    g = golden["fft_n16_patterns"]
    for case in g["cases"]:
        if case.get("iota"):
            x = np.arange(1, 17, dtype=np.complex64)
        elif case.get("alternating"):
            x = (np.arange(16) % 2).astype(np.complex64)
        else:
            x = np.full(16, complex(*case["fill"]), np.complex64)
        sp = G.FFT(16, "None").spectrum(dev(x)).cpu().numpy()[0]
        mag = np.abs(sp) * 2 / 16
        assert int(np.argmax(mag)) == case["peak_index"] and abs(mag.max() - case["peak_amplitude"]) < 1e-4
        assert abs(sp[0].real - case["fft0"][0]) < 1e-4 and abs(sp[0].imag - case["fft0"][1]) < 1e-4


@pytest.mark.parametrize("window", ["None", "Hann", "Hamming", "BlackmanHarris", "Kaiser", "FlatTop"])
@pytest.mark.parametrize("N", [256, 1024, 8192])
def test_fft_block_outputs_parity(G, window, N):
    frames = 3
    x = O.signal_c32(11, frames * N)
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    out = G.FFT(N, window).process_bulk(dev(x))
    for f in range(frames):
        mag, ph, re, im = O.fft_block_truth(x[f * N:(f + 1) * N], wid)
        assert _rel(out["magnitude"][f].cpu().numpy(), mag) <= TOL
        assert _rel(out["re"][f].cpu().numpy(), re) <= TOL and _rel(out["im"][f].cpu().numpy(), im) <= TOL
        # phase: compare where the bin is not numerically empty (atan2 of rounding noise is arbitrary)
        strong = mag > 1e-3 * mag.max()
        d = np.angle(np.exp(1j * (out["phase"][f].cpu().numpy() - ph)))
        assert np.max(np.abs(d[strong])) <= 1e-3
        rg = out["ranges"][f].cpu().numpy()
        for s, name in enumerate(("magnitude", "phase", "re", "im")):
            v = out[name][f].cpu().numpy()
            assert rg[s, 0] == v.min() and rg[s, 1] == v.max()


def test_fft_block_random_configurations(G):
    """seeded random draws over the FFT block's parameter space: size (powers of two up to 65536, Bluestein sizes), window, complex / real input, frames"""
    rng = np.random.default_rng(77)
    names = [w for w in O.WINDOWS]
    sizes = [2, 4, 16, 32, 128, 256, 512, 1024, 4096, 8192, 16384, 3, 7, 60, 100, 1000, 2049, 4095]
    for case in range(30):
        N = int(rng.choice(sizes))
        real = bool(rng.integers(0, 2)) and N % 2 == 0 and N >= 4
        wid = int(rng.integers(0, len(names)))
        frames = int(rng.integers(1, 7))
        x = (O.signal_f32 if real else O.signal_c32)(300 + case, frames * N, tone_frel=float(rng.uniform(0.0, 0.5)), tone_amp=float(rng.uniform(0.0, 1.0)))
        out = G.FFT(N, names[wid], dtype=torch.float32 if real else torch.complex64).process_bulk(dev(x))
        for f in range(frames):
            mag, ph, re, im = O.fft_block_truth(x[f * N:(f + 1) * N], wid)
            what = (case, N, "real" if real else "complex", names[wid], frames, f)
            assert out["magnitude"][f].shape[0] == len(mag), what
            assert _rel(out["magnitude"][f].cpu().numpy(), mag) <= TOL, what
            assert _rel(out["re"][f].cpu().numpy(), re) <= TOL and _rel(out["im"][f].cpu().numpy(), im) <= TOL, what
            strong = mag > 1e-3 * mag.max()
            if strong.any():
                d = np.angle(np.exp(1j * (out["phase"][f].cpu().numpy() - ph)))
                assert np.max(np.abs(d[strong])) <= 1e-3, what
            rg = out["ranges"][f].cpu().numpy()
            for s_, name in enumerate(("magnitude", "phase", "re", "im")):
                v = out[name][f].cpu().numpy()
                assert rg[s_, 0] == v.min() and rg[s_, 1] == v.max(), what


@pytest.mark.parametrize("nsec,order", [(5, 2), (8, 2), (3, 4), (4, 4)])
def test_iir_more_than_eight_state_values_runs_as_two_cascades(G, nsec, order):
    """5 .. 8 biquads / 3 .. 4 fourth-order sections: the first 8 state values' worth of sections and the rest as two cascades one behind the other (each on
    the fast kernels) -- the section order and the float32 stream between sections are the cascade's own; long ragged calls, state across calls, reset"""
    import scipy.signal as sps
    sos = sps.butter(2 * nsec, 0.12, output="sos")
    if order == 2:
        b, a = sos[:, :3], sos[:, 3:]
    else:  # pairs of biquads multiplied out into fourth-order sections
        sos = sps.butter(4 * nsec, 0.12, output="sos")
        b = np.array([np.convolve(sos[2 * i, :3], sos[2 * i + 1, :3]) for i in range(nsec)])
        a = np.array([np.convolve(sos[2 * i, 3:], sos[2 * i + 1, 3:]) for i in range(nsec)])
    b, a = b.astype(np.float32), a.astype(np.float32)
    n = 700_001
    x = O.signal_f32(77, n)
    sec = O.make_sections([(bb, aa) for bb, aa in zip(b, a)])
    truth = O.iir_cascade(sec, x, O.DF_II, f64=True)
    seq32 = O.iir_cascade(sec, x, O.DF_II, f64=False)
    bar = max(TOL, 3 * _rel(seq32, truth))
    f = G.iir_filter(b, a)
    cuts = [0, 5, 300_000, 300_077, n]
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _rel(y, truth) <= bar
    f.reset()
    assert _rel(f.process_bulk(dev(x[:100_000])).cpu().numpy(), truth[:100_000]) <= bar


def test_iir_random_cascades(G):
    """seeded random stable cascades (random pole radii / angles, 1 ... 8 biquads and fourth-order sections), random span lengths and chunkings"""
    rng = np.random.default_rng(31)
    for case in range(16):
        order = int(rng.choice([1, 2, 4]))
        nsec = int(rng.integers(1, (8 if order <= 2 else 4) + 1))
        b, a = [], []
        for _ in range(nsec):
            poles = []
            while len(poles) < order:
                r, th = rng.uniform(0.2, 0.97), rng.uniform(0.05, 3.0)
                if order - len(poles) >= 2:
                    poles += [r * np.exp(1j * th), r * np.exp(-1j * th)]
                else:
                    poles += [rng.uniform(-0.9, 0.9)]
            a.append(np.real(np.poly(poles)))
            b.append(rng.uniform(-1, 1, order + 1) * 0.5)
        b, a = np.array(b, np.float32), np.array(a, np.float32)
        n = int(rng.integers(1, 400_000))
        x = O.signal_f32(500 + case, n)
        truth = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b, a)]), x, O.DF_II, f64=True)
        f = G.iir_filter(b, a)
        cuts = sorted(set([0, n] + [int(c) for c in rng.integers(0, n, size=2)]))
        y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo])
        # lightly damped random cascades are ill-conditioned in float32 whichever way they are evaluated: the bar is the parity tolerance or three times
        # what the reference's own sequential float32 recurrence loses against float64, whichever is larger
        seq32 = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b, a)]), x, O.DF_II, f64=False)
        assert _rel(y, truth) <= max(TOL, 3 * _rel(seq32, truth)), (case, order, nsec, n, cuts, _rel(seq32, truth))


def test_fft_block_db_deg_unwrap_and_peak(G, golden):
    g = golden["fft_block"]
    N = g["N"]
    x = (np.cos(2 * np.pi * g["tone_frel"] * np.arange(N)) + 0.05 * O.gauss_f32(3, N)).astype(np.complex64)
    out = G.FFT(N, "Hann", outputInDb=True, outputInDeg=True, unwrapPhase=True).process_bulk(dev(x))
    mag, ph, _, _ = O.fft_block_truth(x, 3, in_db=True, in_deg=True, unwrap=True)
    assert abs(abs(out["frequency"][int(np.argmax(out["magnitude"][0].cpu().numpy()))]) - g["tone_frel"]) <= 1.0 / N
    assert np.max(np.abs(out["magnitude"][0].cpu().numpy() - mag)) < 1e-3  # dB values
    d = out["phase"][0].cpu().numpy() - ph  # unwrapped degrees: equal up to whole turns at borderline jumps
    assert np.max(np.abs(d - 360.0 * np.round(d / 360.0))) < 0.05
    assert np.mean(np.abs(d) < 0.05) > 0.9


@pytest.mark.parametrize("window", ["Hann", "None"])
@pytest.mark.parametrize("N", [64, 512, 1024, 2048, 8192])
def test_fft_real_input(G, N, window):
    """float frames: N >= 512 run as N/2 complex points + split (z[n] = x[2n] + i x[2n+1]); outputs keep the block's real-input conventions"""
    frames = 5 if N <= 2048 else 3
    x = O.signal_f32(5, frames * N)
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    out = G.FFT(N, window, dtype=torch.float32).process_bulk(dev(x))
    assert out["magnitude"].shape == (frames, N // 2)
    for f in range(frames):
        mag, ph, re, im = O.fft_block_truth(x[f * N:(f + 1) * N], wid)
        assert _rel(out["magnitude"][f].cpu().numpy(), mag) <= TOL
        assert _rel(out["re"][f].cpu().numpy(), re) <= TOL and _rel(out["im"][f].cpu().numpy(), im) <= TOL
        strong = mag > 1e-3 * mag.max()
        d = np.angle(np.exp(1j * (out["phase"][f].cpu().numpy() - ph)))
        assert np.max(np.abs(d[strong])) <= 1e-3
        rg = out["ranges"][f].cpu().numpy()
        for s_, name in enumerate(("magnitude", "phase", "re", "im")):
            v = out[name][f].cpu().numpy()
            assert rg[s_, 0] == v.min() and rg[s_, 1] == v.max()
    if N == 1024:  # dB / degrees / unwrap take the same kernel
        o2 = G.FFT(N, "Hann", outputInDb=True, outputInDeg=True, unwrapPhase=True, dtype=torch.float32).process_bulk(dev(x))
        mag, ph, _, _ = O.fft_block_truth(x[:N], 3, in_db=True, in_deg=True, unwrap=True)
        finite = mag > -300
        assert np.max(np.abs(o2["magnitude"][0].cpu().numpy()[finite] - mag[finite])) < 1e-2
        d = o2["phase"][0].cpu().numpy() - ph
        assert np.mean(np.abs(d - 360.0 * np.round(d / 360.0)) < 0.05) > 0.9


@pytest.mark.parametrize("N", [256, 1024, 2048, 8192])
def test_fft_many_frames_match_small_batches(G, N):
    """persistent workgroups / several frames per workgroup: a long call equals the same frames processed a few at a time, bit for bit"""
    frames = 3 * 512 * 16 // N + 5
    rng = np.random.default_rng(N)
    x = dev((rng.standard_normal(frames * N) + 1j * rng.standard_normal(frames * N)).astype(np.complex64))
    F = G.FFT(N, "Hann")
    whole = F.spectrum(x)
    for f0 in (0, 7, frames - 3):
        part = F.spectrum(x[f0 * N:(f0 + 3) * N])
        assert torch.equal(part, whole[f0:f0 + 3])
    assert torch.equal(F.mag2(x), whole.real ** 2 + whole.imag ** 2) or float((F.mag2(x) - (whole.real ** 2 + whole.imag ** 2)).abs().max()) <= 1e-6 * float(F.mag2(x).max())


def test_fft_linearity_and_roundtrip_properties(G):
    N, frames = 8192, 64
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(frames * N) + 1j * rng.standard_normal(frames * N)).astype(np.complex64)
    y = (rng.standard_normal(frames * N) + 1j * rng.standard_normal(frames * N)).astype(np.complex64)
    F = G.FFT(N, "None")
    fx, fy, fs = F.spectrum(dev(x)), F.spectrum(dev(y)), F.spectrum(dev(x + y))
    assert float((fs - (fx + fy)).abs().max()) < 1e-4 * N  # qa_SimdFFT.cpp:399-424
    back = torch.conj(F.spectrum(torch.conj(fx).reshape(-1))) / N  # inverse through conjugation
    assert float((back.reshape(-1) - dev(x)).abs().max()) <= 1e-5 * N  # qa_SimdFFT.cpp:122-185
    # Parseval: sum |X|^2 == N * sum |x|^2
    e_t = float((dev(x).abs() ** 2).sum())
    e_f = float(F.mag2(dev(x)).sum())
    assert abs(e_f / (N * e_t) - 1) < 1e-5


# ------------------------------------------------------------------ headline chain
def test_chain_max_workgroups_is_only_a_schedule(G):
    """capping the persistent grid (CUs left to an RCCL fan-in on another stream) changes which CU takes which frame, nothing else"""
    N, frames = 8192, 40
    b = O.design_taps_hamming_lowpass(256, 0.1)
    x = dev(O.signal_c32(9, frames * N))
    for window in ("None", "Hann"):
        ref = G.Chain(b, N, window).process_bulk(x)
        for cap in (1, 7, 224):
            ch = G.Chain(b, N, window)
            ch.set_max_workgroups(cap)
            assert torch.equal(ch.process_bulk(x), ref)


def test_chain_fused_input_alignment(G):
    """the fused kernels stage frames with 16-byte LDS-DMA pieces: an 8-byte-aligned span must give the same spectra"""
    N, frames = 8192, 5
    b = O.design_taps_hamming_lowpass(256, 0.1)
    x = O.signal_c32(3, frames * N)
    buf = torch.empty(frames * N + 1, dtype=torch.complex64, device="cuda")
    buf[1:].copy_(torch.from_numpy(x))
    for window in ("None", "Hann"):
        ref = G.Chain(b, N, window, 0).process_bulk(dev(x))
        got = G.Chain(b, N, window, 0).process_bulk(buf[1:])
        assert torch.equal(ref, got)


@pytest.mark.parametrize("algo", [1, 0, 3, 2])
@pytest.mark.parametrize("N,ntaps,window", [(8192, 256, "None"), (8192, 256, "Hann"), (8192, 91, "Rectangular"), (8192, 1, "None"),
                                            (8192, 200, "BlackmanHarris"), (8192, 256, "Kaiser"), (8192, 17, "FlatTop"),
                                            (1024, 64, "None"), (256, 33, "Hann"), (1024, 64, "Hann"), (512, 256, "BlackmanHarris"),
                                            (2048, 100, "Kaiser"), (4096, 256, "None"), (4096, 31, "Hamming")])
def test_chain_parity(G, algo, N, ntaps, window):
    frames = 6 if N >= 4096 else 3 * (8192 // N) + 5  # small fftSize: whole 8192-sample blocks plus a ragged tail in every call
    b = O.design_taps_hamming_lowpass(ntaps, 0.1) if ntaps > 1 else np.array([0.5], np.float32)
    x = O.signal_c32(42, frames * N)
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    truth, _ = O.chain(b, x, N, wid, truth=True)
    if algo == G.capi.CHAIN_FUSED_TD and N > 4096:
        with pytest.raises(G.capi.Gr4HipError):  # the fused time-domain kernel covers fftSize 256 .. 4096
            G.Chain(b, N, window, algo)
        return
    ch = G.Chain(b, N, window, algo)
    if algo == 0:  # the headline configuration and the FFT block's default sizes must take a fused kernel: the time-domain one up to 64 taps
        assert ch.algo == (G.capi.CHAIN_FUSED_TD if ntaps <= 64 and N <= 4096 else G.capi.CHAIN_FUSED_FD)
    half = (frames // 2) * N
    got = np.concatenate([ch.process_bulk(dev(x[:half])).cpu().numpy().ravel(), ch.process_bulk(dev(x[half:])).cpu().numpy().ravel()])
    assert _rel(got, truth) <= TOL
    # noise-only stream (no dominant tone bin in the rms)
    xn = O.signal_c32(43, 2 * N, tone_amp=0.0)
    tn, _ = O.chain(b, xn, N, wid, truth=True)
    ch.reset()
    assert _rel(ch.process_bulk(dev(xn)).cpu().numpy().ravel(), tn) <= TOL
    cpu32, _ = O.chain(b, xn, N, wid, truth=False)
    ch.reset()
    assert _rel(ch.process_bulk(dev(xn)).cpu().numpy().ravel(), tn) <= _rel(cpu32, tn) + 2e-6  # as accurate as the float32 CPU port, to 1/5 of TOL


@pytest.mark.parametrize("window", ["None", "Hann"])
@pytest.mark.parametrize("N,ntaps", [(256, 64), (512, 17), (1024, 64), (1024, 200), (2048, 128), (4096, 64), (4096, 256), (1024, 1)])
def test_chain_fused_time_domain_many_segments(G, N, ntaps, window):
    """GR4HIP_CHAIN_FUSED_TD at a device-generated stream of many 4096-sample segments (every workgroup takes several, registers prefetch the next
    one), in ragged calls whose frame counts are not whole segments: sampled frames against the float64 oracle, and the whole output against the
    FIR kernel + FFT kernel pair"""
    frames = (1 << 22) // N + 3
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    b = O.design_taps_hamming_lowpass(ntaps, 0.1) if ntaps > 1 else np.array([0.5], np.float32)
    x = G.synth_c32(frames * N, seed=23)
    ch = G.Chain(b, N, window, G.capi.CHAIN_FUSED_TD)
    assert ch.algo == G.capi.CHAIN_FUSED_TD
    cuts = [0, 1, 1 + (4096 // N) * 5 + 1, frames // 2, frames]
    got = torch.cat([ch.process_bulk(x[a * N: c * N]) for a, c in zip(cuts[:-1], cuts[1:])])
    ref = G.Chain(b, N, window, G.capi.CHAIN_TIME_DOMAIN).process_bulk(x)
    assert float((got - ref).abs().max()) <= 3e-6 * float(ref.abs().max())
    fps = max(4096 // N, 1)
    for f in sorted({0, 1, 2, fps - 1, fps, 4 * fps, 4 * fps + 1, cuts[2] - 1, cuts[2], cuts[3] - 1, cuts[3], frames - 1}):
        lo = max(f - (256 + N - 1) // N, 0)
        truth, _ = O.chain(b, x[lo * N:(f + 1) * N].cpu().numpy(), N, wid, truth=True)
        assert _rel(got[f].cpu().numpy(), truth.reshape(-1, N)[f - lo]) <= TOL, (f,)


@pytest.mark.parametrize("N,ntaps,window", [(1000, 33, "Hann"), (8192, 300, "None"), (16384, 64, "Hann"), (4096, 1024, "BlackmanHarris"), (128, 16, "None")])
def test_chain_shapes_outside_the_fused_kernel(G, N, ntaps, window):
    """AUTO falls back to the FIR kernel + FFT kernel pair for what the fused kernel does not cover (more than 256 taps, sizes that are not a power
    of two in 256 ... 8192): same contract, same parity bar; asking for the fused kernel explicitly is refused with UNSUPPORTED"""
    frames = 4
    b = O.design_taps_hamming_lowpass(ntaps, 0.1)
    x = O.signal_c32(7, frames * N)
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    truth, _ = O.chain(b, x, N, wid, truth=True)
    ch = G.Chain(b, N, window, 0)
    assert ch.algo == G.capi.CHAIN_UNFUSED
    got = np.concatenate([ch.process_bulk(dev(x[:N])).cpu().numpy().ravel(), ch.process_bulk(dev(x[N:])).cpu().numpy().ravel()])
    assert _rel(got, truth) <= TOL
    with pytest.raises(G.capi.Gr4HipError) as e:
        G.Chain(b, N, window, G.capi.CHAIN_FUSED_FD)
    assert e.value.status == G.capi.UNSUPPORTED


def test_chain_dynamic_range_and_the_time_domain_algo(G):
    """a tone 30 dB above the noise, removed by a narrow low-pass: the fast-convolution kernels carry the float32 rounding of their transforms, which scales
    with the INPUT (error floor ~2e-6 of the input rms per output sample); relative to the much smaller OUTPUT that exceeds 1e-5.  CHAIN_AUTO measures the
    power ratio and hands such a stream to the direct-form kernels (the reference's arithmetic) before anything is published; an explicit CHAIN_FUSED_FD does not"""
    N, frames, ntaps = 8192, 80, 64
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    x = O.signal_c32(77, frames * N, tone_frel=0.31, tone_amp=30.0)
    check = slice(70 * N, 72 * N)  # two frames deep inside the span (the oracle's float64 chain over the whole span is the truth)
    truth, _ = O.chain(b, x, N, 3, truth=True)
    in_rms = float(np.sqrt(np.mean(np.abs(x) ** 2)))
    errs = {}
    for algo in (G.capi.CHAIN_AUTO, G.capi.CHAIN_FUSED_FD, G.capi.CHAIN_TIME_DOMAIN):
        ch = G.Chain(b, N, "Hann", algo)
        got = ch.process_bulk(dev(x)).cpu().numpy().ravel()
        errs[algo] = _rel(got[check], truth[check])
        if algo == G.capi.CHAIN_AUTO:
            assert _rel(got, truth) <= TOL  # every frame, the probed first ones included
            ratio, td = ch.last_power_ratio()
            assert not td and 0 <= ratio < 0.08, (ratio, td)  # (the call's marked frames were evaluated again on the device, behind the fused launch: nobody waited, nothing switched yet)
            # ... the next call finds that measurement and moves the stream to the time-domain kernels (history handed over), where it stays until reset
            x2 = O.signal_c32(78, 4 * N, tone_frel=0.31, tone_amp=30.0)
            t2, _ = O.chain(b, np.concatenate([x, x2]), N, 3, truth=True)
            assert _rel(ch.process_bulk(dev(x2)).cpu().numpy().ravel(), t2[frames * N:]) <= TOL
            assert ch.last_power_ratio()[1]
    assert errs[G.capi.CHAIN_TIME_DOMAIN] <= TOL and errs[G.capi.CHAIN_AUTO] <= TOL
    assert errs[G.capi.CHAIN_FUSED_FD] > TOL > errs[G.capi.CHAIN_TIME_DOMAIN]  # the price of the fused kernel on this input ...
    # ... and its bound: amplitude errors stay below 4e-6 of the input rms: |d mag2| <= 2 |Y| dY + dY^2 with dY = 4e-6 in_rms sqrt(N sum w^2)
    y, _ = O.fir(b, x)
    fir_auto = G.fir_filter(b, torch.complex64)
    fir_td = G.fir_filter(b, torch.complex64)
    fir_td.set_algo(G.capi.FIR_TIME_DOMAIN)
    ya, yt = fir_auto.process_bulk(dev(x)).cpu().numpy(), fir_td.process_bulk(dev(x)).cpu().numpy()
    assert _rel(yt, y) <= TOL                          # direct form: inside the bar relative to the output
    assert _rel(ya, y) <= TOL                          # FIR_AUTO: the same guard (first fast convolution probed, this input sent to the direct form)
    # pass-band input keeps the fast convolution (its floor is relative to the input: 4e-6 of the input rms), also across calls
    xp = O.signal_c32(79, 80 * N, tone_frel=0.005, tone_amp=1.0)
    yp, _ = O.fir(b, xp)
    fa = G.fir_filter(b, torch.complex64)
    got = np.concatenate([fa.process_bulk(dev(xp[: 70 * N])).cpu().numpy(), fa.process_bulk(dev(xp[70 * N:])).cpu().numpy()])
    assert np.max(np.abs(got - yp)) <= 4e-6 * float(np.sqrt(np.mean(np.abs(xp) ** 2))) and _rel(got, yp) <= TOL


def test_chain_every_frame_marked_meets_the_bar(G):
    """GR4HIP_GUARD_STRICT: a stream whose every frame is marked still meets the bar -- the second evaluation (chain_redo_kernel) rides the same stream behind the fused
    launch.  (The timing half -- the call returns while its launch runs, two guarded chains overlap -- is tests/test_zz_gpu_stress.py::test_chain_strict_guard_does_not_wait_for_its_launch.)"""
    N, ntaps = 8192, 256
    # every frame marked: the result is the time-domain evaluation's
    n2 = 64 * N
    loud = O.signal_c32(6, n2, tone_frel=0.31, tone_amp=300.0)
    bl = O.design_taps_hamming_lowpass(ntaps, 0.02)
    truth, _ = O.chain(bl, loud, N, 0, truth=True)
    for window, wid in (("None", 0), ("Hann", 3)):
        tw, _ = O.chain(bl, loud, N, wid, truth=True)
        cg = G.Chain(bl, N, window)
        assert cg.algo == G.capi.CHAIN_FUSED_FD
        assert _rel(cg.process_bulk(dev(loud)).cpu().numpy().ravel(), tw) <= TOL, window


@pytest.mark.parametrize("window,wid", [("None", 0), ("Hann", 3)])
def test_chain_guard_judges_frames_on_what_the_error_depends_on(G, window, wid):
    """round 6: the guard's two statistics (include/gr4hip.h, chain_fused.hip kGuardR4Max / kGuardPeakMax).  (1) A 1 %-pass-band channel filter over wide-band noise ALONE
    (output / input power 0.008: every frame marked until round 6) has R4 = 6 .. 13 of 20 (a frame in forty goes over under the Hann window): not marked, the fused launch alone meets the bar.  (2) The same noise beside
    a wide-band neighbour 20 dB stronger outside the pass band: R4 ~ 50, every frame marked, evaluated again behind the launch.  (3) A line the filter only dents -- a 2-tap
    average over noise + a tone near fs / 2, 20 dB down at the output but still its strongest component (the wide fuzzer's case: the transform's image of the line lands in the
    pass band; output / input power 0.15, R4 = 1.9, never marked by either earlier test): marked by the line statistic."""
    N, frames = 8192, 40
    n = frames * N
    rng = np.random.default_rng(77)
    noise = O.signal_c32(31, n, tone_amp=0.0)
    b = O.design_taps_hamming_lowpass(256, 0.005)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    V = np.fft.fft(v); V[np.abs(np.fft.fftfreq(n) - 0.3) > 0.05] = 0
    v = np.fft.ifft(V); v *= 10.0 * np.sqrt(np.mean(np.abs(noise) ** 2) / np.mean(np.abs(v) ** 2))
    k = np.arange(n)
    cases = ((b, noise, 0.0, 0.1), (b, (noise + v).astype(np.complex64), 1.0, 1.0),
             (np.array([0.5, 0.5], np.float32), (noise + 1.7 * np.sqrt(np.mean(np.abs(noise) ** 2)) * np.exp(2j * np.pi * 0.5326 * k)).astype(np.complex64), 1.0, 1.0))
    for taps, x, lo, hi in cases:
        truth, _ = O.chain(taps, x, N, wid, truth=True)
        ch = G.Chain(taps, N, window)
        assert ch.algo == G.capi.CHAIN_FUSED_FD
        got = ch.process_bulk(dev(x)).cpu().numpy().ravel()
        marked, f64 = ch.last_guard_fractions()
        assert lo <= marked <= hi, (len(taps), marked)
        assert _rel(got, truth) <= TOL, (len(taps), marked, f64)


def test_chain_kernel_pair_under_a_removed_tone(G):
    """fft sizes beyond 8192 (CHAIN_AUTO -> the kernel pair: FIR kernel -> HBM -> FFT kernel): a tone 15 dB above the noise that a 65-tap filter removes by ~60 dB leaves a
    residue at the level of the output spectrum's rms.  The two-term f16 direct form's 22-bit products err coherently on the tone and the transform gathers that into the
    residue's bin: 1.0 .. 4.2e-5 in ~1 % of such streams until round 6's last day (tools/dbg/pair_coherent.py), where the reference's float32 sum is at 6e-7.  The pair's
    filter runs on float32 products since: inside the bar, or inside the reference's own float32 error -- factor ONE"""
    N, frames = 16384, 6
    n = frames * N
    b = O.design_taps_hamming_lowpass(65, 0.05)
    rng = np.random.default_rng(12)
    H = np.abs(np.fft.fft(b.astype(np.float64), 65536))
    worst = 0.0
    for trial in range(24):
        f0 = float(rng.uniform(0.11, 0.18)); amp = float(rng.uniform(5.0, 7.0))
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n) + amp * np.exp(2j * np.pi * (f0 * np.arange(n) + rng.random()))).astype(np.complex64)
        truth, _ = O.chain(b, x, N, 0, truth=True)
        ch = G.Chain(b, N, "None")
        assert ch.algo == G.capi.CHAIN_UNFUSED
        got = ch.process_bulk(dev(x)).cpu().numpy().ravel()
        y32 = O.fir(b, x, acc64=False)[0].reshape(frames, N)
        t32 = (np.abs(np.fft.fft(y32.astype(np.complex128), axis=1)) ** 2).ravel()
        e, e32 = _rel(got, truth), _rel(t32, truth)
        assert e <= max(TOL, e32), (trial, f0, amp, e, e32)
        worst = max(worst, e)
    assert worst <= 5e-6, worst  # (measured 1.4e-6; the f16 form reached 4e-5)


@pytest.mark.parametrize("level", [1e-17, 1e-12, 1e9, 1e12])
def test_chain_guard_at_extreme_stream_levels(G, level):
    """the guard's statistic sums fourth powers: beyond samples of ~3e7 (or below ~1e-12 .. 1e-17) sum |Y_k|^4 leaves float32's range and nothing can be judged -- such frames are
    marked wholesale and evaluated again behind the launch (a sum of 0 or Inf marks): the bar holds at every level float32 can carry the spectrum at"""
    N, frames = 8192, 12
    b = O.design_taps_hamming_lowpass(256, 0.02)
    x = (O.signal_c32(14, frames * N, tone_frel=0.31, tone_amp=3.0).astype(np.complex128) * level).astype(np.complex64)
    for window, wid in (("None", 0), ("Hann", 3)):
        truth, _ = O.chain(b, x, N, wid, truth=True)
        ch = G.Chain(b, N, window)
        got = ch.process_bulk(dev(x)).cpu().numpy().ravel()
        marked, f64 = ch.last_guard_fractions()
        assert _rel(got, truth) <= TOL, (window, marked, f64)
        if level >= 1e9 or level <= 1e-17:
            assert marked == 1.0


@pytest.mark.parametrize("N,ntaps,window,wid,fc,amp,f0", [(8192, 256, "None", 0, 0.005, 1.0, 0.1), (8192, 256, "Hann", 3, 0.005, 1.0, 0.1), (8192, 129, "Kaiser", 11, 0.01, 0.0, 0.1),
                                                       (1024, 200, "Hamming", 2, 0.005, 1.0, 0.1), (256, 100, "BlackmanHarris", 7, 0.004, 3.0, 0.2), (4096, 256, "None", 0, 0.008, 0.5, 0.3),
                                                       (8192, 256, "None", 0, 0.02, 300.0, 0.31), (8192, 256, "Hann", 3, 0.02, 30.0, 0.31), (2048, 77, "Hann", 3, 0.02, 1000.0, 0.4)])
def test_chain_marked_frames_on_the_f16_pipe_then_float64(G, N, ntaps, window, wid, fc, amp, f0):
    """round 6: the frames a fused launch marks (fourth-moment statistic and line statistic, R4 / 20 + T' / 2000 > 1: the fast convolution's error, sized by the INPUT, would
    show) are evaluated again by chain_td16_kernel at 8192 points -- filter on the f16 matrix pipe (22-bit products under one block exponent per frame), window, one transform
    from LDS, stored where it agrees with the fused result in every bin -- and what that leaves (the loud rejected tones of the last three cases; every marked frame at
    fftSize < 8192) by chain_redo_kernel's float64 products behind it.  A stream in which more than a tenth of the frames end in float64 moves to the time-domain kernel pair.
    A narrow channel filter removing a tone at the noise's level (every frame marked, none in float64: the stream stays), all windows' code paths (8192 rectangular / windowed, fftSize < 8192),
    ragged calls, the call after the stream has moved: all against the float64 oracle at the contract's bar"""
    b = O.design_taps_hamming_lowpass(ntaps, fc)
    n = 21 * 8192
    x = O.signal_c32(5, n, tone_frel=f0, tone_amp=amp)
    truth, _ = O.chain(b, x, N, wid, truth=True)
    ch = G.Chain(b, N, window)
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    d = dev(x)
    cuts = [0, 8192 * 5, 8192 * 5 + N * (8192 // N // 2 + 1), 8192 * 13, n]  # (a cut inside an 8192-sample block when fftSize < 8192: the staged tail)
    got = np.concatenate([ch.process_bulk(d[lo:hi]).cpu().numpy().ravel() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert _rel(got, truth) <= TOL
    ratio, moved = ch.last_power_ratio()
    marked, f64 = ch.last_guard_fractions()
    assert 0 <= ratio < 0.08 and 0 <= f64 <= 1
    if amp >= 30:
        assert moved and f64 > 0.1  # (the later calls ran in the time domain; the first one in-stream)
    if N == 8192 and fc == 0.005:
        assert not moved and marked == 1.0 and f64 <= 0.1, (marked, f64)  # every frame marked, the 22-bit tier absorbed them: fused launch + second evaluation IS this stream's way
    ch.reset()
    assert _rel(ch.process_bulk(d).cpu().numpy().ravel(), truth) <= TOL  # the whole span in-stream: fused launch + the second evaluations, one call


@pytest.mark.parametrize("N,ntaps,window,wid", [(4096, 64, "None", 0), (2048, 64, "Hann", 3), (256, 33, "BlackmanHarris", 7), (1024, 17, "Hamming", 2)])
def test_fused_time_domain_chain_answers_to_the_guard(G, N, ntaps, window, wid):
    """CHAIN_AUTO with <= 64 taps at fft sizes <= 4096 runs the fused time-domain kernel (chain_td.hip: the filter as float32 sums in the matrix pipe's order).  tools/fuzz_chain.py
    against the oracle's reference-order float32 FIR found it at up to 4.6 x that sum's error under a rejected interferer; since round 5 the kernel marks the 4096-sample
    segments whose filter output carries less than (sum b^2 / 128) x their input power and chain_redo_kernel evaluates the blocks that hold one again with float64 products
    behind the launch: within the float64 bar, or within the reference's own float32 error -- factor ONE.  An interferer that sets in mid-stream, ragged calls, a span that
    is not a whole number of 8192-sample blocks"""
    rng = np.random.default_rng(N + ntaps)
    frames = (3 * 8192 + 4096) // N * 4 + 1 if N < 4096 else 13
    n = frames * N
    b = O.design_taps_hamming_lowpass(ntaps, 0.05)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    start = n // 3 + 17
    x[start:] += (300.0 * np.exp(2j * np.pi * 0.41 * np.arange(n - start))).astype(np.complex64)
    truth, _ = O.chain(b, x, N, wid, truth=True)
    y32 = O.fir(b, x, acc64=False)[0].reshape(frames, N)
    w = O.window(wid, N).astype(np.float64) if wid else 1.0
    t32 = (np.abs(np.fft.fft(y32.astype(np.complex128) * w, axis=1)) ** 2).ravel()
    ch = G.Chain(b, N, window)
    assert ch.algo == G.capi.CHAIN_FUSED_TD
    cuts = [0, frames // 4, frames // 4 + 1, frames]
    got = np.concatenate([ch.process_bulk(dev(x[a * N:c * N])).cpu().numpy().ravel() for a, c in zip(cuts[:-1], cuts[1:])])

    def rel_frames(a, t):  # the chain's metric: per frame
        a, t = a.reshape(frames, N), t.reshape(frames, N)
        rms = np.sqrt(np.mean(t ** 2, axis=1, keepdims=True))
        return float(np.max(np.abs(a - t) / np.maximum(t, rms)))
    e, e_ref = rel_frames(got, truth), rel_frames(t32, truth)
    assert e <= max(TOL, e_ref), (e, e_ref)
    off = G.Chain(b, N, window)
    off.set_guard_mode(G.capi.GUARD_OFF)
    assert rel_frames(off.process_bulk(dev(x)).cpu().numpy().ravel(), truth) > e  # (what the second evaluation is for)


def test_chain_guard_hands_small_fft_sizes_to_the_fused_time_domain_kernel(G):
    """fftSize <= 4096 with more than 64 taps: CHAIN_AUTO starts on the fused fast convolution; a stream whose filter removes most of the input is handed
    (history included) to the fused time-domain kernel -- one launch, the reference's arithmetic -- and meets the bar relative to the OUTPUT"""
    N, frames, ntaps = 1024, 700, 200
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    x = O.signal_c32(81, frames * N, tone_frel=0.31, tone_amp=30.0)
    truth, _ = O.chain(b, x, N, 3, truth=True)
    ch = G.Chain(b, N, "Hann")
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    cut = 650 * N
    got = np.concatenate([ch.process_bulk(dev(x[:cut])).cpu().numpy().ravel(), ch.process_bulk(dev(x[cut:])).cpu().numpy().ravel()])
    ratio, td = ch.last_power_ratio()
    assert td and 0 <= ratio < 0.08, (ratio, td)
    assert _rel(got, truth) <= TOL
    fd = G.Chain(b, N, "Hann", G.capi.CHAIN_FUSED_FD).process_bulk(dev(x)).cpu().numpy().ravel()
    assert _rel(fd, truth) > TOL  # what the guard is for


def test_chain_guard_switches_mid_stream_and_not_on_ordinary_input(G):
    """the guard of CHAIN_AUTO: pass-band input never leaves the fused kernel; an interferer that appears in a LATER call is found by that call's own
    measurement.  GUARD_STRICT (default): the frames the fused kernel marks are evaluated again in the time domain by a launch enqueued behind it -- EVERY call meets the bar, no call waits.  GUARD_DEFERRED: the call
    that measures the drop is published from the fused kernel (its floor: ~2e-6 of the input rms, as include/gr4hip.h says) and the next call has switched."""
    N, ntaps = 8192, 64
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    clean = O.signal_c32(5, 40 * N, tone_frel=0.01, tone_amp=1.0)        # tone in the pass band
    loud = O.signal_c32(6, 40 * N, tone_frel=0.31, tone_amp=30.0)        # interferer far outside
    truth, _ = O.chain(b, np.concatenate([clean, loud, loud]), N, 0, truth=True)
    t = truth.reshape(3, -1)
    ch = G.Chain(b, N, "None")
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    parts = [ch.process_bulk(dev(clean)).cpu().numpy().ravel()]
    r, td = ch.last_power_ratio()
    assert not td and r > 0.08
    parts.append(ch.process_bulk(dev(loud)).cpu().numpy().ravel())     # every frame measured below the threshold -> evaluated again in the time domain behind the fused launch (chain_redo_kernel)
    r, td = ch.last_power_ratio()
    assert 0 <= r < 0.08 and not td                                    # (the stream moves with the NEXT call, which finds this measurement without waiting for it)
    parts.append(ch.process_bulk(dev(loud)).cpu().numpy().ravel())
    assert ch.last_power_ratio()[1]
    assert _rel(parts[0], t[0]) <= TOL and _rel(parts[1], t[1]) <= TOL and _rel(parts[2], t[2]) <= TOL
    # the interferer may also arrive in the middle of a call: the whole span is redone
    ch.reset()
    mixed = np.concatenate([clean[: 20 * N], loud[: 20 * N]])
    tm, _ = O.chain(b, mixed, N, 0, truth=True)
    assert _rel(ch.process_bulk(dev(mixed)).cpu().numpy().ravel(), tm) <= TOL and not ch.last_power_ratio()[1]  # (frame by frame: only the marked ones)
    # GUARD_DEFERRED: asynchronous calls, the switch lags by one call
    cd = G.Chain(b, N, "None")
    cd.set_guard_mode(G.capi.GUARD_DEFERRED)
    pd = [cd.process_bulk(dev(clean)).cpu().numpy().ravel()]
    pd.append(cd.process_bulk(dev(loud)).cpu().numpy().ravel())        # still fused: this call is the one that measures the drop
    r, td = cd.last_power_ratio()
    assert 0 <= r < 0.08 and not td
    pd.append(cd.process_bulk(dev(loud)).cpu().numpy().ravel())        # switched before this call, history carried over
    assert cd.last_power_ratio()[1]
    assert _rel(pd[0], t[0]) <= TOL and _rel(pd[2], t[2]) <= TOL
    in_rms = float(np.sqrt(np.mean(np.abs(loud.astype(np.complex128)) ** 2)))
    amp_err = np.abs(np.sqrt(np.maximum(pd[1], 0)) - np.sqrt(t[1])) / (in_rms * np.sqrt(N))  # spectra carry a factor sqrt(N) of the time-domain rms
    assert float(np.max(amp_err)) <= 2e-5, float(np.max(amp_err))      # the documented floor of the one deferred call (a few 1e-6 of the input rms)
    # GUARD_OFF never measures nor switches
    co = G.Chain(b, N, "None")
    co.set_guard_mode(G.capi.GUARD_OFF)
    co.process_bulk(dev(loud)); co.process_bulk(dev(loud))
    assert co.last_power_ratio() == (-1.0, False)
    ch.reset()
    assert _rel(ch.process_bulk(dev(clean)).cpu().numpy().ravel(), t[0]) <= TOL and not ch.last_power_ratio()[1]  # a reset re-arms the fused kernel
    # the measured ratio is the filter's power gain whatever the fftSize and window: white noise through a DC-gain-1 low-pass passes sum b^2 of its power
    noise = O.signal_c32(8, 64 * N, tone_amp=0.0)
    b100 = O.design_taps_hamming_lowpass(100, 0.02)  # (up to 64 taps the small sizes take the fused time-domain kernel: nothing to guard)
    for fft_size, window, taps in ((8192, "None", b), (8192, "Hann", b), (1024, "Hann", b100), (256, "None", b100)):
        want = float(np.sum(taps.astype(np.float64) ** 2))
        c2 = G.Chain(taps, fft_size, window)
        assert c2.algo == G.capi.CHAIN_FUSED_FD
        c2.process_bulk(dev(noise))
        r, _ = c2.last_power_ratio()
        assert 0.7 * want < r < 1.4 * want, (fft_size, window, r, want)
    c3 = G.Chain(b, 1024, "Hann")
    assert c3.algo == G.capi.CHAIN_FUSED_TD and c3.last_power_ratio() == (-1.0, False)


def test_fir_decimate_by_8_dynamic_range_guard(G, devsw):
    """the frequency-domain decimator (FIR_AUTO, decimate 8, long spans) carries the float32 rounding of its transforms, ~2e-6 of the INPUT rms; an anti-alias
    low-pass in front of a +40 dB out-of-band blocker removes almost all of the input, so that floor is far above 1e-5 of the OUTPUT.  The guard measures
    every such launch and (strict, the default) redoes the span on the polyphase kernels before the call returns; ordinary input stays on the fast kernel."""
    ntaps, D = 1024, 8
    b = O.design_taps_hamming_lowpass(ntaps, 0.05)            # pass band well inside fs / 16
    n = 96 * 7168
    quiet = O.signal_f32(41, n, tone_frel=0.01, tone_amp=1.0, noise_amp=0.05)
    k = np.arange(n)
    blocker = (100.0 * np.cos(2 * np.pi * 0.31 * k)).astype(np.float32)      # +40 dB, far outside
    for name, x, expect_switch in (("ordinary", quiet, False), ("blocker", quiet + blocker, True)):
        truth, _ = O.fir_decim(b, x, D)
        f = G.fir_filter(b, torch.float32, decimate=D)
        y = f.process_bulk(dev(x)).cpu().numpy()
        assert _rel(y, truth) <= TOL, name
        # (late round 4: the default above is the f16 band-form kernel of fir_decim_f16.hip, whose error is relative to the output and which judges its own segments;
        # the frequency-domain kernel and its host-side guard stay behind GR4HIP_FIR_NO_DECIM_F16 -- and are what the rest of this test is about)
        devsw("GR4HIP_FIR_NO_DECIM_F16", 1)
        f1 = G.fir_filter(b, torch.float32, decimate=D)
        assert _rel(f1.process_bulk(dev(x)).cpu().numpy(), truth) <= TOL, name
        # what the guard is for: the same span forced through the frequency-domain kernel
        f2 = G.fir_filter(b, torch.float32, decimate=D)
        G.capi.check(G.capi.lib().gr4hip_fir_set_guard_mode(f2._h, G.capi.GUARD_OFF), "guard off")
        e_fd = _rel(f2.process_bulk(dev(x)).cpu().numpy(), truth)
        devsw("GR4HIP_FIR_NO_DECIM_F16", 0)
        assert (e_fd > TOL) == expect_switch, (name, e_fd)


def test_complex_fast_convolution_guard_without_the_host(G):
    """fir_filter<complex<float>>, 97 .. 256 taps, on a long span that is only 8-byte aligned: the fast-convolution kernel (chain_fd_kernel<kModeFir>) -- whose error floor is
    relative to the INPUT.  Round 5: its strict guard judges every 8192-sample frame behind the launch (fir_judge_kernel at the 0.04 threshold) and fir_exact_kernel
    evaluates the marked frames again; the call does not wait, a blocker in a few frames of a long call is seen, ordinary input keeps the fast convolution's result"""
    ntaps = 200
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    n = 100 * 8192
    base = torch.empty(n + 3, dtype=torch.complex64, device="cuda")

    def run(x, guard=None):
        t = base[3:]  # 24 bytes past a 256-byte boundary: 8-byte aligned only
        assert t.data_ptr() % 16 == 8
        t.copy_(torch.from_numpy(x))
        f = G.fir_filter(b, torch.complex64)
        if guard is not None:
            f.set_guard_mode(guard)
        return f.process_bulk(t).cpu().numpy()
    quiet = O.signal_c32(5, n, tone_frel=0.005, tone_amp=1.0)
    loud = quiet.copy()
    loud[60 * 8192:63 * 8192] += (300.0 * np.exp(2j * np.pi * 0.31 * np.arange(3 * 8192))).astype(np.complex64)
    for x, tripped in ((quiet, False), (loud, True)):
        truth = O.fir(b, x)[0]
        assert _rel(run(x), truth) <= TOL
        assert (_rel(run(x, G.capi.GUARD_OFF), truth) > TOL) == tripped  # (what the guard is for)


def test_guard_sees_every_frame_and_block(G, devsw):
    """an interferer that sets in near the END of a long call -- where one workgroup has long left its first frame behind -- or only for a few frames is seen:
    the kernels judge every frame / block by itself (workgroup-wide sums of output - threshold x input power), not a sample of them, and not the launch's totals,
    which such a short event barely moves.  Strict guard: the marked frames are evaluated again behind the launch (chain_redo_kernel), every output inside the bar."""
    N, ntaps = 8192, 100
    b = O.design_taps_hamming_lowpass(ntaps, 0.05)
    frames = 700                                                  # 256 workgroups: frames 512 .. 699 are every workgroup's third iteration
    x = O.signal_c32(9, frames * N, tone_frel=0.01, tone_amp=1.0)
    k = np.arange(5 * N)
    for first, count in ((frames - 5, 5), (600, 2)):
        xi = x.copy()
        xi[first * N:(first + count) * N] += (60.0 * np.exp(2j * np.pi * 0.31 * k[: count * N])).astype(np.complex64)
        truth, _ = O.chain(b, xi, N, 0, truth=True)
        ch = G.Chain(b, N, "None")
        assert ch.algo == G.capi.CHAIN_FUSED_FD
        got = ch.process_bulk(dev(xi)).cpu().numpy().ravel()
        r, td = ch.last_power_ratio()
        marked, f64 = ch.last_guard_fractions()
        assert not td and r > 0.03 and count <= round(marked * frames) <= count + 2, (first, count, r, marked)  # the launch-wide ratio is 0.04 .. 0.09, a narrow filter's: the frames are judged one by one (and the marked ones evaluated again behind the launch)
        assert _rel(got, truth) <= TOL, (first, count)
    # the frequency-domain decimator: a blocker in the last 3 of 700 blocks
    D, nt = 8, 1024
    bd = O.design_taps_hamming_lowpass(nt, 0.05)
    n = 700 * 7168
    xq = O.signal_f32(41, n, tone_frel=0.01, tone_amp=1.0, noise_amp=0.05)
    xq[-3 * 7168:] += (100.0 * np.cos(2 * np.pi * 0.31 * np.arange(3 * 7168))).astype(np.float32)
    truth, _ = O.fir_decim(bd, xq, D)
    assert _rel(G.fir_filter(bd, torch.float32, decimate=D).process_bulk(dev(xq)).cpu().numpy(), truth) <= TOL  # (the default: the f16 band-form kernel)
    devsw("GR4HIP_FIR_NO_DECIM_F16", 1)
    assert _rel(G.fir_filter(bd, torch.float32, decimate=D).process_bulk(dev(xq)).cpu().numpy(), truth) <= TOL
    f2 = G.fir_filter(bd, torch.float32, decimate=D)
    G.capi.check(G.capi.lib().gr4hip_fir_set_guard_mode(f2._h, G.capi.GUARD_OFF), "guard off")
    assert _rel(f2.process_bulk(dev(xq)).cpu().numpy(), truth) > TOL  # (what the guard was for)
    devsw("GR4HIP_FIR_NO_DECIM_F16", 0)


def test_chain_kernel_pair_squares_its_filter_output(G):
    """round 5 (tools/fuzz_chain.py 120 41, case 828; tools/dbg_chain_case828.py): a 65-tap / fc 0.02 filter in front of a BlackmanHarris 8192-point transform, a tone ~20 dB
    above the noise far outside the pass band: the frames sit 33 dB below their input -- 19 dB more than white noise loses, 2 dB short of the FIR guard's 21 dB -- so the
    kernel pair's filter (two-term f16 products) left them unmarked at ~5e-6 of the OUTPUT, and |Y|^2 doubles that: 1.015e-5 where the reference's float32 chain is at 6e-7.
    The pair's filter and the fused time-domain kernel now mark 6 dB earlier (chain.hip kChainPairGuardRatio).  Per-frame metric, as the fuzzer's."""
    from scipy.signal import lfilter
    N, ntaps, frames, on = 8192, 65, 20, 4
    k = np.arange(ntaps)
    b = np.hamming(ntaps) * 0.04 * np.sinc(0.04 * (k - (ntaps - 1) / 2))
    b = (b / b.sum()).astype(np.float32)
    rng = np.random.default_rng(828)
    noise = (rng.standard_normal(frames * N) + 1j * rng.standard_normal(frames * N)).astype(np.complex64)
    tone = np.exp(2j * np.pi * 0.41 * np.arange((frames - on) * N))
    w = O.window(7, N, np.float32).astype(np.float64)
    worst = 0.0
    for db in (19.5, 20.0, 20.48, 21.0, 21.5, 22.0):
        x = noise.copy()
        x[on * N:] += (10 ** (db / 20) * tone).astype(np.complex64)
        y = lfilter(b.astype(np.float64), [1.0], x.astype(np.complex128)).reshape(frames, N) * w
        truth = np.abs(np.fft.fft(y, axis=1)) ** 2
        rms = np.sqrt(np.mean(truth ** 2, axis=1, keepdims=True))
        for algo in (G.capi.CHAIN_UNFUSED, G.capi.CHAIN_AUTO):
            ch = G.Chain(b, N, "BlackmanHarris", algo)
            got = np.concatenate([ch.process_bulk(dev(x[:on * N])).cpu().numpy(), ch.process_bulk(dev(x[on * N:])).cpu().numpy()]).reshape(frames, N)
            worst = max(worst, float(np.max(np.abs(got - truth) / np.maximum(truth, rms))))
    # measured: 1.04e-6 (the reference's float32 chain: 6 - 8e-7); with the FIR guard's own 21 dB threshold (developer build -DGR4_T_PAIR_GUARD_128) 8.3e-6 on this data and 1.015e-5 on the
    # fuzzer's -- so the pin is well inside the bar, not at it
    assert worst <= 3e-6, worst


def test_guard_destination_multiplies_in_float32(G):
    """where the guard sends a stream -- a rejected signal far above the output -- is where product precision shows: the three-term bf16 products keep everything
    above 2^-23 of a product (3 .. 16 x the error of a float32 sum there), so the guard's destination and GR4HIP_CHAIN_TIME_DOMAIN run the direct form with
    float32 products on the f32 matrix pipe (GR4HIP_FIR_TIME_DOMAIN_F32): inside the bar with an interferer 50 dB above the noise, where the default direct form
    (and the float32 CPU form) are not"""
    N, ntaps, frames = 8192, 100, 64
    b = O.design_taps_hamming_lowpass(ntaps, 0.05)
    x = O.signal_c32(12, frames * N, tone_frel=0.01, tone_amp=1.0)
    x += (316.0 * np.exp(2j * np.pi * 0.41 * np.arange(frames * N))).astype(np.complex64)
    truth, _ = O.chain(b, x, N, 0, truth=True)
    ch = G.Chain(b, N, "None")                                   # AUTO: the guard trips on the first call and redoes it
    got = ch.process_bulk(dev(x)).cpu().numpy().ravel()
    assert 0 <= ch.last_power_ratio()[0] < 0.08 and _rel(got, truth) <= TOL
    assert _rel(G.Chain(b, N, "None", G.capi.CHAIN_TIME_DOMAIN).process_bulk(dev(x)).cpu().numpy().ravel(), truth) <= TOL
    # the FIR alone: float32 products against the default three-term bf16 ones, both against float64
    yt, _ = O.fir(b, x)                                           # (float64 accumulation)
    # (guard off: the products by themselves.  Under the guard -- since round 5 every kernel answers to it -- both hand these segments to the float64 second evaluation)
    f32 = G.fir_filter(b, torch.complex64); f32.set_algo(G.capi.FIR_TIME_DOMAIN_F32); f32.set_guard_mode(G.capi.GUARD_OFF)
    fbf = G.fir_filter(b, torch.complex64); fbf.set_algo(G.capi.FIR_TIME_DOMAIN_BF16X3); fbf.set_guard_mode(G.capi.GUARD_OFF)
    e32, ebf = _rel(f32.process_bulk(dev(x)).cpu().numpy(), yt), _rel(fbf.process_bulk(dev(x)).cpu().numpy(), yt)
    assert e32 <= TOL and e32 < 0.5 * ebf, (e32, ebf)
    for algo in (G.capi.FIR_TIME_DOMAIN_F32, G.capi.FIR_TIME_DOMAIN_BF16X3):
        fg = G.fir_filter(b, torch.complex64); fg.set_algo(algo)
        assert _rel(fg.process_bulk(dev(x)).cpu().numpy(), yt) <= 1e-6
    # since round 4 the direct form proper (GR4HIP_FIR_TIME_DOMAIN) is the f16 kernel that judges every segment and evaluates the rejected ones again with three-term
    # f16 products (float32 products): as close as the float32 kernel
    fhf = G.fir_filter(b, torch.complex64); fhf.set_algo(G.capi.FIR_TIME_DOMAIN)
    ehf = _rel(fhf.process_bulk(dev(x)).cpu().numpy(), yt)
    assert ehf <= TOL and ehf <= 1.5 * e32 + 1e-7, (ehf, e32)


def test_auto_chain_without_a_guard_multiplies_better_than_float32(G):
    """AUTO chains of <= 64 taps at fft sizes <= 4096 take the fused time-domain kernel, which has no dynamic-range guard to fall back on: its products are
    therefore eight-term bf16 splits (exact to ~2^-31, below a float32 product's 2^-25).  Pinned where it shows: an interferer 50 dB above the output that the
    filter rejects -- |Y|^2 must be as close to float64 as the reference's float32 arithmetic gets there (profiles/r03_fuzz_summary.txt: the six-term form
    measured 3 x the float32 CPU form, 6.7e-5)"""
    for N, ntaps in ((1024, 64), (4096, 48), (256, 33)):
        frames = 8 * 8192 // N
        b = O.design_taps_hamming_lowpass(ntaps, 0.05)
        x = O.signal_c32(31, frames * N, tone_frel=0.01, tone_amp=1.0)
        x += (316.0 * np.exp(2j * np.pi * 0.41 * np.arange(frames * N))).astype(np.complex64)
        truth, _ = O.chain(b, x, N, 0, truth=True)
        cpu32, _ = O.chain(b, x, N, 0, truth=False)  # the reference-faithful float32 path
        ch = G.Chain(b, N, "None")
        assert ch.algo == G.capi.CHAIN_FUSED_TD
        got = ch.process_bulk(dev(x)).cpu().numpy().ravel()
        e_dev, e_cpu = _rel(got, truth), _rel(cpu32.ravel(), truth)
        assert e_dev <= max(1.5 * e_cpu, TOL), (N, ntaps, e_dev, e_cpu)


def _aligned16(x):
    """a device copy of x whose first element sits on a 16-byte boundary (what the matrix-pipe FIR kernels ask of a span)"""
    pad = 4 if x.dtype == np.float32 else 2
    t = torch.empty(x.size + pad, dtype=torch.from_numpy(x[:1]).dtype, device="cuda")[pad:][:x.size]
    t.copy_(torch.from_numpy(x))
    return t


@pytest.mark.parametrize("cplx,ntaps", [(False, 64), (False, 200), (True, 256), (True, 64)])
def test_fir_non_finite_samples(G, cplx, ntaps):
    """One +Inf, one NaN and one finite sample above bf16's largest value (3.4e38) in a long stream.  The reference's transform_reduce
    (time_domain_filter.hpp:44-47) gives +-Inf / NaN on exactly the ntaps outputs whose window contains the sample and leaves 3.4e38 finite.
      GR4HIP_FIR_EXACT_F32: the same classes (+Inf, -Inf, NaN) on the same outputs, everything else inside the parity bar.
      default (three-term bf16 products on the matrix pipe): what include/gr4hip.h promises instead -- every output the reference makes non-finite is
      non-finite (as NaN), the reach is the kernel's 32-sample-granular window (at most 15 outputs earlier and 46 later than the reference's), a sample
      above 3.39e38 counts as infinite, and all other outputs are inside the parity bar."""
    n = 300_000
    pos = {"inf": 50_001, "nan": 120_003, "big": 200_005}
    b = O.design_taps_hamming_lowpass(ntaps, 0.1)
    x = (O.signal_c32 if cplx else O.signal_f32)(7, n)
    x[pos["inf"]] = np.inf
    x[pos["nan"]] = np.nan
    x[pos["big"]] = 3.4e38
    truth, _ = O.fir(b, x)
    with np.errstate(over="ignore", invalid="ignore"):
        t32 = truth.astype(np.complex64 if cplx else np.float32)
    tbad = ~np.isfinite(t32)
    assert int(tbad.sum()) == 2 * ntaps                                     # the reference: exactly ntaps outputs per non-finite sample, 3.4e38 stays finite
    xc = x.copy()
    xc[list(pos.values())] = 0
    rms = float(np.sqrt(np.mean(np.abs(O.fir(b, xc)[0]) ** 2)))             # level of the ordinary output
    tol = lambda y, m: float(np.max(np.abs(y[m] - truth[m]) / np.maximum(np.abs(truth[m]), rms)))
    dt = torch.complex64 if cplx else torch.float32
    # --- exact float32 arithmetic, per handle
    f = G.fir_filter(b, dt)
    f.set_algo(G.capi.FIR_EXACT_F32)
    y = f.process_bulk(_aligned16(x)).cpu().numpy()
    for part in ((np.real, np.imag) if cplx else (np.asarray,)):
        yp, tp = part(y), part(t32)
        assert np.array_equal(np.isnan(yp), np.isnan(tp)) and np.array_equal(np.isposinf(yp), np.isposinf(tp)) and np.array_equal(np.isneginf(yp), np.isneginf(tp))
    assert tol(y, ~tbad) <= TOL
    # --- default algorithm
    y = G.fir_filter(b, dt).process_bulk(_aligned16(x)).cpu().numpy()
    if True:  # since round 4: the two-term f16 kernels (float and complex) give a segment with such a sample to their float32 paths -- the reference's classes and reach, exactly
        for part in ((np.real, np.imag) if cplx else (np.asarray,)):
            yp, tp = part(y), part(t32)
            assert np.array_equal(np.isnan(yp), np.isnan(tp)) and np.array_equal(np.isposinf(yp), np.isposinf(tp)) and np.array_equal(np.isneginf(yp), np.isneginf(tp))
        assert tol(y, ~tbad) <= TOL
        f = G.fir_filter(b, dt)
        f.set_algo(G.capi.FIR_TIME_DOMAIN_BF16X3)  # the three-term bf16 kernel, per handle: what the text above says
        y = f.process_bulk(_aligned16(x)).cpu().numpy()
    ybad = ~np.isfinite(y)
    assert not np.any(tbad & ~ybad)                                         # nothing the reference makes non-finite comes out finite
    allowed = np.zeros(n, bool)
    for m in pos.values():                                                  # (3.4e38 counts as infinite on this path)
        allowed[max(0, m - 15): m + ntaps + 46] = True
    assert not np.any(ybad & ~allowed), np.flatnonzero(ybad & ~allowed)[:8]
    for m in pos.values():
        assert np.all(ybad[m: m + ntaps])
    assert tol(y, ~ybad) <= TOL


@pytest.mark.parametrize("ntaps", [256, 64])
def test_chain_non_finite_samples(G, ntaps):
    """the same three samples through fir -> 8192-point FFT -> |X|^2: a frame whose filtered samples contain a non-finite value has no finite bin in the
    reference either.  Every algorithm marks those frames; the frequency-domain kernels' correction term reads the last 255 samples of the previous frame
    whatever the tap count, so with fewer than 256 taps a non-finite sample 64 .. 255 samples before a frame boundary also takes the following frame
    (include/gr4hip.h says so); the time-domain algorithm marks exactly the reference's frames.  All other frames stay inside the parity bar."""
    N = 8192
    b = O.design_taps_hamming_lowpass(ntaps, 0.1)
    x = O.signal_c32(9, 12 * N)
    x[2 * N + 100] = np.inf        # early in frame 2: frame 2 only
    x[5 * N - 100] = np.nan        # 100 samples before the end of frame 4: frame 5 too iff ntaps > 100
    x[8 * N - 200] = 3.4e38        # 200 samples before the end of frame 7 (finite in the reference's filter, far beyond float32 in its spectrum)
    x[10 * N + 5] = np.nan
    truth, _ = O.chain(b, x, N, 0, truth=True)
    t2 = truth.reshape(-1, N)
    with np.errstate(over="ignore", invalid="ignore"):
        tbad = np.any(~np.isfinite(t2.astype(np.float32)), axis=1)
    want = {2, 4, 7, 10} | ({5, 8} if ntaps > 200 else set())
    assert set(np.flatnonzero(tbad).tolist()) == want
    for algo in (G.capi.CHAIN_AUTO, G.capi.CHAIN_FUSED_FD, G.capi.CHAIN_TIME_DOMAIN):
        y = G.Chain(b, N, "None", algo).process_bulk(dev(x)).cpu().numpy().reshape(-1, N)
        gbad = np.any(~np.isfinite(y), axis=1)
        marked = set(np.flatnonzero(gbad).tolist())
        assert want <= marked, (algo, marked)
        extra = marked - want
        assert extra <= ({5, 8} if algo != G.capi.CHAIN_TIME_DOMAIN else set()), (algo, extra)
        for f in marked:                                                  # a marked frame is marked in every bin -- but for a bin where the filter has a ZERO: an even-length
            assert np.count_nonzero(np.isfinite(y[f])) <= 1, (algo, f)    # symmetric low-pass cancels the 3.4e38 sample exactly at fs / 2 when the products are float32
        for f in set(range(12)) - marked:
            assert _rel(y[f], t2[f]) <= TOL, (algo, f)


def test_chain_process_multi_one_launch(G):
    """gr4hip_chain_process_multi: the parallel channels of one device in ONE launch.  Shared taps + sum only: the fold math::Add (Math.hpp:73-108) kept in
    registers; own taps per channel: workgroup b works for channel b mod n.  Both against the float64 oracle, histories carried across calls, frame counts
    below and above the grid size, and the chain-by-chain fallback for plans the single launch does not take."""
    from gnuradio4_amd.blocks import chain_process_multi
    N = 8192
    nch = 3
    b = O.design_taps_hamming_lowpass(256, 0.1)
    calls = (5, 301)
    xs = [O.signal_c32(70 + c, sum(calls) * N, tone_frel=0.05 + 0.01 * c) for c in range(nch)]
    truths = [O.chain(b, xs[c], N, 0, truth=True)[0].reshape(-1, N) for c in range(nch)]
    tsum = truths[0] + truths[1] + truths[2]
    # (1) shared taps, only the sum asked for: one launch, fold in registers
    chains = [G.Chain(b, N, "None") for _ in range(nch)]
    got, f0 = [], 0
    for k in calls:
        _, s_ = chain_process_multi(chains, [dev(x[f0 * N:(f0 + k) * N]) for x in xs], want_outs=False)
        got.append(s_.cpu().numpy())
        f0 += k
    assert _rel(np.concatenate(got), tsum) <= TOL
    r, td = chains[0].last_power_ratio()
    assert not td and r > 0.08
    # the same handles go on one by one: the histories the multi launch left behind are the right ones
    x_more = [O.signal_c32(90 + c, 2 * N) for c in range(nch)]
    for c in range(nch):
        want, _ = O.chain(b, np.concatenate([xs[c][-N:], x_more[c]]), N, 0, truth=True)
        assert _rel(chains[c].process_bulk(dev(x_more[c])).cpu().numpy().ravel(), want.reshape(-1, N)[1:].ravel()) <= TOL
    # (2) own taps per channel, spectra and sum
    bs = [O.design_taps_hamming_lowpass(256 - 31 * c, 0.08 + 0.03 * c) for c in range(nch)]
    tr2 = [O.chain(bs[c], xs[c], N, 0, truth=True)[0].reshape(-1, N) for c in range(nch)]
    chains2 = [G.Chain(bs[c], N, "None") for c in range(nch)]
    outs_all, sums_all, f0 = [[] for _ in range(nch)], [], 0
    for k in calls:
        sum_out = torch.empty((k, N), dtype=torch.float32, device="cuda")
        outs, s_ = chain_process_multi(chains2, [dev(x[f0 * N:(f0 + k) * N]) for x in xs], sum_out=sum_out)
        for c in range(nch):
            outs_all[c].append(outs[c].cpu().numpy())
        sums_all.append(s_.cpu().numpy())
        f0 += k
    for c in range(nch):
        assert _rel(np.concatenate(outs_all[c]), tr2[c]) <= TOL, c
    assert _rel(np.concatenate(sums_all), tr2[0] + tr2[1] + tr2[2]) <= TOL
    # the n-ary Add is a LEFT fold: bit-identical to (o0 + o1) + o2 of the published spectra
    o = [np.concatenate(outs_all[c]) for c in range(nch)]
    assert np.array_equal(np.concatenate(sums_all), (o[0] + o[1]) + o[2])
    # (3) plans the single launch does not take (1024-point Hann here) are served chain by chain with the same interface
    b64 = O.design_taps_hamming_lowpass(100, 0.1)
    ch3 = [G.Chain(b64, 1024, "Hann") for _ in range(2)]
    x3 = [O.signal_c32(33 + c, 24 * 1024) for c in range(2)]
    outs, s_ = chain_process_multi(ch3, [dev(x) for x in x3], sum_out=torch.empty((24, 1024), dtype=torch.float32, device="cuda"))
    t3 = [O.chain(b64, x3[c], 1024, O.WINDOWS.index("Hann"), truth=True)[0].reshape(-1, 1024) for c in range(2)]
    for c in range(2):
        assert _rel(outs[c].cpu().numpy(), t3[c]) <= TOL
    assert _rel(s_.cpu().numpy(), t3[0] + t3[1]) <= TOL


def test_chain_process_multi_guard(G):
    """the dynamic-range guard inside the multi launch: an interferer on ONE channel (own-taps mode: per-channel verdicts; fold mode: a frame is marked when any channel's
    share of it fell below the threshold).  GUARD_STRICT since round 5: the marked frames are evaluated again on the device behind the launch (chain_redo_kernel per
    channel, chain_redo_fold_kernel for the fold: every channel of a marked frame again, the sum kept in registers) -- the call does not wait; the NEXT call finds the
    measurement and moves the guarded chains to the time-domain kernels"""
    from gnuradio4_amd.blocks import chain_process_multi
    N, ntaps, nch = 8192, 64, 3
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    clean = [O.signal_c32(5 + c, 24 * N, tone_frel=0.01, tone_amp=1.0) for c in range(nch)]
    loud = O.signal_c32(16, 24 * N, tone_frel=0.31, tone_amp=30.0)
    second = [clean[0], loud, clean[2]]
    truths = [O.chain(b, np.concatenate([clean[c], second[c], second[c]]), N, 0, truth=True)[0].reshape(3, -1) for c in range(nch)]
    for fold in (False, True):
        chains = [G.Chain(b, N, "None") for _ in range(nch)]
        o1, s1 = chain_process_multi(chains, [dev(x) for x in clean], want_outs=not fold, sum_out=torch.empty((24, N), dtype=torch.float32, device="cuda"))
        assert not any(c.last_power_ratio()[1] for c in chains)
        o2, s2 = chain_process_multi(chains, [dev(x) for x in second], want_outs=not fold, sum_out=torch.empty((24, N), dtype=torch.float32, device="cuda"))
        assert _rel(s1.cpu().numpy().ravel(), sum(t[0] for t in truths)) <= TOL
        assert _rel(s2.cpu().numpy().ravel(), sum(t[1] for t in truths)) <= TOL, fold  # (the marked frames were evaluated again behind the launch)
        if not fold:
            for c in range(nch):
                assert _rel(o2[c].cpu().numpy().ravel(), truths[c][1]) <= TOL, c
        assert not chains[1].last_power_ratio()[1], fold                                  # (nothing has moved yet: nobody waited for the measurement)
        o3, s3 = chain_process_multi(chains, [dev(x) for x in second], want_outs=not fold, sum_out=torch.empty((24, N), dtype=torch.float32, device="cuda"))
        assert chains[1].last_power_ratio()[1], fold                                      # the third call found it: the guarded chains run in the time domain from here on
        assert _rel(s3.cpu().numpy().ravel(), sum(t[2] for t in truths)) <= TOL, fold


def test_chain_process_multi_mixed_guard_modes(G):
    """a multi launch over chains with DIFFERENT guard modes: a GUARD_OFF chain is never moved to the time domain (and its history is put back before the rejected
    span is redone), a GUARD_OFF chain 0 does not switch the others' guard off (the in-register fold would measure into chain 0 only), and one STRICT chain makes
    the launch strict"""
    from gnuradio4_amd.blocks import chain_process_multi
    N, ntaps, nch = 8192, 64, 3
    b = O.design_taps_hamming_lowpass(ntaps, 0.02)
    clean = [O.signal_c32(25 + c, 24 * N, tone_frel=0.01, tone_amp=1.0) for c in range(nch)]
    loud = O.signal_c32(36, 24 * N, tone_frel=0.31, tone_amp=30.0)
    second = [clean[0], loud, clean[2]]
    truths = [O.chain(b, np.concatenate([clean[c], second[c], second[c]]), N, 0, truth=True)[0].reshape(3, -1) for c in range(nch)]
    for fold in (False, True):
        chains = [G.Chain(b, N, "None") for _ in range(nch)]
        chains[0].set_guard_mode(G.capi.GUARD_OFF)
        chains[2].set_guard_mode(G.capi.GUARD_DEFERRED)
        o1, s1 = chain_process_multi(chains, [dev(x) for x in clean], want_outs=not fold, sum_out=torch.empty((24, N), dtype=torch.float32, device="cuda"))
        o2, s2 = chain_process_multi(chains, [dev(x) for x in second], want_outs=not fold, sum_out=torch.empty((24, N), dtype=torch.float32, device="cuda"))
        assert _rel(s1.cpu().numpy().ravel(), sum(t[0] for t in truths)) <= TOL
        assert _rel(s2.cpu().numpy().ravel(), sum(t[1] for t in truths)) <= TOL, fold  # the strict chain's marked frames were evaluated again behind the launch ...
        assert not chains[1].last_power_ratio()[1], fold      # ... nobody waited, nothing has moved yet
        o3, s3 = chain_process_multi(chains, [dev(x) for x in second], want_outs=not fold, sum_out=torch.empty((24, N), dtype=torch.float32, device="cuda"))
        assert chains[1].last_power_ratio()[1], fold          # the next call found the measurement: the strict chain runs in the time domain ...
        assert not chains[0].last_power_ratio()[1], fold      # ... and the unguarded chain stays on the fused kernel
        assert chains[0].algo == G.capi.CHAIN_FUSED_FD
        assert _rel(s3.cpu().numpy().ravel(), sum(t[2] for t in truths)) <= TOL, fold
        # the unguarded chain's history survived the move: a further call continues its stream
        third = O.signal_c32(47, 8 * N, tone_frel=0.01)
        t3 = O.chain(b, np.concatenate([clean[0], second[0], second[0], third]), N, 0, truth=True)[0].reshape(-1, N)[72:]
        got = chains[0].process_bulk(dev(third)).cpu().numpy()
        assert _rel(got.ravel(), t3.ravel()) <= TOL, fold


def test_chain_random_configurations(G):
    """seeded random draws over the chain's parameter space (fftSize, tap count, window, frame counts per call): every one against the float64 oracle"""
    rng = np.random.default_rng(2024)
    names = [w for w in O.WINDOWS]
    for case in range(24):
        N = int(rng.choice([256, 512, 1024, 2048, 4096, 8192]))
        ntaps = int(rng.integers(1, 257))
        wid = int(rng.integers(0, len(names)))
        per = 8192 // N
        frames = int(rng.integers(1, 3 * per + 4)) if N < 8192 else int(rng.integers(1, 9))
        b = O.design_taps_hamming_lowpass(ntaps, float(rng.uniform(0.02, 0.4))) if ntaps > 1 else np.array([rng.uniform(0.2, 2.0)], np.float32)
        x = O.signal_c32(100 + case, frames * N, tone_frel=float(rng.uniform(0.0, 0.5)), tone_amp=float(rng.uniform(0.0, 1.0)))  # (stronger out-of-band tones: the dynamic-range test above)
        truth, _ = O.chain(b, x, N, wid, truth=True)
        ch = G.Chain(b, N, names[wid])
        cuts = sorted(set([0, frames] + [int(c) for c in rng.integers(0, frames + 1, size=2)]))
        got = np.concatenate([ch.process_bulk(dev(x[a * N: c * N])).cpu().numpy().ravel() for a, c in zip(cuts[:-1], cuts[1:]) if c > a])
        assert got.shape == truth.shape and _rel(got, truth) <= TOL, (case, N, ntaps, names[wid], frames, cuts)


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_chain_small_fft_size_chunking(G, N):
    """fftSize < 8192 runs 8192-sample blocks through the fused kernel and stages the ragged tail: any split of the stream into calls
    (tail only, blocks only, blocks + tail) must give the spectra of the unfused kernels"""
    per = 8192 // N
    b = O.design_taps_hamming_lowpass(64, 0.1)
    frames = 5 * per + 3
    x = dev(O.signal_c32(11, frames * N))
    ref = G.Chain(b, N, "Hann", 1).process_bulk(x)
    ch = G.Chain(b, N, "Hann", G.capi.CHAIN_FUSED_FD)
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    cuts = [0, 1, per, 2 * per + 1, 4 * per + 1, frames]  # 1 frame (tail only), per-1, per+1 (block + tail), 2 blocks, rest
    got = torch.cat([ch.process_bulk(x[a * N: c * N]) for a, c in zip(cuts[:-1], cuts[1:])])
    assert got.shape == ref.shape
    floor = ref.pow(2).mean().sqrt()

    def close(a):  # both sides carry float32 rounding: twice the parity tolerance, relative to max(|bin|, rms) like _rel
        return float(((a - ref).abs() / torch.maximum(ref.abs(), floor)).max()) <= 2 * TOL
    assert close(got)
    ch.reset()
    assert close(ch.process_bulk(x))


def test_chain_matches_reference_block_magnitude(G):
    """mag2[(k+N/2) mod N] == (magnitude_block[k]*N/2)^2 ties the stream to the FFT block's DataSet output."""
    N = 1024
    b = O.design_taps_hamming_lowpass(64, 0.1)
    x = O.signal_c32(1, 2 * N)
    m2 = G.Chain(b, N, "Hann").process_bulk(dev(x)).cpu().numpy()
    y = G.fir_filter(b, torch.complex64).process_bulk(dev(x))
    mag = G.FFT(N, "Hann").process_bulk(y)["magnitude"].cpu().numpy()
    np.testing.assert_allclose(np.fft.fftshift(m2, axes=1), (mag.astype(np.float64) * N / 2) ** 2, rtol=1e-4, atol=1e-6 * m2.max())


@pytest.mark.parametrize("window", ["None", "Hann"])
def test_chain_parity_many_frames_per_workgroup(G, window):
    """the persistent grid at bench scale: more frames than CUs, so every workgroup loops (double-buffered LDS-DMA, deferred stores,
    carried tail) -- sampled frames straight against the float64 oracle on the same device-generated stream, in two calls so that the
    history crosses a call boundary in the middle of a workgroup's share"""
    N, frames, ntaps = 8192, 1400, 256  # > 5 frames per workgroup on 256 CUs
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    b = O.design_taps_hamming_lowpass(ntaps, 0.1)
    x = G.synth_c32(frames * N, seed=17)
    ch = G.Chain(b, N, window)
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    cut = 777
    got = torch.cat([ch.process_bulk(x[: cut * N]), ch.process_bulk(x[cut * N:])])
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for f in sorted({0, 1, n_cu - 1, n_cu, n_cu + 1, 2 * n_cu, 599, 600, cut - 1, cut, cut + 1, 1024, frames - 2, frames - 1}):
        lo = max(f - 1, 0)
        truth, _ = O.chain(b, x[lo * N:(f + 1) * N].cpu().numpy(), N, wid, truth=True)
        assert _rel(got[f].cpu().numpy(), truth.reshape(-1, N)[f - lo]) <= TOL, (window, f)


def test_chain_full_size_properties(G):
    """BASELINE-size frames (N=8192, 256 taps) over a long device-generated stream: size-independent properties."""
    N, frames = 8192, 512
    b = O.design_taps_hamming_lowpass(256, 0.1)
    x = G.synth_c32(frames * N, seed=5)
    ch = G.Chain(b, N, "None")
    whole = ch.process_bulk(x)
    ch.reset()
    parts = torch.cat([ch.process_bulk(x[: 100 * N]), ch.process_bulk(x[100 * N: 101 * N]), ch.process_bulk(x[101 * N:])])
    assert float((whole - parts).abs().max()) <= 1e-5 * float(whole.pow(2).mean().sqrt())  # chunking invariance
    # linearity of the underlying filter+transform: |F(2x)|^2 == 4 |F(x)|^2
    ch.reset()
    twice = ch.process_bulk(2 * x)
    assert float((twice - 4 * whole).abs().max()) <= 1e-5 * float((4 * whole).pow(2).mean().sqrt())
    # Parseval against the separately filtered stream
    y = G.fir_filter(b, torch.complex64).process_bulk(x)
    e_t = float((y.abs().double() ** 2).sum())
    assert abs(float(whole.double().sum()) / (N * e_t) - 1) < 1e-5
    # tone at 0.1 fs sits in the passband: its bin dominates every frame
    assert torch.all(whole.argmax(dim=1) == round(0.1 * N))


def test_bench_size_launch_properties(G):
    """one launch of the bench's size (2^28 samples = 32768 frames, 128 per workgroup) on a device-generated stream: chunking invariance against 2^26-sample calls,
    Parseval against the separately filtered stream, and the float64 oracle on frames from every region of the launch (first, across a call seam of the
    chunked run, deep inside a workgroup's share, last)"""
    N, frames = 8192, 1 << 15
    b = O.design_taps_hamming_lowpass(256, 0.1)
    x = G.synth_c32(frames * N, seed=11)
    ch = G.Chain(b, N, "None")
    whole = ch.process_bulk(x)
    ch.reset()
    q = frames // 4
    parts = torch.cat([ch.process_bulk(x[i * q * N:(i + 1) * q * N]) for i in range(4)])
    rms = float(whole.double().pow(2).mean().sqrt())
    assert float((whole - parts).abs().max()) <= 1e-5 * rms
    del parts
    y = G.fir_filter(b, torch.complex64).process_bulk(x)
    assert abs(float(whole.double().sum()) / (N * float((y.abs().double() ** 2).sum())) - 1) < 1e-5
    del y
    for f in (0, q - 1, q, 12345, frames - 1):
        lo = max(f - 1, 0)
        truth, _ = O.chain(b, x[lo * N:(f + 1) * N].cpu().numpy(), N, 0, truth=True)
        assert _rel(whole[f].cpu().numpy(), truth.reshape(-1, N)[f - lo]) <= TOL, f


@pytest.mark.parametrize("order,fc", [(8, 0.022), (6, 0.021), (8, 0.031)])
def test_fir_iir_narrow_butterworth_against_the_float32_cascade(G, order, fc):
    """profiles/r04_fuzz_summary.txt: decimate-by-8 FIR -> Butterworth order 6 / 8 at cut-off <= 0.031 fs came out at 1.0e-5 .. 2.1e-5 in every mode of
    gr4hip_fir_iir_process -- the float32 floor of the cascade's state, not the device's.  Pinned here with the contract's second clause: the bound is the error of
    the reference's own float32 cascade (oracle: gr4o_iir_cascade_f32, iir_filter<float, DF_II> section by section) on the same decimated stream, factor ONE"""
    import gnuradio4_amd.blocks as B
    rng = np.random.default_rng(order)
    n = 200 * 7168 + 8 * 123
    nt = 1000
    k = np.arange(nt); t = np.hamming(nt) * np.sinc(0.1 * (k - (nt - 1) / 2)); taps = (t / t.sum()).astype(np.float32)
    b, a = B.design_iir(G.capi.LOWPASS, order, fc, float("nan"), 1.0, G.capi.BUTTERWORTH)
    x = rng.standard_normal(n).astype(np.float32)
    mid = O.fir_decim(taps, x, 8)[0].astype(np.float32)  # what the decimator hands the cascade (float64 sums, rounded once)
    secs = O.make_sections([(bb, aa) for bb, aa in zip(np.asarray(b, np.float32).reshape(-1, 3), np.asarray(a, np.float32).reshape(-1, 3))])
    truth = O.iir_cascade(secs, mid, 3, f64=True)
    e_ref = min(_rel(O.iir_cascade(secs, mid, form, f64=False), truth) for form in (O.DF_I, O.DF_II))  # (the better of the reference's two default-able forms)
    cut = (n // 8 // 3) * 8
    for mode in (G.capi.FIR_IIR_AUTO, G.capi.FIR_IIR_ONE_LAUNCH, G.capi.FIR_IIR_TWO_LAUNCHES):
        fir, iir = G.fir_filter(taps, torch.float32, decimate=8), G.iir_filter(b, a)
        xd = dev(x)
        y = np.concatenate([B.fir_iir_process(fir, iir, xd[:cut], mode=mode).cpu().numpy(), B.fir_iir_process(fir, iir, xd[cut:], mode=mode).cpu().numpy()])
        e = _rel(y, truth)
        assert e <= max(TOL, e_ref), (mode, e, e_ref)


def test_configs2_full_size_properties(G):
    """BASELINE configs[2] at bench size (2^27 input samples: frequency-domain decimator + sequential-run IIR): chunking invariance over calls that take
    different kernels, linearity, DC gain of the decimated stream, and the float64 oracle on a slice deep inside the span"""
    n = (1 << 27) + 8 * 1234  # not a whole number of decimator hops: the partial last block rides in the launch
    k = np.arange(1024) - 511.5
    t = np.hamming(1024) * 0.1 * np.sinc(0.1 * k)
    taps = (t / t.sum()).astype(np.float32)
    bi, ai = G.blocks.design_iir(G.capi.LOWPASS, 8, 0.05, float("nan"), 1.0, G.capi.BUTTERWORTH)
    x = G.synth_f32(n, seed=12)
    fir, iir = G.fir_filter(taps, torch.float32, decimate=8), G.iir_filter(bi, ai)
    yd = fir.process_bulk(x)
    yo = iir.process_bulk(yd)
    assert yd.numel() == n // 8
    fir.reset(); iir.reset()
    cuts = [0, 8 * 1000, 8 * 1000 + 7168 * 64 * 3 + 8 * 77, 1 << 26, n]  # polyphase VALU | FD + partial block | FD | FD + partial block
    yd2 = torch.cat([fir.process_bulk(x[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])])
    yo2 = torch.cat([iir.process_bulk(yd2[lo // 8:hi // 8]) for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert float((yd - yd2).abs().max()) <= 1e-5 * float(yd.double().pow(2).mean().sqrt())
    # (two float32 evaluations of the cascade with different run boundaries: each is within 1e-5 of the float64 oracle, so they may differ by up to 2e-5)
    assert float((yo - yo2).abs().max()) <= 2e-5 * float(yo.double().pow(2).mean().sqrt()), float((yo - yo2).abs().max()) / float(yo.double().pow(2).mean().sqrt())
    del yd2, yo2
    fir.reset(); iir.reset()
    y3 = iir.process_bulk(fir.process_bulk(4 * x))  # linearity of the pair (a power of two: every product and sum scales exactly -- the f16 decimator's block exponent moves with it)
    assert float((y3 - 4 * yo).abs().max()) <= 1e-6 * float((4 * yo).double().pow(2).mean().sqrt())
    fir.reset(); iir.reset()
    y3 = iir.process_bulk(fir.process_bulk(-4 * x))  # (a sign flip is not exact on the matrix pipe: its accumulators do not round symmetrically -- 8e-7 of the rms measured)
    assert float((y3 + 4 * yo).abs().max()) <= 1e-5 * float((4 * yo).double().pow(2).mean().sqrt())
    del y3
    ones = torch.ones(1 << 22, dtype=torch.float32, device="cuda")  # DC gain 1 x Butterworth DC gain 1
    fir.reset(); iir.reset()
    dc = iir.process_bulk(fir.process_bulk(ones))
    assert abs(float(dc[-1000:].mean()) - 1.0) <= 1e-5
    m0 = (1 << 26) + 8 * 5000  # oracle on 40000 decimated samples behind 2^26 inputs: the FIR needs 1023 inputs of history, the IIR is warmed up over 30000 outputs
    seg = x[m0 - 8 * 30000 - 1024:m0 + 8 * 40000].cpu().numpy()
    tf, _ = O.fir_decim(taps, seg, 8)
    ti = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(bi, ai)]), tf.astype(np.float32), O.DF_II, f64=True)
    got = yo[m0 // 8:m0 // 8 + 40000].cpu().numpy()
    assert _rel(got, ti[-40000:]) <= TOL
    # the same stream through gr4hip_fir_iir_process: the cascade as the decimator's store epilogue (ONE launch for the whole blocks, the decimated stream never in HBM),
    # in two calls cut inside the span; and the library's own choice (AUTO)
    rms = float(yo.double().pow(2).mean().sqrt())
    for mode in (G.capi.FIR_IIR_ONE_LAUNCH, G.capi.FIR_IIR_AUTO):
        fir.reset(); iir.reset()
        cut = (1 << 26) + 8 * 4321
        y1 = torch.cat([G.blocks.fir_iir_process(fir, iir, x[:cut], mode=mode), G.blocks.fir_iir_process(fir, iir, x[cut:], mode=mode)])
        assert y1.numel() == n // 8
        assert float((y1 - yo).abs().max()) <= 2e-5 * rms, (mode, float((y1 - yo).abs().max()) / rms)
        assert _rel(y1[m0 // 8:m0 // 8 + 40000].cpu().numpy(), ti[-40000:]) <= TOL
        del y1


def test_configs3_full_size_properties(G):
    """BASELINE configs[3] at bench size (64 channels x 256 taps x 2^22 samples): every channel equals the single-stream kernel on its row, linearity, and the
    float64 oracle on slices of three channels"""
    nch, ntaps, n = 64, 256, 1 << 22
    rng = np.random.default_rng(7)
    taps = (rng.standard_normal((nch, ntaps)) / 16).astype(np.float32)
    x = torch.stack([G.synth_f32(n, seed=100 + c) for c in range(nch)])
    fb = G.FirBatched(taps)
    y = fb.process_bulk(x)
    fb2 = G.FirBatched(taps)
    y2 = fb2.process_bulk(2 * x)
    assert float((y2 - 2 * y).abs().max()) <= 1e-5 * float((2 * y).double().pow(2).mean().sqrt())
    del y2
    for c in (0, 31, 63):
        one = G.fir_filter(taps[c], torch.float32).process_bulk(x[c])
        assert float((one - y[c]).abs().max()) <= 1e-5 * float(one.double().pow(2).mean().sqrt())
        seg = x[c, 1_000_000 - 255:1_000_000 + 5000].cpu().numpy()
        truth, _ = O.fir(taps[c], seg)
        assert _rel(y[c, 1_000_000:1_000_000 + 5000].cpu().numpy(), truth[255:]) <= TOL


# ------------------------------------------------------------------ math (a11, a12) + rotator (a13)
_OPS = {"Add": O.ADD, "Subtract": O.SUB, "Multiply": O.MUL, "Divide": O.DIV}


def _rand(dtype_id, n, rng, nonzero=False):
    dt = O.NP_DTYPES[dtype_id]
    if np.issubdtype(dt, np.integer):
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
        if nonzero:
            v[v == 0] = 3
            if info.min < 0:
                v[v == -1] = 5  # INT_MIN / -1 is UB in the reference
        return v
    if np.issubdtype(dt, np.complexfloating):
        return (rng.uniform(0.5, 4, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))).astype(dt)
    return (rng.uniform(0.5, 4, n) * rng.choice([-1, 1], n)).astype(dt)


@pytest.mark.parametrize("dtype_id", range(12))
@pytest.mark.parametrize("opname", list(_OPS))
def test_math_parity(G, dtype_id, opname):
    rng = np.random.default_rng(dtype_id * 7 + _OPS[opname])
    op = _OPS[opname]
    n = 100_003  # vector body + scalar tail
    integer = dtype_id < 8
    ins = [_rand(dtype_id, n, rng, nonzero=(op == O.DIV and k > 0)) for k in range(3)]
    for k in (1, 2, 3):
        got = G.math_nary(opname, [dev(a) for a in ins[:k]]).cpu().numpy()
        want = O.math_nary(op, dtype_id, ins[:k])
        if integer or op in (O.ADD, O.SUB):
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (opname, k)  # bit-exact
        else:
            np.testing.assert_allclose(got, want, rtol=3e-6 if dtype_id in (8, 10) else 1e-14)
    value = _rand(dtype_id, 1, rng, nonzero=True)[0]
    got = G.math_const(opname, dev(ins[0]), value).cpu().numpy()
    want = O.math_const(op, dtype_id, ins[0], value)
    if integer or op in (O.ADD, O.SUB):
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    else:
        np.testing.assert_allclose(got, want, rtol=3e-6 if dtype_id in (8, 10) else 1e-14)


@pytest.mark.parametrize("dtype_id", [O.UF32, O.UF64])
@pytest.mark.parametrize("opname", ["Add", "Subtract", "Multiply", "Divide"])
def test_math_uncertain_value_parity(G, golden, dtype_id, opname):
    """MathOpImpl / MathOpMultiPortImpl<gr::UncertainValue<float | double>> (Math.hpp:25-28, 68-71; the operators of meta/.../UncertainValue.hpp:121-250): streams of
    {value, uncertainty} pairs, uncorrelated propagation; against the oracle (pinned on qa_UncertainValue.cpp's known answers) and those known answers themselves.
    Values are one IEEE operation each -> bit-exact; uncertainties go through hypot (1 ulp between libraries)"""
    rng = np.random.default_rng(dtype_id * 11 + _OPS[opname])
    op, dt = _OPS[opname], O.NP_DTYPES[dtype_id]
    tol = 4e-7 if dt == np.float32 else 1e-15
    n = 100_003
    def rand():
        v = rng.uniform(0.5, 4.0, n) * rng.choice([-1.0, 1.0], n)
        return np.stack([v, rng.uniform(0.0, 0.5, n)], axis=1).astype(dt)
    ins = [rand() for _ in range(3)]
    for k in (1, 2, 3):
        got = G.math_nary(opname, [dev(a) for a in ins[:k]], uncertain=True).cpu().numpy()
        want = O.math_nary(op, dtype_id, ins[:k])
        assert got.shape == (n, 2)
        assert np.array_equal(got[:, 0], want[:, 0]), (opname, k)
        np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=tol * k)
    value = (float(dt(1.75)), float(dt(0.125)))
    got = G.math_const(opname, dev(ins[0]), value, uncertain=True).cpu().numpy()
    want = O.math_const(op, dtype_id, ins[0], value)
    assert np.array_equal(got[:, 0], want[:, 0])
    np.testing.assert_allclose(got[:, 1], want[:, 1], rtol=tol)
    c = golden["uncertain_value"][opname]
    np.testing.assert_allclose(G.math_const(opname, dev(np.array([c["a"]], dt)), c["b"], uncertain=True).cpu().numpy(), np.array([c["out"]], dt), rtol=tol)
    np.testing.assert_allclose(G.math_nary(opname, [dev(np.array([c["a"]], dt)), dev(np.array([c["b"]], dt))], uncertain=True).cpu().numpy(), np.array([c["out"]], dt), rtol=tol)
    # ... and what the reference's own UncertainValue.hpp computes (fixture generated by running it: tests/golden/make_uncertain_fixture.py)
    fx = np.load(os.path.join(O.ROOT, "tests", "golden", "uncertain_value_ops.npz"))["f32" if dtype_id == O.UF32 else "f64"]
    k = ["Add", "Subtract", "Multiply", "Divide"].index(opname)
    fa, fb, fw = np.ascontiguousarray(fx[:, 0:2]), np.ascontiguousarray(fx[:, 2:4]), fx[:, 4 + 2 * k:6 + 2 * k]
    fg = G.math_nary(opname, [dev(fa), dev(fb)], uncertain=True).cpu().numpy()
    assert np.array_equal(fg[:, 0], fw[:, 0])
    np.testing.assert_allclose(fg[:, 1], fw[:, 1], rtol=tol, atol=0)
    # a span that starts anywhere (8- / 16-byte elements in a ring): scalar head and tail around the 16-byte body, and an odd element count
    for off in (1, 3):
        buf = torch.empty((n + 4, 2), dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda")
        buf[off:off + n].copy_(dev(ins[0]))
        got2 = G.math_const(opname, buf[off:off + n], value, uncertain=True).cpu().numpy()
        assert np.array_equal(got2, got)
    assert G.math_nary("Add", [dev(np.zeros((0, 2), dt))], uncertain=True).numel() == 0
    with pytest.raises(G.capi.Gr4HipError):  # merged programs of UncertainValue elements: refused (UNSUPPORTED), the caller keeps one launch per block
        G.capi.check(G.capi.lib().gr4hip_ewise_create(C.byref(C.c_void_p()), dtype_id), "ewise_create")


def test_tiny_and_empty_spans_every_block(G):
    """work() hands a block whatever the upstream produced: 0, 1, 2 ... samples per call must stream exactly like one long call (state carried)"""
    sizes = [0, 1, 2, 3, 7, 0, 31, 33, 255, 257, 1, 1000]
    n = sum(sizes)
    xf, xc = O.signal_f32(8, n), O.signal_c32(9, n)
    b = O.design_taps_hamming_lowpass(45, 0.1)
    bi, ai = G.blocks.design_iir(G.capi.LOWPASS, 4, 0.1, float("nan"), 1.0, G.capi.BUTTERWORTH)
    cases = [("fir f32", lambda: G.fir_filter(b, torch.float32), xf, O.fir(b, xf)[0]),
             ("fir c32", lambda: G.fir_filter(b, torch.complex64), xc, O.fir(b, xc)[0]),
             ("iir", lambda: G.iir_filter(bi, ai), xf, O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(bi, ai)]), xf, O.DF_II, f64=True)),
             ("rotator", lambda: G.Rotator(phase_increment=0.37, initial_phase=0.1), xc, O.rotator(xc.astype(np.complex128), float(np.float32(0.37)), float(np.float32(0.1)))[0]),
             ("rotator (float recurrence)", lambda: G.Rotator(phase_increment=0.37, initial_phase=0.1, algo="recurrence"), xc, O.rotator(xc, 0.37, 0.1)[0])]
    # the float64 instantiations and the interpolator stream the same way
    b64, x64 = b.astype(np.float64) * 1.000000123, xf.astype(np.float64) + 1e-9
    bi64, ai64 = bi.astype(np.float64), ai.astype(np.float64)
    import scipy.signal as sps
    t_iir64 = x64.copy()
    for bb, aa in zip(bi64, ai64):
        t_iir64 = sps.lfilter(bb, aa, t_iir64)
    xc64 = xc.astype(np.complex128)
    cases += [("fir f64", lambda: G.fir_filter(b64, torch.float64), x64, np.convolve(x64, b64)[:n]),
              ("iir f64", lambda: G.iir_filter(bi64, ai64, dtype=torch.float64), x64, t_iir64),
              ("rotator c128", lambda: G.Rotator(phase_increment=0.37, initial_phase=0.1, dtype=torch.complex128), xc64, xc64 * np.exp(1j * (0.1 + 0.37 * np.arange(1, n + 1))))]
    for name, make, x, truth in cases:
        blk, parts, at = make(), [], 0
        for k in sizes:
            parts.append(blk.process_bulk(dev(x[at:at + k])).cpu().numpy())
            assert parts[-1].shape == (k,), (name, k)
            at += k
        assert _rel(np.concatenate(parts), truth) <= (1e-11 if "64" in name or "128" in name else TOL), name
    itp, parts, at = G.fir_interpolator(b, 3, torch.float32), [], 0
    for k in sizes:
        parts.append(itp.process_bulk(dev(xf[at:at + k])).cpu().numpy())
        assert parts[-1].shape == (3 * k,)
        at += k
    assert _rel(np.concatenate(parts), O.fir_interp(b, xf, 3)[0]) <= TOL
    assert G.FFT(64, "Hann", dtype=torch.float64).process_bulk(dev(np.zeros(0, np.float64)))["magnitude"].shape == (0, 32)
    assert G.math_const("Add", dev(np.zeros(0, np.int16)), 3).numel() == 0 and G.math_const("Multiply", dev(np.array([7], np.int16)), 3).cpu().numpy()[0] == 21
    assert G.Decimator(4).process_bulk(dev(np.zeros(0, np.float32))).numel() == 0
    f = G.FFT(64, "Hann")
    assert f.mag2(dev(np.zeros(0, np.complex64))).shape == (0, 64)
    ch = G.Chain(b, 1024, "Hann")
    assert ch.process_bulk(dev(np.zeros(0, np.complex64))).shape == (0, 1024)


def test_float_blocks_any_span_alignment(G):
    """float streams whose spans start 4 bytes past a 16-byte boundary (an odd ring position): fir_filter (VALU and MFMA sizes, decimating), iir_filter,
    Decimator and the real-input FFT block give exactly what they give on aligned spans"""
    n = 1 << 17
    x0 = G.synth_f32(n, seed=4)

    def shifted(off):  # the same samples, starting `off` floats into a fresh aligned allocation
        t = torch.empty(n + 8, dtype=torch.float32, device="cuda")[off:off + n]
        t.copy_(x0)
        return t
    b32, b200 = O.design_taps_hamming_lowpass(32, 0.1), O.design_taps_hamming_lowpass(200, 0.1)
    bi, ai = G.blocks.design_iir(G.capi.LOWPASS, 4, 0.1, float("nan"), 1.0, G.capi.BUTTERWORTH)
    makers = {"fir32": lambda: G.fir_filter(b32, torch.float32), "fir200": lambda: G.fir_filter(b200, torch.float32),
              "fir_decim4": lambda: G.fir_filter(b200, torch.float32, decimate=4), "iir": lambda: G.iir_filter(bi, ai), "decimator": lambda: G.Decimator(4)}
    for name, make in makers.items():
        ref = make().process_bulk(x0)
        for off in (1, 2, 3):
            xin = shifted(off)
            out = torch.empty(ref.numel() + 8, dtype=torch.float32, device="cuda")[off:off + ref.numel()]
            blk = make()
            got = blk.process_bulk(xin, out) if name != "decimator" else blk.process_bulk(xin)
            if name in ("fir200", "fir_decim4"):  # an unaligned output takes the VALU kernel instead of the MFMA one: same filter, different summation order
                assert float((got - ref).abs().max()) <= TOL * float(ref.pow(2).mean().sqrt()), (name, off)
            else:
                assert torch.equal(got, ref), (name, off)
    fr = G.FFT(1024, "Hann", dtype=torch.float32)
    ref = fr.process_bulk(x0)
    got = G.FFT(1024, "Hann", dtype=torch.float32).process_bulk(shifted(1))
    for k in ("magnitude", "phase", "re", "im"):
        assert torch.equal(got[k], ref[k]), k


@pytest.mark.parametrize("dtype_id", [0, 5, 6, 8, 10, 11])
def test_math_any_span_alignment(G, dtype_id):
    """a ring span starts at any element: inputs and output sharing one misalignment keep the 16-byte vector body (scalar head and tail), spans misaligned
    against each other take the element loop -- bit-identical to the aligned call in both cases"""
    rng = np.random.default_rng(dtype_id)
    n = 70_001
    a, b = _rand(dtype_id, n, rng), _rand(dtype_id, n, rng, nonzero=True)
    ref_nary = G.math_nary("Multiply", [dev(a), dev(b)])
    ref_const = G.math_const("Add", dev(a), a[3])
    tdt = ref_nary.dtype
    val = np.array([a[3]], O.NP_DTYPES[dtype_id])

    def view(src, off):  # a device copy of src that starts `off` elements into an aligned allocation
        t = torch.empty(n + 8, dtype=tdt, device="cuda")[off:off + n]
        if src is not None:
            t.copy_(dev(src))
        return t
    for off_a, off_b, off_o in ((1, 1, 1), (3, 3, 3), (1, 2, 0), (0, 0, 5), (7, 0, 3)):
        xa, xb, out = view(a, off_a), view(b, off_b), view(None, off_o)
        G.capi.check(G.capi.lib().gr4hip_math_nary(2, dtype_id, (C.c_void_p * 2)(xa.data_ptr(), xb.data_ptr()), 2, out.data_ptr(), n, None), "nary")
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.uint8), ref_nary.view(torch.uint8)), (off_a, off_b, off_o)
        G.capi.check(G.capi.lib().gr4hip_math_const(0, dtype_id, xa.data_ptr(), out.data_ptr(), n, val.ctypes.data, None), "const")
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.uint8), ref_const.view(torch.uint8)), (off_a, off_o)


@pytest.mark.parametrize("dtype_id", range(12))
def test_math_golden_vectors(G, golden, dtype_id):
    dt = O.NP_DTYPES[dtype_id]
    cast = (lambda v: np.array([int(q) for q in v]).astype(dt)) if np.issubdtype(dt, np.integer) else (lambda v: np.array(v).astype(dt))
    for name in _OPS:
        for case in golden["math_nary"][name]:
            if np.issubdtype(dt, np.integer) and not all(float(v).is_integer() for row in case["inputs"] + [case["output"]] for v in row):
                continue
            got = G.math_nary(name, [dev(cast(v)) for v in case["inputs"]]).cpu().numpy()
            np.testing.assert_allclose(got, cast(case["output"]), rtol=1e-6)
        g = golden["math_const"]
        assert G.math_const(name, dev(np.array([g["x"]], dt)), g["value"]).cpu().numpy()[0] == dt(g[name])
    assert G.math_nary("Add", [dev(np.zeros(0, dt))]).numel() == 0
    with pytest.raises(G.capi.Gr4HipError):
        G.math_nary("Add", [dev(np.zeros(4, dt))] * 33)


def test_rotator_golden_and_parity(G, golden):
    g = golden["rotator"]
    inc = np.float32(np.pi * g["phase_increment_over_pi"])
    r = G.Rotator(phase_increment=float(inc), initial_phase=0.0, sample_rate=1.0)
    assert abs(r.frequency_shift - 0.25) < 1e-3  # qa_Rotator.cpp:76
    y = r.process_bulk(dev(np.ones(g["n"], np.complex64))).cpu().numpy()
    for i in range(g["n"]):
        want = (i + 1) * float(inc)
        assert abs(y[i].real - np.cos(want)) < g["tolerance"] and abs(y[i].imag - np.sin(want)) < g["tolerance"]
    # long stream, algo "recurrence": the float phase accumulation of the reference (incl. its drift) is reproduced across calls
    n = 200_000 + 13
    x = O.signal_c32(3, n)
    cases = ((0.6283185, 0.25), (-0.01, 0.25), (3.0, 0.25), (7.5, 0.25), (-7.5, 0.25), (0.3, -1.0), (-0.3, 9.0), (0.0, 0.25))  # incl. |inc| > 2 pi, start outside [0, 2 pi]
    for inc, ph0 in cases:
        want, ph = O.rotator(x, inc, ph0)
        r = G.Rotator(phase_increment=inc, initial_phase=ph0, algo="recurrence")
        got = np.concatenate([r.process_bulk(dev(x[:777])).cpu().numpy(), r.process_bulk(dev(x[777:])).cpu().numpy()])
        assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want))
        assert r.accumulated_phase == np.float32(ph)  # bit-identical phase state
    # default algo "closed_form": the float64 oracle's phase (gr4o_rotator_c64), one HBM-bound pass; ragged calls, an 8-byte-aligned span, hand-over
    # of the carried phase to the recurrence and back
    x64 = x.astype(np.complex128)
    for inc, ph0 in cases:
        want, ph = O.rotator(x64, float(np.float32(inc)), float(np.float32(ph0)))
        r = G.Rotator(phase_increment=inc, initial_phase=ph0)
        assert r.algo == "closed_form"
        xd = dev(x)
        buf = torch.empty(n + 1, dtype=torch.complex64, device="cuda")
        buf[1:].copy_(xd)
        got = np.concatenate([r.process_bulk(xd[:777]).cpu().numpy(), r.process_bulk(buf[1:][777:100_000]).cpu().numpy(), r.process_bulk(xd[100_000:]).cpu().numpy()])
        assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want)), (inc, ph0)
        two_pi = 2 * np.pi
        dphi = (r.accumulated_phase - ph) % two_pi
        assert min(dphi, two_pi - dphi) <= 2e-6  # the carried float phase: same angle modulo 2 pi, float rounding per call
        # switch algorithms on the live handle: the carried float phase is the hand-over, exactly
        st0 = r.accumulated_phase
        r.set_algo("recurrence")
        a = r.process_bulk(xd[:1000]).cpu().numpy()
        wa, st1 = O.rotator(x[:1000], inc, st0)  # the reference's float recurrence from the carried state
        assert np.max(np.abs(a - wa)) <= 1e-5 * np.max(np.abs(wa)) and r.accumulated_phase == np.float32(st1)
        r.set_algo("closed_form")
        b2 = r.process_bulk(xd[1000:3000]).cpu().numpy()
        wb, _ = O.rotator(x64[1000:3000], float(np.float32(inc)), float(np.float32(st1)))
        assert np.max(np.abs(b2 - wb)) <= 1e-5 * np.max(np.abs(wb))
    with pytest.raises(ValueError):
        G.Rotator(phase_increment=0.1, frequency_shift=0.2)
    r = G.Rotator(frequency_shift=2.0, sample_rate=100.0)
    assert abs(r.phase_increment - 2 * np.pi * 0.02) < 1e-6


def test_rotator_closed_form_phase_survives_many_small_calls(G):
    """scheduler-sized chunks: 20 000 calls of 37 samples.  The closed form's carried phase lives in float64 on the host, so the last call is as close to
    the float64 oracle as the first (a float carried between calls would random-walk 2.4e-7 rad per call: beyond 1e-5 after a few thousand calls)"""
    calls, per = 20_000, 37
    inc, ph0 = 0.6283185, 0.25
    x = O.signal_c32(12, calls * per)
    want, _ = O.rotator(x.astype(np.complex128), float(np.float32(inc)), float(np.float32(ph0)))
    r = G.Rotator(phase_increment=inc, initial_phase=ph0)
    xd = dev(x)
    out = torch.empty_like(xd)
    for c in range(calls):
        r.process_bulk(xd[c * per:(c + 1) * per], out[c * per:(c + 1) * per])
    got = out.cpu().numpy()
    scale = np.max(np.abs(want))
    assert np.max(np.abs(got[-10 * per:] - want[-10 * per:])) <= 1e-5 * scale
    assert np.max(np.abs(got - want)) <= 1e-5 * scale


def test_rotator_leaping_walker_is_bit_identical(G, devsw):
    """small increments take the leaping walker (exact arithmetic progressions inside a binade): every checkpoint, hence every output sample, and
    the carried phase must equal the plain sample-by-sample walker's, bit for bit -- also for increments that tie between two ulps, that vanish
    against the phase, that are negative, and across calls"""
    n = (1 << 20) + 77
    x = G.synth_c32(n, seed=9)
    rng = np.random.default_rng(5)
    incs = [0.01, -0.01, 0.2499, 1e-3, -3.3e-4, 1e-7, 1.5 * 2.0 ** -23, 2.5 * 2.0 ** -22, -1.5 * 2.0 ** -21, 2.0 ** -10, 0.1, 6.1e-5, 1.0, -2.5, 7.0] + list(rng.uniform(-0.25, 0.25, 6))
    for inc in incs:
        for ph0 in (0.25, 6.2831, 0.0):
            res = {}
            for mode in ("leap", "walk"):
                if mode == "walk":
                    devsw("GR4HIP_ROTATOR_LEAP", 0)
                    devsw("GR4HIP_ROTATOR_WALK", 1)
                else:  # force the leaping walker also above the increment where the library would stop using it: short segments stress its boundary logic
                    devsw("GR4HIP_ROTATOR_WALK", 0)
                    devsw("GR4HIP_ROTATOR_LEAP", 1)
                r = G.Rotator(phase_increment=float(np.float32(inc)), initial_phase=ph0, algo="recurrence")
                y = torch.cat([r.process_bulk(x[:100001]), r.process_bulk(x[100001:])])
                res[mode] = (y, r.accumulated_phase)
            assert res["leap"][1] == res["walk"][1], (inc, ph0)
            assert torch.equal(res["leap"][0].view(torch.float32), res["walk"][0].view(torch.float32)), (inc, ph0)
    devsw("GR4HIP_ROTATOR_WALK", 0)
    devsw("GR4HIP_ROTATOR_LEAP", 0)
    # and against the oracle's float recurrence (library defaults: these increments leap)
    xs = O.signal_c32(3, 300_000)
    for inc in (0.01, -0.003, 2.0 ** -12):
        want, ph = O.rotator(xs, inc, 0.5)
        r = G.Rotator(phase_increment=inc, initial_phase=0.5, algo="recurrence")
        got = r.process_bulk(dev(xs)).cpu().numpy()
        assert np.max(np.abs(got - want)) <= 1e-5 * np.max(np.abs(want)) and r.accumulated_phase == np.float32(ph)



def test_chain16_kernel_matches_oracle_and_the_eight_wave_kernel():
    """the 16-wave kernel (csrc/chain16.hip, selected per process with GR4HIP_CHAIN16=1) on the headline configuration: sampled frames against the
    float64 oracle, every frame against the 8-wave kernel's output of this process, history across calls, the filter-less |FFT|^2 mode"""
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, ROOT); sys.path.insert(0, ROOT + "/tests")
import gnuradio4_amd as G, oracle_lib as O
N, frames = 8192, 700
b = O.design_taps_hamming_lowpass(256, 0.1)
x = G.synth_c32(frames * N, seed=23)
ch = G.Chain(b, N, "None")
got = torch.cat([ch.process_bulk(x[: 301 * N]), ch.process_bulk(x[301 * N:])])
F = G.FFT(N, "None")
np.savez(OUT, chain=got.cpu().numpy(), fft=F.mag2(x[: 300 * N]).cpu().numpy())
'''
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for flag in ("0", "1"):
            out = os.path.join(td, f"k{flag}.npz")
            env = dict(os.environ, GR4HIP_CHAIN16=flag)
            p = subprocess.run([sys.executable, "-c", code.replace("ROOT", repr(root)).replace("OUT", repr(out))], env=env, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
            outs[flag] = dict(np.load(out))
    N = 8192
    for key in ("chain", "fft"):
        a, c = outs["0"][key].astype(np.float64), outs["1"][key].astype(np.float64)
        rms = np.sqrt(np.mean(a ** 2, axis=1, keepdims=True))
        assert np.max(np.abs(a - c) / np.maximum(np.abs(a), rms)) <= 2e-6, key  # two float32 evaluations of the same spectra
    import gnuradio4_amd as G2
    x = G2.synth_c32(700 * N, seed=23)
    b = O.design_taps_hamming_lowpass(256, 0.1)
    for f in (0, 1, 255, 256, 300, 301, 302, 699):
        lo = max(f - 1, 0)
        truth, _ = O.chain(b, x[lo * N:(f + 1) * N].cpu().numpy(), N, 0, truth=True)
        assert _rel(outs["1"]["chain"][f], truth.reshape(-1, N)[f - lo]) <= TOL, f


# ------------------------------------------------------------------ a15: the device-side generator behind the bench input and the long-stream tests
def test_device_generator_is_the_reference_prng(G, golden):
    """gr4hip_synth_*: group g of 8 samples has its own Xoshiro256pp(seed ^ MIX (g + 1)) and is filled with the reference's GaussianNoise recipe.
    The integer core is pinned by the reference's seed-0 known answer (qa_Xoshiro256pp.cpp:55-69) and bit for bit by the oracle (itself bit-exact
    against the reference's own header, oracle/_ref); the float samples by the oracle's fill / fillComplex for the same generator; plus statistics."""
    MIX, M64 = G.capi.SYNTH_MIX, 2 ** 64 - 1
    want0 = [int(h, 16) for h in golden["xoshiro_seed0_first5"]["draws_hex"]]
    got0 = [int(v) & M64 for v in G.synth_draws(5, MIX, 0).cpu().numpy()]  # seed ^ MIX * 1 == 0: the generator is Xoshiro256pp(0)
    assert got0 == want0
    for seed, g in ((42, 0), (42, 7), (43, 123456789), (0, 2 ** 40)):
        sg = (seed ^ (MIX * (g + 1))) & M64
        got = G.synth_draws(64, seed, g).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, O.xoshiro_draws(sg, 64)), (seed, g)
    # samples: every 8-sample group is fillComplex / fill of its own generator (float log / sqrt differ by an ulp or two between libm and the device)
    n, seed = 1 << 16, 42
    xc = G.synth_c32(n, seed=seed, tone_frel=0.1, tone_amp=1.0, noise_amp=1.0).cpu().numpy()
    xf = G.synth_f32(n, seed=seed, tone_frel=0.1, tone_amp=1.0, noise_amp=1.0).cpu().numpy()
    for g in (0, 1, 2, 777, n // 8 - 1):
        sg = (seed ^ (MIX * (g + 1))) & M64
        i = np.arange(8 * g, 8 * g + 8, dtype=np.float64)
        ph = 2 * np.pi * np.mod(0.1 * i, 1.0)
        wc = O.gauss_c32(sg, 8).astype(np.complex128) + np.exp(1j * ph)
        wf = O.gauss_f32(sg, 8).astype(np.float64) + np.sin(ph)
        assert np.max(np.abs(xc[8 * g: 8 * g + 8] - wc)) <= 4e-6, g
        assert np.max(np.abs(xf[8 * g: 8 * g + 8] - wf)) <= 4e-6, g
    # statistics of the bench input (2^22 samples): unit noise power, zero mean, independent components, the tone on its bin
    n = 1 << 22
    z = G.synth_c32(n, seed=42, tone_frel=0.0, tone_amp=0.0, noise_amp=1.0)
    p = float((z.abs().double() ** 2).mean())
    assert abs(p - 1.0) < 5e-3 and abs(complex(z.mean())) < 3e-3
    assert abs(float((z.real.double() * z.imag.double()).mean())) < 3e-3 and abs(float((z.real.double() ** 2).mean()) - 0.5) < 3e-3
    assert abs(float((z[1:].real.double() * z[:-1].real.double()).mean())) < 3e-3  # neighbours (same group and across groups) uncorrelated
    zt = G.synth_c32(n, seed=42, tone_frel=0.1, tone_amp=1.0, noise_amp=1.0)
    m2 = G.FFT(8192, "None").mag2(zt[: 64 * 8192]).double().mean(dim=0)
    assert int(m2.argmax()) == 819  # 0.1 fs * 8192 = 819.2
    assert abs(float((zt.abs().double() ** 2).mean()) - 2.0) < 1e-2  # unit tone + unit noise


# ---------------------------------------------------------------------------------------------------------------- float64 instantiations
# the second registered type of the filter / fourier / rotator blocks (time_domain_filter.hpp:20, 57-60; fourier/fft.hpp:29; Rotator.hpp:15).  Truth: the
# same formulas in float64 (numpy / the oracle's double sections); the device differs only by the order of its float64 sums, so the bar is 1e-12, not 1e-5
TOL64 = 1e-12


@pytest.mark.parametrize("ntaps,decim", [(1, 1), (7, 1), (64, 1), (300, 1), (1024, 8), (33, 3), (2048, 1)])
def test_fir_filter_float64(G, ntaps, decim):
    rng = np.random.default_rng(ntaps + decim)
    b = rng.standard_normal(ntaps) / np.sqrt(ntaps)
    n = 60_000 - 60_000 % decim
    x = rng.standard_normal(n)
    full = np.convolve(x, b)[:n]  # y[i] = sum_k b[k] x[i - k], zero history
    truth = full[::decim]
    f = G.fir_filter(b, torch.float64, decimate=decim)
    cuts = [0, 3 * decim, 3 * decim + 7000 * decim - (7000 * decim) % decim, n]
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])  # history across calls
    assert y.dtype == np.float64 and y.shape == truth.shape and _rel(y, truth) <= TOL64
    f.reset()
    assert _rel(f.process_bulk(dev(x[:999 * decim])).cpu().numpy(), truth[:999]) <= TOL64
    if ntaps >= 7 and ntaps <= 64:  # settingsChanged keeps the history while it fits (time_domain_filter.hpp:38-42)
        f2 = G.fir_filter(b, torch.float64, decimate=decim)
        y1 = f2.process_bulk(dev(x[:3000 * decim])).cpu().numpy()
        b2 = b[::-1].copy()
        f2.settings_changed(b2)
        y2 = f2.process_bulk(dev(x[3000 * decim:6000 * decim])).cpu().numpy()
        t2 = np.convolve(x[:6000 * decim], b2)[:6000 * decim][::decim][3000:]
        assert _rel(y1, truth[:3000]) <= TOL64 and _rel(y2, t2) <= TOL64
    with pytest.raises(G.capi.Gr4HipError) as e:
        G.fir_filter(np.ones(4096), torch.float64)
    assert e.value.status == G.capi.UNSUPPORTED


@pytest.mark.parametrize("ntaps", [17, 64, 65, 100, 129, 256, 257, 700, 1024, 2048])
def test_fir_filter_float64_matrix_pipe(G, ntaps):
    """fir_filter<double>, 17 .. 2048 taps, spans of >= 32768 samples: the block-Toeplitz contraction on v_mfma_f64_16x16x4_f64 (fir64_mfma_kernel) -- many
    segments per workgroup, ragged ends, history handed between the matrix-pipe and the plain kernel across calls"""
    rng = np.random.default_rng(ntaps)
    b = rng.standard_normal(ntaps) / np.sqrt(ntaps)
    n = 400_003
    x = rng.standard_normal(n)
    truth = np.convolve(x, b)[:n]
    f = G.fir_filter(b, torch.float64)
    cuts = [0, 100_001, 100_004, 105_000, 370_000, 371_000, n]  # long spans (matrix pipe), short ones (plain kernel) in between
    y = np.concatenate([f.process_bulk(dev(x[lo:hi])).cpu().numpy() for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert y.dtype == np.float64 and _rel(y, truth) <= TOL64
    f.reset()
    assert _rel(f.process_bulk(dev(x)).cpu().numpy(), truth) <= TOL64


@pytest.mark.parametrize("kind", ["biquad4", "pole1", "order4", "narrow"])
def test_iir_filter_float64(G, kind):
    import scipy.signal as sps
    rng = np.random.default_rng(3)
    if kind == "biquad4":
        sos = sps.butter(8, 0.1, output="sos")  # 4 biquads
        b, a = sos[:, :3], sos[:, 3:]
    elif kind == "pole1":
        b, a = np.array([[0.3, 0.0]]), np.array([[1.0, -0.7]])
    elif kind == "order4":
        b, a = np.array([[0.1, 0.2, 0.3, 0.2, 0.1]]), np.array([[1.0, -0.9, 0.5, -0.1, 0.02]])
    else:
        sos = sps.butter(4, 0.0005, output="sos")  # poles within 1e-3 of the unit circle: the scan must carry long memory exactly
        b, a = sos[:, :3], sos[:, 3:]
    n = 3 * 8192 * 17 + 1234
    x = rng.standard_normal(n)
    truth = x.copy()
    for bb, aa in zip(b, a):
        truth = sps.lfilter(bb, aa, truth)
    f = G.iir_filter(b, a, dtype=torch.float64)
    cut = 8192 * 5 + 77
    y = np.concatenate([f.process_bulk(dev(x[:cut])).cpu().numpy(), f.process_bulk(dev(x[cut:])).cpu().numpy()])  # state across calls, ragged tiles
    assert y.dtype == np.float64 and _rel(y, truth) <= (1e-9 if kind == "narrow" else TOL64)  # (narrow: condition of the filter itself, ~1e3 / (1 - |p|))
    sec = O.make_sections([(bb, aa) for bb, aa in zip(b, a)])  # and the oracle's own double sections on the (float32-representable) head of the stream
    x32 = x[:50_000].astype(np.float32)
    f.reset()
    assert _rel(f.process_bulk(dev(x32.astype(np.float64))).cpu().numpy(), O.iir_cascade(sec, x32, O.DF_II, f64=True)) <= (1e-9 if kind == "narrow" else TOL64)
    with pytest.raises(G.capi.Gr4HipError) as e:
        G.iir_filter(np.ones((5, 3)), np.ones((5, 3)), dtype=torch.float64)  # 10 state values
    assert e.value.status == G.capi.UNSUPPORTED


_IIR64_CASES = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (1, 2), (2, 2), (3, 2), (4, 2), (1, 3), (2, 3), (1, 4), (2, 4), (1, 5), (1, 6), (1, 7), (1, 8)]


@pytest.mark.parametrize("nsec,order", _IIR64_CASES, ids=[f"{s}x{o}" for s, o in _IIR64_CASES])
def test_iir_filter_float64_every_instantiation(G, nsec, order):
    """every (sections, order) pair of gr4hip_iir64_process's dispatch (GR4_IIR64_CASE, csrc/f64.hip): stable random sections (pole radii <= 0.95), spans of 1, 15, 16,
    17 and 33 tiles plus a ragged tail -- the 16-tile groups of iir64_pass_b --, each in two calls on one handle; against scipy's lfilter section by section.
    A direct-form section of order N loses about eps x kappa in ANY float64 evaluation, lfilter's included, with kappa = ||1 / A||_1 ||a||_1 (the gain from a rounding
    error of the recurrence to its state, times the size of the terms that are rounded): a draw with kappa > 100 (clustered poles: one of order 6 came out at 3900, and
    lfilter itself at 1.5e-13 from a long-double evaluation where the others stay at 1e-15) is drawn again, so that eps x kappa stays 40 times inside TOL64"""
    import scipy.signal as sps
    rng = np.random.default_rng(100 * nsec + order)
    b, a = [], []
    impulse = np.zeros(4000)
    impulse[0] = 1.0
    for _ in range(nsec):
        while True:
            poles = []
            while len(poles) < order:
                if order - len(poles) >= 2:
                    r, th = rng.uniform(0.3, 0.95), rng.uniform(0.1, 3.0)
                    poles += [r * np.exp(1j * th), r * np.exp(-1j * th)]
                else:
                    poles += [rng.uniform(-0.95, 0.95)]
            aa, bb = np.real(np.poly(poles)), rng.uniform(-1, 1, order + 1) * 0.5
            if np.sum(np.abs(sps.lfilter([1.0], aa, impulse))) * np.sum(np.abs(aa)) <= 100.0:
                break
        a.append(aa)
        b.append(bb)
    b, a = np.array(b), np.array(a)
    tile, tail = 8192, 1234
    n = 2 * (33 * tile + tail)
    x = rng.standard_normal(n)
    truth = x.copy()
    for bb, aa in zip(b, a):
        truth = sps.lfilter(bb, aa, truth)
    for tiles in (1, 15, 16, 17, 33):
        m = (tiles - 1) * tile + tail  # `tiles` tiles, the last one ragged
        f = G.iir_filter(b, a, dtype=torch.float64)
        y = np.concatenate([f.process_bulk(dev(x[:m])).cpu().numpy(), f.process_bulk(dev(x[m:2 * m])).cpu().numpy()])
        assert y.dtype == np.float64 and _rel(y, truth[:2 * m]) <= TOL64, (tiles, _rel(y, truth[:2 * m]))


def test_iir_a0_is_taken_as_one(G):
    """a section with a[0] = 2: the reference's computeFilter never reads a[0] (FilterTool.hpp:116-158), nor does the oracle (oracle/gr4_oracle.h: "a[0] assumed 1") --
    nothing is divided by it, on the float32 handle and on the float64 one alike"""
    b, a = np.array([[0.2, 0.3, 0.2], [0.5, -0.1, 0.3]]), np.array([[2.0, -0.9, 0.5], [2.0, 0.3, 0.2]])
    x = O.signal_f32(5, 3 * 8192 + 77)
    a1 = a.copy()
    a1[:, 0] = 1.0
    truth = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b.astype(np.float32), a.astype(np.float32))]), x, O.DF_II, f64=True)
    same = O.iir_cascade(O.make_sections([(bb, aa) for bb, aa in zip(b.astype(np.float32), a1.astype(np.float32))]), x, O.DF_II, f64=True)
    assert np.array_equal(truth, same)  # (the oracle's reading)
    cut = 8192 + 5
    f32 = G.iir_filter(b, a)
    y32 = np.concatenate([f32.process_bulk(dev(x[:cut])).cpu().numpy(), f32.process_bulk(dev(x[cut:])).cpu().numpy()])
    assert _rel(y32, truth) <= TOL
    fs = G.iir_filter(b, a)
    fs.set_algo(G.capi.IIR_SEQUENTIAL_F32)
    assert _rel(fs.process_bulk(dev(x)).cpu().numpy(), truth) <= TOL
    f64 = G.iir_filter(b.astype(np.float32).astype(np.float64), a.astype(np.float32).astype(np.float64), dtype=torch.float64)
    x64 = x.astype(np.float64)
    y64 = np.concatenate([f64.process_bulk(dev(x64[:cut])).cpu().numpy(), f64.process_bulk(dev(x64[cut:])).cpu().numpy()])
    assert _rel(y64, truth) <= TOL64


@pytest.mark.parametrize("kind", ["biquad4", "narrow"])
def test_iir_filter_float64_more_tiles_than_one_scan_round(G, kind):
    """the tile-level scan of the float64 cascade (iir64_pass_b) covers 4096 tiles = 2^25 samples per round: a span beyond that carries the state into a
    second round, and a span that ends inside the first groups leaves most lanes of the scan idle"""
    import scipy.signal as sps
    sos = sps.butter(8, 0.1, output="sos") if kind == "biquad4" else sps.butter(4, 0.0005, output="sos")
    b, a = sos[:, :3], sos[:, 3:]
    n = (1 << 25) + 8192 * 9 + 321
    x = np.random.default_rng(11).standard_normal(n)
    truth = sps.sosfilt(sos, x)
    f = G.iir_filter(b, a, dtype=torch.float64)
    y = f.process_bulk(dev(x)).cpu().numpy()
    bar = 1e-9 if kind == "narrow" else TOL64
    assert _rel(y, truth) <= bar
    f.reset()
    cut = 8192 * 3 + 5  # four tiles in the first call: lanes 1 .. 255 of the scan idle
    y2 = np.concatenate([f.process_bulk(dev(x[:cut])).cpu().numpy(), f.process_bulk(dev(x[cut:1_000_000])).cpu().numpy()])
    assert _rel(y2, truth[:1_000_000]) <= bar


@pytest.mark.parametrize("N", [2, 4, 8, 16, 32, 64, 512, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("window", ["None", "Hann", "BlackmanHarris"])
def test_fft_block_float64(G, N, window):
    """FFT<double>: real double frames; magnitude / phase = bins 0 .. N/2-1, Re / Im = bins N/2 .. N-1 (fft.hpp:221-227), all in double"""
    rng = np.random.default_rng(N)
    frames = 700 if N <= 64 else 5  # (N >= 16: 8192 / N frames share a workgroup -- several workgroups with a partial last one, or one partial workgroup)
    x = rng.standard_normal(frames * N) + np.cos(0.3 * np.arange(frames * N))
    w = np.ones(N) if window == "None" else O.window(O.WINDOWS.index(window), N, np.float64)
    X = np.fft.fft(x.reshape(frames, N) * w, axis=1)
    out = G.FFT(N, window, dtype=torch.float64).process_bulk(dev(x))
    h = N // 2
    assert out["magnitude"].dtype == torch.float64
    assert _rel(out["magnitude"].cpu().numpy(), np.abs(X[:, :h]) * 2 / N) <= TOL64
    assert _rel(out["re"].cpu().numpy(), X[:, h:].real) <= TOL64 and _rel(out["im"].cpu().numpy(), X[:, h:].imag) <= TOL64
    ph, tp = out["phase"].cpu().numpy(), np.angle(X[:, :h])
    d = np.abs(ph - tp)
    d = np.minimum(d, 2 * np.pi - d)  # +-pi is one point
    big = np.abs(X[:, :h]) > 1e-6 * np.abs(X).max()
    assert not big.any() or d[big].max() <= 1e-9  # (N = 2 under a window that is zero at both ends: nothing to compare)
    if N >= 16:
        o2 = G.FFT(N, window, outputInDb=True, outputInDeg=True, unwrapPhase=True, dtype=torch.float64).process_bulk(dev(x))
        assert _rel(o2["magnitude"].cpu().numpy(), 20 * np.log10(np.abs(X[:, :h]) * 2 / N)) <= 1e-9
        tph = np.degrees(np.unwrap(np.angle(X[:, :h]), axis=1))
        if big.all():
            assert np.abs(o2["phase"].cpu().numpy() - tph).max() <= 1e-6
        assert o2["ranges"].shape == (frames, 4, 2)
    with pytest.raises(G.capi.Gr4HipError) as e:
        G.FFT(1000, "None", dtype=torch.float64)
    assert e.value.status == G.capi.UNSUPPORTED


@pytest.mark.parametrize("inc", [1e-3, 0.37, -2.5, 7.0])
def test_rotator_complex128(G, inc):
    rng = np.random.default_rng(5)
    n = (1 << 21) + 333
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    r = G.Rotator(phase_increment=inc, initial_phase=0.25, dtype=torch.complex128)
    cut = 700_001
    y = np.concatenate([r.process_bulk(dev(x[:cut])).cpu().numpy(), r.process_bulk(dev(x[cut:])).cpu().numpy()])
    truth = x * np.exp(1j * (0.25 + inc * np.arange(1, n + 1)))
    assert y.dtype == np.complex128 and np.abs(y - truth).max() <= 1e-9 * np.abs(truth).max()
    yo, _ = O.rotator(x[:4096], inc, 0.25)  # the oracle's float64 recurrence (gr4o_rotator_c64)
    # (beyond 2 pi per sample the recurrence wraps once per step and its accumulator grows without bound: 6.5e-10 of drift in 4096 steps at inc = 7, all its own)
    assert np.abs(y[:4096] - yo).max() <= (1e-10 if abs(inc) < 2 * np.pi else 5e-9)
    assert abs(np.exp(1j * r.accumulated_phase) - np.exp(1j * (0.25 + inc * n))) <= 1e-7
