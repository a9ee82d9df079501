"""The complex-tap FIR on the device (gr4hip_cfir_*, csrc/fir_cplx.hip) against its float64 oracle (tests/complex_fir_oracle.py): every kernel path, the band form's
indices and signs bit for bit, chunking, settings, the guard and its second evaluation, non-finite samples, alignment, the translating decimator and the refusals.
TOL is the parity contract's 1e-5 (include/gr4hip.h); every parity test first shows on the CPU that the float32 sum in fir_filter's order meets 3e-6 on its input, and
that no segment was marked: what is compared is then the main kernel, not the second evaluation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import complex_fir_oracle as CO
import oracle_lib as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
SEQ_TOL = 3e-6
_rel = CO.rel
BIN = os.path.join(O.ROOT, "build", "host", "test_host_complex_fir")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


def _paths(G, f):
    m = C.c_uint(0)
    fn = G.capi.lib().gr4hip_internal_cfir_last_paths  # (test hook, not in include/gr4hip.h)
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_uint)], C.c_int
    assert fn(f._h, C.byref(m)) == 0
    return m.value


def _marked(G, f):
    n = C.c_ulonglong(0)
    fn = G.capi.lib().gr4hip_internal_cfir_marked
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)], C.c_int
    assert fn(f._h, torch.cuda.current_stream().cuda_stream, C.byref(n)) == 0
    return n.value


def _cnoise(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)


def taps(K, D=1, shift=0.2):
    """Hamming low-pass for the decimated rate, shifted to `shift` fs (short filters: random taps)"""
    if K < 8:
        return _cnoise(np.random.default_rng(K), K)
    h = O.design_taps_hamming_lowpass(K, 0.4 / (2 * D)).astype(np.float64)
    return (h * np.exp(2j * np.pi * shift * np.arange(K))).astype(np.complex64)


def signal(n, seed, tone=0.21, amp=1.0):
    """unit complex noise plus a tone (in the pass band of taps() by default)"""
    rng = np.random.default_rng(seed)
    return (_cnoise(rng, n) + amp * np.exp(2j * np.pi * tone * np.arange(n))).astype(np.complex64)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _seq_ok(b, x, D, t):
    e = _rel(CO.cfir32_seq(b, x, D), t)
    assert e <= SEQ_TOL, f"the float32 sum in fir_filter's order errs {e:.2e} on this input"


@pytest.mark.parametrize("D", [1, 2, 3, 8])
@pytest.mark.parametrize("K", [1, 2, 16, 17, 33, 64, 255, 256, 257, 1024])
def test_parity_over_shapes(G, K, D):
    tile = G.complex_fir_filter.tile()
    n = D * (3 * tile + 37)
    b, x = taps(K, D), signal(n, 1000 * K + D)
    t, _ = CO.cfir64(b, x, D)
    _seq_ok(b, x, D, t)
    f = G.complex_fir_filter(b, D)
    y = f.process_bulk(_dev(x)).cpu().numpy()
    e = _rel(y, t)
    print(f"K {K} D {D}: {e:.2e}")
    assert (_paths(G, f) & 3) == (3 if 17 <= K <= 1024 else 2)  # three tile groups on the matrix pipe + the ragged tail on the direct kernel, or the direct kernel alone
    assert _marked(G, f) == 0
    assert y.shape == (n // D,) and e <= TOL


def test_impulses_bit_for_bit(G):
    """products with 1 and 0 are exact: an impulse reads the taps back, which pins every index and sign of the band form"""
    tile, seg = G.complex_fir_filter.tile(), G.complex_fir_filter.segment()
    K = 100
    b = _cnoise(np.random.default_rng(5), K)
    n = 3 * max(tile, seg) + 37
    f = G.complex_fir_filter(b, 1)
    for n0 in sorted({0, 1, 7, 8, 127, 128, tile - 1, tile, seg - 1, seg}):
        for v, want in ((1.0, b), (1j, (-b.imag + 1j * b.real).astype(np.complex64))):
            x = np.zeros(n, np.complex64)
            x[n0] = v
            f.reset()
            y = f.process_bulk(_dev(x)).cpu().numpy()
            assert _paths(G, f) & 1
            exp = np.zeros(n, np.complex64)
            exp[n0:n0 + K] = want
            assert np.array_equal(y.view(np.float32), exp.view(np.float32)), (n0, v)
    f8 = G.complex_fir_filter(b, 8)
    n8 = 8 * (2 * tile + 37)
    for m in (0, 5, 127, tile - 1, tile):
        x = np.zeros(n8, np.complex64)
        x[8 * m + 3] = 1.0
        f8.reset()
        y = f8.process_bulk(_dev(x)).cpu().numpy()
        exp = np.zeros(n8 // 8, np.complex64)
        for mm in range(m + 1, n8 // 8):  # y[m'] = b[8 (m' - m) - 3]
            k = 8 * (mm - m) - 3
            if k < K:
                exp[mm] = b[k]
        assert np.array_equal(y.view(np.float32), exp.view(np.float32)), m


@pytest.mark.parametrize("K,D", [(100, 1), (100, 3), (300, 8)])
def test_chunking(G, K, D):
    tile = G.complex_fir_filter.tile()
    cuts = [D * (tile + 13), D, D * (K // 3), D * (tile + 300)]  # one call of a single output, one shorter than the filter
    n = sum(cuts) + D * 777
    b, x = taps(K, D), signal(n, 77 + K)
    t, _ = CO.cfir64(b, x, D)
    _seq_ok(b, x, D, t)
    f = G.complex_fir_filter(b, D)
    y1 = f.process_bulk(_dev(x)).cpu().numpy()
    assert _marked(G, f) == 0
    f2 = G.complex_fir_filter(b, D)
    parts, at = [], 0
    for c in cuts + [n - sum(cuts)]:
        parts.append(f2.process_bulk(_dev(x[at:at + c])).cpu().numpy())
        at += c
    y5 = np.concatenate(parts)
    assert _rel(y1, t) <= TOL and _rel(y5, t) <= TOL


def test_taps_and_reset_mid_stream(G):
    """set_taps keeps the history unless its buffer must grow (capacity max(32, bit_ceil(K)), replaced by zeros then: fir_filter's rule); reset zeroes it"""
    tile = G.complex_fir_filter.tile()
    n = tile + 500
    xs = [signal(n, 200 + i) for i in range(5)]
    b64, b300, b40, b200 = taps(64), taps(300), taps(40), taps(200)
    f = G.complex_fir_filter(b64)
    run = lambda x: f.process_bulk(_dev(x)).cpu().numpy()  # noqa: E731
    assert _rel(run(xs[0]), CO.cfir64(b64, xs[0])[0]) <= TOL
    f.settings_changed(b300)  # 300 > capacity 64: the history buffer grows, its content is replaced
    assert _rel(run(xs[1]), CO.cfir64(b300, xs[1])[0]) <= TOL
    f.settings_changed(b40)   # shrinking keeps it
    assert _rel(run(xs[2]), CO.cfir64(b40, xs[2], 1, xs[1])[0]) <= TOL
    f.settings_changed(b200)  # growing inside the capacity (512) keeps it
    t = CO.cfir64(b200, xs[3], 1, xs[2])[0]
    assert _rel(run(xs[3]), t) <= TOL
    assert _rel(CO.cfir64(b200, xs[3])[0], t) > 1e-2  # (the history matters in this comparison)
    f.reset()
    assert _rel(run(xs[4]), CO.cfir64(b200, xs[4])[0]) <= TOL


@pytest.mark.parametrize("D", [1, 8])
def test_guard_redoes_rejected_segments(G, D):
    """noise plus a stop-band tone 60 dB above it: the float32 products err by more than TOL of what passes; every segment is marked and evaluated again in float64"""
    K, seg = 256, G.complex_fir_filter.segment()
    n = D * (3 * seg + 37)
    b, x = taps(K, 8), signal(n, 9 + D, tone=-0.3, amp=1000.0)  # (the narrow low-pass of the decimate-by-8 case for both)
    t, _ = CO.cfir64(b, x, D)
    n_seg = -(-(n // D) // seg)
    f = G.complex_fir_filter(b, D)
    y = f.process_bulk(_dev(x)).cpu().numpy()
    assert _paths(G, f) == 7
    marked, e = _marked(G, f), _rel(y, t)
    f.set_guard_mode(G.capi.GUARD_OFF)
    f.reset()
    y_off = f.process_bulk(_dev(x)).cpu().numpy()
    e_off = _rel(y_off, t)
    print(f"D {D}: strict {e:.2e} ({marked} of {n_seg} marked), off {e_off:.2e}, float32 in fir_filter's order {_rel(CO.cfir32_seq(b, x, D), t):.2e}")
    assert marked == n_seg and e <= TOL
    assert _marked(G, f) == 0 and (_paths(G, f) & 4) == 0 and (_paths(G, f) & 3) == 3
    assert e_off > TOL  # the main kernels' own float32 products: without the second evaluation this input misses the bar
    with pytest.raises(G.capi.Gr4HipError) as err:
        f.set_guard_mode(G.capi.GUARD_DEFERRED)
    assert err.value.status == G.capi.UNSUPPORTED


def test_non_finite_samples_reach_exactly_their_window(G):
    tile, seg, K = G.complex_fir_filter.tile(), G.complex_fir_filter.segment(), 64
    n = 3 * max(tile, seg) + 37
    b, x = taps(K), signal(n, 31)
    n0, n1 = tile + 64 + 5, 2 * seg - 1  # the middle of a 16 x 16 tile; the last sample of a segment
    clean = x.copy()
    x[n0] = np.inf
    x[n1] = np.nan
    t, _ = CO.cfir64(b, clean)
    f = G.complex_fir_filter(b)
    y = f.process_bulk(_dev(x)).cpu().numpy()
    bad = np.zeros(n, bool)
    bad[n0:n0 + K] = True
    bad[n1:n1 + K] = True
    fin = np.isfinite(y.real) & np.isfinite(y.imag)
    assert np.array_equal(~fin, bad)
    # everywhere else the clean stream's result (the windows of those outputs hold no bad sample)
    rms = np.sqrt(np.mean(np.abs(t) ** 2))
    assert np.max(np.abs(y[~bad] - t[~bad]) / np.maximum(np.abs(t[~bad]), rms)) <= TOL
    assert 2 <= _marked(G, f) <= 4  # the segments whose windows hold them


@pytest.mark.parametrize("K,D", [(64, 1), (5, 1), (64, 2)])
def test_buffers_aligned_to_8_bytes_only(G, K, D):
    tile = G.complex_fir_filter.tile()
    n = D * (2 * tile + 37)
    b, x = taps(K, D), signal(n, 41 + K)
    t, _ = CO.cfir64(b, x, D)
    _seq_ok(b, x, D, t)
    xin = torch.zeros(n + 1, dtype=torch.complex64, device="cuda")
    xin[1:] = _dev(x)
    out = torch.full((n // D + 2,), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    assert xin[1:].data_ptr() % 16 == 8 and out[1:].data_ptr() % 16 == 8
    f = G.complex_fir_filter(b, D)
    G.capi.check(G.capi.lib().gr4hip_cfir_process(f._h, xin[1:].data_ptr(), n, out[1:].data_ptr(), None, torch.cuda.current_stream().cuda_stream), "process")
    assert _marked(G, f) == 0
    o = out.cpu().numpy()
    assert o[0] == 7 + 7j and o[-1] == 7 + 7j and _rel(o[1:-1], t) <= TOL
    # 4-byte alignment is refused
    rc = G.capi.lib().gr4hip_cfir_process(f._h, xin.data_ptr() + 4, n, out.data_ptr(), None, None)
    assert rc == G.capi.INVALID_ARGUMENT and b"aligned" in G.capi.lib().gr4hip_last_error()


def test_translating_decimator(G):
    """taps h[k] e^{j w k}, decimate by 8, Rotator at the OUTPUT rate  ==  Rotator at the input rate -> real-tap decimating fir_filter<complex>"""
    K, D, n = 128, 8, 1 << 16
    w = np.float32(2 * np.pi * 0.2)
    h = O.design_taps_hamming_lowpass(K, 0.4 / (2 * D))
    c = (h.astype(np.float64) * np.exp(1j * float(w) * np.arange(K))).astype(np.complex64)
    x = signal(n, 55, tone=0.21)
    m, i = np.arange(n // D), np.arange(n)
    # float64 evaluation of each chain of blocks (Rotator: phase of sample i = initial + (i + 1) increment)
    t_old = CO.cfir64(h.astype(np.complex128), x.astype(np.complex128) * np.exp(-1j * float(w) * (i + 1)), D)[0]
    inc8, ph0 = np.float32(-8) * w, np.float32(7) * w
    t_new = CO.cfir64(c, x, D)[0] * np.exp(1j * (float(ph0) + (m + 1) * float(inc8)))
    assert _rel(t_new, t_old) <= 1e-6  # the two chains are the same filter up to the rounding of the shifted taps and of 7 w
    _seq_ok(c, x, D, CO.cfir64(c, x, D)[0])
    xd = _dev(x)
    y_old = G.fir_filter(h, torch.complex64, D).process_bulk(G.Rotator(phase_increment=float(-w)).process_bulk(xd)).cpu().numpy()
    f = G.complex_fir_filter(c, D)
    z = f.process_bulk(xd)
    assert _marked(G, f) == 0 and (_paths(G, f) & 1)
    y_new = G.Rotator(phase_increment=float(inc8), initial_phase=float(ph0)).process_bulk(z).cpu().numpy()
    print(f"old {_rel(y_old, t_old):.2e} new {_rel(y_new, t_new):.2e}")
    assert _rel(y_old, t_old) <= TOL and _rel(y_new, t_new) <= TOL


def test_refusals(G):
    L = G.capi.lib()
    b = taps(33, 4)
    f = G.complex_fir_filter(b, 4)
    xh = signal(4096, 3)
    x = _dev(xh)
    out = torch.full((1024,), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    n_out = C.c_size_t(99)
    assert L.gr4hip_cfir_process(f._h, x.data_ptr(), 4095, out.data_ptr(), C.byref(n_out), st) == G.capi.INVALID_ARGUMENT
    assert b"multiple of decim" in L.gr4hip_last_error() and n_out.value == 99
    torch.cuda.synchronize()
    assert bool((out == 7.0 + 7.0j).all())  # the sentinel is untouched
    assert L.gr4hip_cfir_process(f._h, x.data_ptr(), 0, out.data_ptr(), C.byref(n_out), st) == 0 and n_out.value == 0
    assert L.gr4hip_cfir_process(f._h, None, 0, None, None, st) == 0  # nothing to read or write
    assert _marked(G, f) == 0 and _paths(G, f) == 0
    assert L.gr4hip_cfir_process(f._h, None, 8, out.data_ptr(), None, st) == G.capi.INVALID_ARGUMENT
    # overlapping buffers: in place, and the output's end inside the input
    assert L.gr4hip_cfir_process(f._h, x.data_ptr(), 4096, x.data_ptr(), None, st) == G.capi.INVALID_ARGUMENT and b"overlap" in L.gr4hip_last_error()
    assert L.gr4hip_cfir_process(f._h, x.data_ptr() + 8 * 1000, 3096, x.data_ptr() + 8 * 500, None, st) == G.capi.INVALID_ARGUMENT
    assert L.gr4hip_cfir_process(f._h, x.data_ptr() + 8 * 1024, 3072, x.data_ptr(), C.byref(n_out), st) == 0 and n_out.value == 768  # adjacent is fine
    torch.cuda.synchronize()
    assert bool((out == 7.0 + 7.0j).all())
    # the refused calls left the handle's state alone: that call was the first of its stream
    assert _rel(x[:768].cpu().numpy(), CO.cfir64(b, xh[1024:], 4)[0]) <= TOL


def test_device_graph(G):
    """the C++ host mirror on gpu:hip:0: source -> complex_fir_filter -> sink against its CPU body, alone and inside a hip::plan run behind a Rotator"""
    assert os.path.exists(BIN), "build() compiles host/tests/test_host_complex_fir.cpp"
    r = subprocess.run([BIN, "device", PLUGIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "complex_fir device: ok" in r.stdout
