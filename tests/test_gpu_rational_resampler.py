"""The rational resampler on the device (gr4hip_resamp_*, csrc/fir_resamp.hip) against its float64 oracle (tests/rational_resampler_oracle.py): parity over rates, tap
counts and both data types, the global-tap and direct paths, chunking bit for bit, impulses bit for bit, the special cases M = 1 and L = 1 against the blocks that
already compute them, a long device-generated stream, settings, non-finite samples, refusals, alignment and the device graph.
TOL is the parity contract's 1e-5 (include/gr4hip.h); every parity test first shows on the CPU that the float32 sum in the kernel's order meets 3e-6 on its input."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
import rational_resampler_oracle as RO

pytestmark = pytest.mark.gpu
TOL = 1e-5
SEQ_TOL = 3e-6
_rel = RO.rel
BIN = os.path.join(O.ROOT, "build", "host", "test_host_rational_resampler")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
LDS_TAPS, GLOBAL_TAPS, DIRECT, WINDOW = 1, 2, 4, 8  # WINDOW: beside one of the first two, the register-window form (decimate <= 4)
SHAPES = [(1, 1), (2, 3), (3, 2), (3, 4), (5, 7), (7, 5), (4, 6), (8, 1), (1, 8), (16, 5), (147, 160), (160, 147)]
MAX_TAPS = 65536


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


def _paths(G, f):
    m = C.c_uint(0)
    fn = G.capi.lib().gr4hip_internal_resamp_last_paths  # (test hook, not in include/gr4hip.h)
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_uint)], C.c_int
    assert fn(f._h, C.byref(m)) == 0
    return m.value


def taps(K, L, M):
    """Hamming low-pass at 0.4 / max(L, M) of the L-times rate (short filters: random taps)"""
    if K < 8:
        return (np.random.default_rng(K).standard_normal(K) / K).astype(np.float32)
    return O.design_taps_hamming_lowpass(K, 0.4 / max(L, M))


def signal(n, seed, L=1, M=1):
    """unit complex noise plus a tone inside the pass band of taps(); its real part is the real stream of the same test"""
    rng = np.random.default_rng(seed)
    f = 0.21 * min(1.0, L / M)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0) + np.exp(2j * np.pi * f * np.arange(n))).astype(np.complex64)


def _dev(x):
    return torch.from_numpy(np.array(x)).cuda()  # (a copy: the shared references are read-only)


def _of(x, cplx):
    """the stream of a test in the wanted type (real taps: the real part of the complex oracle is the oracle of the real part)"""
    return x if cplx else np.ascontiguousarray(x.real)


@functools.lru_cache(maxsize=4)
def _reference(L, M, K, n, seed):
    """(taps, complex stream, float64 oracle, float32 sum in the kernel's order): computed once, shared by the real and the complex case, never modified"""
    b, x = taps(K, L, M), signal(n, seed, L, M)
    t, _ = RO.resamp64(b, x, L, M)
    s = RO.resamp32_seq(b, x, L, M)
    for a in (b, x, t, s):
        a.setflags(write=False)
    return b, x, t, s


def _seq_ok(s, t, cplx):
    e = _rel(_of(s, cplx), _of(t, cplx))
    assert e <= SEQ_TOL, f"the float32 sum in the kernel's order errs {e:.2e} on this input"


def _dtype(cplx):
    return torch.complex64 if cplx else torch.float32


def _tap_counts(L):
    return sorted({min(K, MAX_TAPS) for K in (1, L - 1, L, L + 1, 8 * L + 3) if K >= 1})


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("L,M,K", [(L, M, K) for L, M in SHAPES for K in _tap_counts(L)])
def test_parity_over_shapes(G, L, M, K, cplx):
    tile = G.rational_resampler.tile()
    n = M * (3 * tile + 37)
    b, x, t, s = _reference(L, M, K, n, 1000 * L + 10 * M + K)
    _seq_ok(s, t, cplx)
    f = G.rational_resampler(b, L, M, _dtype(cplx))
    y = f.process_bulk(_dev(_of(x, cplx))).cpu().numpy()
    e = _rel(y, _of(t, cplx))
    print(f"L {L} M {M} K {K} {'complex' if cplx else 'real'}: {e:.2e}")
    assert _paths(G, f) == LDS_TAPS | (WINDOW if M <= 4 else 0)  # both forms of the main kernel are in SHAPES
    assert y.shape == (n // M * L,) and e <= TOL


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("L,M,K", [(147, 160, 40000), (8, 3, 10400)])
def test_global_tap_path(G, L, M, K, cplx):
    """a tap table of 160 KB (41 KB at 8 / 3, the window form) does not fit beside the input stage: the kernel reads it through the L2"""
    n = M * (G.rational_resampler.tile() + 5)
    b, x, t, s = _reference(L, M, K, n, 4)
    _seq_ok(s, t, cplx)
    f = G.rational_resampler(b, L, M, _dtype(cplx))
    y = f.process_bulk(_dev(_of(x, cplx))).cpu().numpy()
    e = _rel(y, _of(t, cplx))
    print(f"global taps, L {L} M {M} {'complex' if cplx else 'real'}: {e:.2e}")
    assert _paths(G, f) == GLOBAL_TAPS | (WINDOW if M <= 4 else 0)
    assert e <= TOL


@pytest.mark.parametrize("cplx", [False, True])
def test_direct_path(G, cplx):
    """one cycle's span (M + Kp - 1 samples) past the LDS budget: one output per lane straight from global memory"""
    L, M, K = 1, 1024, 19600
    n = M * 40
    h = O.design_taps_hamming_lowpass(301, 0.4 / M)
    b = np.zeros(K, np.float32)
    b[:150], b[-151:] = h[:150], h[150:]  # the two halves of a short low-pass at either end of the branch: every index of the long window, a float32 sum of 301 terms
    x = signal(n, 5, L, M)
    t, _ = RO.resamp64(b, x, L, M)
    _seq_ok(RO.resamp32_seq(b, x, L, M), t, cplx)
    f = G.rational_resampler(b, L, M, _dtype(cplx))
    y = f.process_bulk(_dev(_of(x, cplx))).cpu().numpy()
    assert _paths(G, f) == DIRECT
    assert _rel(y, _of(t, cplx)) <= TOL
    cuts = [M * 3, M * 17]  # and the carried history (19599 samples) on that path: calls shorter than it
    f.reset()
    y2 = torch.cat([f.process_bulk(_dev(_of(x[a:z], cplx))) for a, z in zip([0] + list(np.cumsum(cuts)), list(np.cumsum(cuts)) + [n])]).cpu().numpy()
    assert np.array_equal(y2.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("L,M,K", [(3, 4, 96), (147, 160, 8 * 147 + 3), (16, 5, 1600), (1, 1, 700)])
def test_chunking_bit_for_bit(G, L, M, K, cplx):
    tile = G.rational_resampler.tile()
    Kp = -(-K // L)
    # an empty call, a single cycle, calls shorter than the history (Kp - 1 inputs), calls on both sides of a tile edge
    cuts = [0, M, M * (tile - 1), M, 0, M * max(1, (Kp - 1) // (2 * M)), M * max(1, (Kp - 1) // (3 * M)), M * (tile + 1), M * tile, M * 2]
    n = sum(cuts) + M * 77
    b, x, t, s = _reference(L, M, K, n, 77 + K)
    _seq_ok(s, t, cplx)
    xs = _of(x, cplx)
    f = G.rational_resampler(b, L, M, _dtype(cplx))
    y1 = f.process_bulk(_dev(xs)).cpu().numpy()
    f2 = G.rational_resampler(b, L, M, _dtype(cplx))
    parts, at = [], 0
    for c in cuts + [n - sum(cuts)]:
        parts.append(f2.process_bulk(_dev(xs[at:at + c])).cpu().numpy())
        assert parts[-1].shape == (c // M * L,)
        at += c
    y2 = np.concatenate(parts)
    assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32))  # one fixed order per output sum, whatever the cut
    assert _rel(y1, _of(t, cplx)) <= TOL


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("L,M", [(3, 4), (4, 6), (7, 5), (147, 160), (160, 147), (8, 1), (1, 8)])
def test_impulses_bit_for_bit(G, L, M, cplx):
    """products with 1 and 0 are exact: an impulse reads the branch taps back, which pins every index of the slot and tap tables"""
    tile = G.rational_resampler.tile()
    K = 5 * L + 2
    b = (0.5 + np.arange(K) / (2.0 * K)).astype(np.float32)
    n = M * (tile + 9)
    f = G.rational_resampler(b, L, M, _dtype(cplx))
    for i in sorted({0, 1, M - 1, M, M * tile - 1, M * tile}):
        for v in ((1.0, 1j) if cplx else (1.0,)):
            x = np.zeros(n, np.complex64 if cplx else np.float32)
            x[i] = v
            f.reset()
            y = f.process_bulk(_dev(x)).cpu().numpy()
            want = (RO.impulse_response(b, L, M, i, n) * np.complex64(v)).astype(x.dtype) if cplx else RO.impulse_response(b, L, M, i, n)
            assert np.array_equal(np.asarray(y).view(np.float32), want.view(np.float32) + np.float32(0)), (i, v)  # (+ 0: -0 of 0 * 1j products is 0 in the sum from 0)


@pytest.mark.parametrize("cplx", [False, True])
def test_decimate_one_is_the_interpolator(G, cplx):
    L, K, n = 8, 67, 5000
    b, x = taps(K, L, 1), _of(signal(n, 8, L, 1), cplx)
    t_i, _ = O.fir_interp(b, x, L)
    t_r, _ = RO.resamp64(b, x, L, 1)
    assert _rel(t_r, t_i) <= 1e-7  # the two oracles state one definition
    y_i = G.fir_interpolator(b, L, _dtype(cplx)).process_bulk(_dev(x)).cpu().numpy()
    y_r = G.rational_resampler(b, L, 1, _dtype(cplx)).process_bulk(_dev(x)).cpu().numpy()
    assert _rel(y_r, t_r) <= TOL and _rel(y_i, t_i) <= TOL and _rel(y_r, t_i) <= TOL and _rel(y_i, t_r) <= TOL


@pytest.mark.parametrize("cplx", [False, True])
def test_interpolate_one_is_the_decimating_fir(G, cplx):
    M, K = 8, 64
    n = M * 2000
    b, x = taps(K, 1, M), _of(signal(n, 9, 1, M), cplx)
    t_f = O.fir(b, x)[0][::M]
    t_r, _ = RO.resamp64(b, x, 1, M)
    assert _rel(t_r, t_f) <= 1e-7
    fir = G.fir_filter(b, _dtype(cplx), M)
    fir.set_algo(G.capi.FIR_EXACT_F32)  # the same class of arithmetic
    y_f = fir.process_bulk(_dev(x)).cpu().numpy()
    y_r = G.rational_resampler(b, 1, M, _dtype(cplx)).process_bulk(_dev(x)).cpu().numpy()
    assert _rel(y_r, t_r) <= TOL and _rel(y_f, t_f) <= TOL and _rel(y_r, t_f) <= TOL and _rel(y_f, t_r) <= TOL


def test_long_device_generated_stream(G):
    """2^22 inputs at 3 / 4 with 96 taps against every 4th output of fir_interpolator(3): two float32 evaluations of one sum, within 2e-6 of the peak (the bound of
    test_interpolating_fir_matrix_pipe_many_workgroups)"""
    L, M, K, n = 3, 4, 96, 1 << 22
    b = taps(K, L, M)
    x = G.synth_f32(n, 7)
    want = G.fir_interpolator(b, L).process_bulk(x)[::M]
    f = G.rational_resampler(b, L, M)
    y = f.process_bulk(x)
    assert _paths(G, f) == LDS_TAPS | WINDOW and y.shape == (n // M * L,) and want.shape == y.shape
    peak = float(want.abs().max())
    err = float((y - want).abs().max())
    print(f"long stream: max |difference| {err:.2e}, peak {peak:.2e}")
    assert peak > 0.1 and err <= 2e-6 * peak


@pytest.mark.parametrize("cplx", [False, True])
def test_reset_and_settings_changed_mid_stream(G, cplx):
    """set_taps keeps the carried inputs unless their buffer must grow (capacity max(32, bit_ceil(Kp)), replaced by zeros then); reset zeroes them"""
    L, M = 3, 4
    n = M * (G.rational_resampler.tile() + 50)
    xs = [_of(signal(n, 200 + i, L, M), cplx) for i in range(5)]
    b60, b300, b45, b200 = taps(60, L, M), taps(300, L, M), taps(45, L, M), taps(200, L, M)
    f = G.rational_resampler(b60, L, M, _dtype(cplx))
    run = lambda x: f.process_bulk(_dev(x)).cpu().numpy()  # noqa: E731
    assert _rel(run(xs[0]), RO.resamp64(b60, xs[0], L, M)[0]) <= TOL
    f.settings_changed(b300)  # Kp 100 > capacity 32: the buffer grows, its content is replaced
    assert _rel(run(xs[1]), RO.resamp64(b300, xs[1], L, M)[0]) <= TOL
    f.settings_changed(b45)   # shrinking keeps it
    assert _rel(run(xs[2]), RO.resamp64(b45, xs[2], L, M, xs[1])[0]) <= TOL
    f.settings_changed(b200)  # growing inside the capacity (128) keeps it
    t = RO.resamp64(b200, xs[3], L, M, xs[2])[0]
    assert _rel(run(xs[3]), t) <= TOL
    assert _rel(RO.resamp64(b200, xs[3], L, M)[0], t) > 1e-2  # (the history matters in this comparison)
    f.reset()
    assert _rel(run(xs[4]), RO.resamp64(b200, xs[4], L, M)[0]) <= TOL


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("L,M,K", [(3, 4, 96), (7, 5, 59), (147, 160, 1179)])
def test_non_finite_samples_reach_exactly_their_window(G, L, M, K, cplx):
    tile = G.rational_resampler.tile()
    Kp = -(-K // L)
    n = M * (2 * tile + 37)
    b, x = taps(K, L, M), _of(signal(n, 31 + L, L, M), cplx)
    clean = x.copy()
    p0, p1 = M * tile - 1, M * (tile + 20) + 1  # the last input of a tile; inside the next
    x[p0], x[p1] = np.inf, np.nan
    t, _ = RO.resamp64(b, clean, L, M)
    y = G.rational_resampler(b, L, M, _dtype(cplx)).process_bulk(_dev(x)).cpu().numpy()
    o, _ = RO.slots(L, M)
    top = (np.arange(n // M)[:, None] * M + o[None, :]).ravel()  # c M + o_p of output c L + p
    bad = np.zeros(len(y), bool)
    for pos in (p0, p1):
        bad |= (top - Kp < pos) & (pos <= top)
    fin = np.isfinite(y.real) & np.isfinite(y.imag)
    assert np.array_equal(~fin, bad)  # (a zero-padded tap times Inf is NaN: every slot sums all Kp terms)
    rms = np.sqrt(np.mean(np.abs(t) ** 2))
    assert np.max(np.abs(y[~bad] - t[~bad]) / np.maximum(np.abs(t[~bad]), rms)) <= TOL


def test_refusals_leave_the_output_untouched(G):
    lib = G.capi.lib()
    L, M = 3, 4
    b = taps(33, L, M)
    f = G.rational_resampler(b, L, M, torch.complex64)
    xh = signal(4096, 3, L, M)
    x = _dev(xh)
    out = torch.full((3072,), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    n_out = C.c_size_t(99)
    INV = G.capi.INVALID_ARGUMENT
    assert lib.gr4hip_resamp_process(f._h, x.data_ptr(), 4095, out.data_ptr(), C.byref(n_out), st) == INV
    assert b"multiple of decim" in lib.gr4hip_last_error() and n_out.value == 99
    assert lib.gr4hip_resamp_process(None, x.data_ptr(), 4096, out.data_ptr(), None, st) == INV
    assert lib.gr4hip_resamp_process(f._h, None, 8, out.data_ptr(), None, st) == INV
    assert lib.gr4hip_resamp_process(f._h, x.data_ptr(), 8, None, None, st) == INV
    assert lib.gr4hip_resamp_process(f._h, x.data_ptr() + 4, 8, out.data_ptr(), None, st) == INV and b"aligned" in lib.gr4hip_last_error()
    assert lib.gr4hip_resamp_process(f._h, x.data_ptr(), 8, out.data_ptr() + 4, None, st) == INV
    # overlapping buffers: in place, and the output's end inside the input
    assert lib.gr4hip_resamp_process(f._h, x.data_ptr(), 4096, x.data_ptr(), None, st) == INV and b"overlap" in lib.gr4hip_last_error()
    assert lib.gr4hip_resamp_process(f._h, x.data_ptr() + 8 * 1000, 3096, x.data_ptr() + 8 * 500, None, st) == INV
    # set_taps: NULL, empty, non-finite
    bad = b.copy()
    bad[7] = np.nan
    assert lib.gr4hip_resamp_set_taps(f._h, None, 33) == INV and lib.gr4hip_resamp_set_taps(f._h, b.ctypes.data, 0) == INV
    assert lib.gr4hip_resamp_set_taps(f._h, bad.ctypes.data, 33) == INV and b"tap 7 is not finite" in lib.gr4hip_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0 + 7.0j).all())  # the sentinel is untouched
    assert lib.gr4hip_resamp_process(f._h, x.data_ptr(), 0, out.data_ptr(), C.byref(n_out), st) == 0 and n_out.value == 0
    assert lib.gr4hip_resamp_process(f._h, None, 0, None, None, st) == 0 and _paths(G, f) == 0  # nothing to read or write
    torch.cuda.synchronize()
    assert bool((out == 7.0 + 7.0j).all())
    # adjacent buffers are fine, and the refused calls left the handle's state alone: this call is the first of its stream
    assert lib.gr4hip_resamp_process(f._h, x.data_ptr() + 8 * 1752, 2336, x.data_ptr(), C.byref(n_out), st) == 0 and n_out.value == 1752  # the output ends where the input starts
    assert _rel(x[:1752].cpu().numpy(), RO.resamp64(b, xh[1752:1752 + 2336], L, M)[0]) <= TOL
    with pytest.raises(G.capi.Gr4HipError):
        f.process_bulk(_dev(xh.real.copy()))  # the handle's type


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("L,M,K", [(3, 4, 96), (147, 160, 1179)])
def test_views_offset_from_16_bytes(G, L, M, K, cplx):
    n = M * (G.rational_resampler.tile() + 37)
    b, xc, t, s = _reference(L, M, K, n, 41 + K)
    _seq_ok(s, t, cplx)
    x, dt, es = _of(xc, cplx), _dtype(cplx), 8 if cplx else 4
    fill = (7.0 + 7.0j) if cplx else 7.0
    xin = torch.zeros(n + 1, dtype=dt, device="cuda")
    xin[1:] = _dev(x)
    n_out = n // M * L
    out = torch.full((n_out + 2,), fill, dtype=dt, device="cuda")
    assert xin[1:].data_ptr() % 16 == es and out[1:].data_ptr() % 16 == es
    f = G.rational_resampler(b, L, M, dt)
    G.capi.check(G.capi.lib().gr4hip_resamp_process(f._h, xin[1:].data_ptr(), n, out[1:].data_ptr(), None, torch.cuda.current_stream().cuda_stream), "process")
    o = out.cpu().numpy()
    assert o[0] == fill and o[-1] == fill and _rel(o[1:-1], _of(t, cplx)) <= TOL


def test_device_graph(G):
    """the C++ host mirror on gpu:hip:0: VectorSource -> rational_resampler -> VectorSink against its CPU body, behind the compute_domain seam and as a hip::plan run"""
    assert os.path.exists(BIN), "build() compiles host/tests/test_host_rational_resampler.cpp"
    r = subprocess.run([BIN, "device", PLUGIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rational_resampler device: ok" in r.stdout
