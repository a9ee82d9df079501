"""The polyphase filter bank on the device (gr4hip_pfb_*, csrc/pfb.hip, csrc/pfb_kernels.hpp) against its float64 oracle (tests/pfb_oracle.py): every kernel plan
and both load paths of the front end, the FFT block's own values at one tap per channel, chunking, reset, new taps, non-finite samples, the refusals and the
host layer's device graph.  TOL is the parity contract's 1e-5 (include/gr4hip.h); every parity test first shows on the CPU that the float32 front end followed
by an exact transform meets 1e-6 on its input: what is compared is then the kernel, not the input's conditioning.

Shapes: N = 8 and 64 run the LDS kernel (one and several lanes per frame), 256 / 1024 / 4096 / 8192 one fast-kernel plan each (no third pass, R3 < 16, R3 = 16,
the extra radix-2).  2 FPB + 3 frames (FPB frames per workgroup) make three workgroups with a ragged last one; at least P + 3 frames, so that windows lie wholly
in the history, across it, and wholly in the input."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
import pfb_oracle as PO

pytestmark = pytest.mark.gpu
TOL = 1e-5
FRONT_TOL = 1e-6
SIZES = [8, 64, 256, 1024, 4096, 8192]
TAPS = [1, 2, 3, 4, 8, 32]
SHAPES = [(N, P) for N in SIZES for P in TAPS]
BIN = os.path.join(O.ROOT, "build", "host", "test_host_pfb")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


def n_frames(N, P):
    fpb = max(1, 8192 // N) if N >= 256 else 64 // max(1, N // 8)
    return max(2 * fpb + 3, P + 3)


def signal(n, seed):
    """unit complex noise plus a tone of amplitude 4 at 0.2137 fs"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0) + 4.0 * np.exp(2j * np.pi * 0.2137 * np.arange(n))
    return x.astype(np.complex64)


_cases = {}


def case(N, P):
    """prototype, input and float64 result of one shape: computed once, shared by the tests, never written to"""
    if (N, P) not in _cases:
        h = PO.design(N, P, "Hamming")
        x = signal(n_frames(N, P) * N, 1000 * P + N)
        t = PO.pfb(h, x, N, P)
        for a in (h, x, t):
            a.setflags(write=False)
        _cases[(N, P)] = (h, x, t)
    return _cases[(N, P)]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared cases are read-only)


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("N,P", SHAPES)
def test_parity(G, N, P):
    h, x, t = case(N, P)
    e_front = PO.rel(PO.front_end_f32(h, x, N, P), t)
    print(f"N {N} P {P}: float32 front end + exact transform {e_front:.2e}")
    assert e_front <= FRONT_TOL
    bank = G.PolyphaseFilterBank(N, P)  # the library's own default design
    assert np.array_equal(G.design_pfb(N, P), h)
    xd = dev(x)
    spec, mag2 = host(bank.process_bulk(xd)), None
    bank.reset()
    mag2 = host(bank.power(xd))
    assert spec.shape == t.shape and spec.dtype == np.complex64 and mag2.shape == t.shape and mag2.dtype == np.float32
    e_s, e_m = PO.rel(spec, t), PO.rel(mag2, np.abs(t) ** 2)
    print(f"N {N} P {P}: spectrum {e_s:.2e}, |X|^2 {e_m:.2e}")
    assert e_s <= TOL and e_m <= TOL
    # the front end alone, value for value: the FFT block (no window) on the float32 sums evaluated on the CPU is the bank's output.  (The 1e-5 above is mostly
    # the transform's error on the tone: an error in a weak tap would hide in it; not here.)
    u = dev(PO.front_end_u32(h, x, N, P))
    fft = G.FFT(N, "None")
    assert np.array_equal(host(fft.spectrum(u)), spec) and np.array_equal(host(fft.mag2(u)), mag2)
    # both outputs in one call are the values of the single-output calls
    L = G.capi.lib()
    bank.reset()
    s2, m2 = torch.empty(t.shape, dtype=torch.complex64, device="cuda"), torch.empty(t.shape, dtype=torch.float32, device="cuda")
    assert L.gr4hip_pfb_process(bank._h, xd.data_ptr(), len(t), s2.data_ptr(), m2.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert np.array_equal(host(s2), spec) and np.array_equal(host(m2), mag2)


@pytest.mark.parametrize("N", SIZES)
def test_one_tap_per_channel_is_the_fft_block(G, N):
    """h = the float Hann window: value for value gr4hip_fft_spectrum / gr4hip_fft_mag2 of a Hann FFT handle"""
    w = np.empty(N, np.float32)
    assert G.capi.lib().gr4hip_window_create(G.capi.WINDOWS.index("Hann"), w.ctypes.data, N, 1.6) == 0
    _, x, _ = case(N, 1)
    xd = dev(x)
    bank, fft = G.PolyphaseFilterBank(N, 1, taps=w), G.FFT(N, "Hann")
    assert np.array_equal(host(bank.process_bulk(xd)), host(fft.spectrum(xd)))
    assert np.array_equal(host(bank.power(xd)), host(fft.mag2(xd)))


@pytest.mark.parametrize("N,P", SHAPES)
def test_chunking(G, N, P):
    """one call = calls of 1, 2, P - 1 frames and the rest, value for value; for P >= 4 the first two are both shorter than the history (the shift, twice in a row)"""
    h, x, _ = case(N, P)
    M = len(x) // N
    xd = dev(x)
    for power in (False, True):
        run = (lambda b, v: b.power(v)) if power else (lambda b, v: b.process_bulk(v))
        whole = host(run(G.PolyphaseFilterBank(N, P, taps=h), xd))
        bank, parts, at = G.PolyphaseFilterBank(N, P, taps=h), [], 0
        for n in (1, 2, P - 1, M - (P + 2)):
            parts.append(host(run(bank, xd[at * N:(at + n) * N])))  # (P = 1: a call of 0 frames, a no-op)
            at += n
        assert at == M
        got = np.concatenate(parts)
        assert got.shape == whole.shape and np.array_equal(got, whole), (N, P, power)


@pytest.mark.parametrize("N,P", [(8, 3), (64, 32), (256, 4), (1024, 8), (8192, 2)])
def test_reset_and_first_frames(G, N, P):
    h, x, t = case(N, P)
    xd = dev(x)
    bank = G.PolyphaseFilterBank(N, P, taps=h)
    first = host(bank.process_bulk(xd))
    carried = host(bank.process_bulk(xd))
    bank.reset()
    again = host(bank.process_bulk(xd))
    assert PO.rel(first, t) <= TOL  # (the oracle starts from zeros)
    assert np.array_equal(again, first)
    assert not np.array_equal(carried[:P - 1], first[:P - 1]) and np.array_equal(carried[P - 1:], first[P - 1:])
    assert PO.rel(carried, PO.pfb(h, x, N, P, history=x)) <= TOL


@pytest.mark.parametrize("N,P", [(64, 4), (256, 3), (4096, 4), (8192, 8)])
def test_set_taps_mid_stream(G, N, P):
    h, x, _ = case(N, P)
    h2 = PO.design(N, P, "Hann")
    M = len(x) // N
    cut = (P - 1) * N if P > 2 else N  # the history of the second call is exactly the first one
    x1, x2 = dev(x[:cut]), dev(x[cut:])
    bank = G.PolyphaseFilterBank(N, P, taps=h)
    a = host(bank.process_bulk(x1))
    bank.set_taps(h2)
    b = host(bank.process_bulk(x2))
    assert PO.rel(a, PO.pfb(h, x[:cut], N, P)) <= TOL
    assert PO.rel(b, PO.pfb(h2, x[cut:], N, P, history=x[:cut])) <= TOL  # new taps, old samples
    other = G.PolyphaseFilterBank(N, P, taps=h2)
    other.process_bulk(x1)
    assert np.array_equal(host(other.process_bulk(x2)), b)
    assert len(a) + len(b) == M
    with pytest.raises(G.capi.Gr4HipError) as e:
        bank.set_taps(h2[:-1])
    assert e.value.status == G.capi.INVALID_ARGUMENT


@pytest.mark.parametrize("N,P", [(8, 4), (64, 2), (256, 32), (1024, 3), (4096, 1), (8192, 4)])
def test_non_finite_reach(G, N, P):
    """one NaN sample: exactly the P frames whose window holds it are non-finite, in every bin; every other frame is the run without it"""
    h, x, _ = case(N, P)
    M = len(x) // N
    clean_s = host(G.PolyphaseFilterBank(N, P, taps=h).process_bulk(dev(x)))
    clean_m = host(G.PolyphaseFilterBank(N, P, taps=h).power(dev(x)))
    for frame, cut in ((1, 0), (M - P - 1, 0), (1, 2)):  # cut > 0: the NaN arrives in the call before
        bad = x.copy()
        bad[frame * N + (3 * N) // 4 + 1] = np.nan
        for clean, power in ((clean_s, False), (clean_m, True)):
            bank = G.PolyphaseFilterBank(N, P, taps=h)
            run = bank.power if power else bank.process_bulk
            got = np.concatenate([host(run(dev(bad[:cut * N]))), host(run(dev(bad[cut * N:])))]) if cut else host(run(dev(bad)))
            hit = np.zeros(M, bool)
            hit[frame:frame + P] = True
            assert not np.isfinite(got[hit]).any(), (N, P, frame, cut, power)
            assert np.array_equal(got[~hit], clean[~hit]), (N, P, frame, cut, power)


def _run_length(G, bank, frames):
    fn = G.capi.lib().gr4hip_internal_pfb_set_run_length  # (test hook, not in include/gr4hip.h): frames per workgroup of the run form; 0 (the default): the simple form
    fn.argtypes, fn.restype = [C.c_void_p, C.c_long], C.c_int
    assert fn(bank._h, frames) == 0


def _took_run_form(G, bank):
    fn, v = G.capi.lib().gr4hip_internal_pfb_last_run_form, C.c_int(-1)
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_int)], C.c_int
    assert fn(bank._h, C.byref(v)) == 0
    return bool(v.value)


@pytest.mark.parametrize("P", [2, 3, 4])
def test_run_form_equals_the_simple_form(G, P):
    """N = 8192, P = 2 .. 4: a workgroup walks a run of frames with a register window.  Runs of 1 (every frame reads its predecessors again), 3 (a ragged last
    run), the whole call and longer than the call; the first run of a call reads the history: value for value the simple form, across two calls, NaN included."""
    N = 8192
    h, x, t = case(N, P)
    M = len(x) // N
    bad = x.copy()
    bad[2 * N - 5] = np.nan  # in frame 1, the last of the first call
    for sig in (x, bad):
        for power in (False, True):
            run = (lambda b, v: b.power(v)) if power else (lambda b, v: b.process_bulk(v))
            ref_bank = G.PolyphaseFilterBank(N, P, taps=h)
            ref = host(run(ref_bank, dev(sig)))
            assert not _took_run_form(G, ref_bank)
            for L in (1, 3, M, 100):
                bank = G.PolyphaseFilterBank(N, P, taps=h)
                _run_length(G, bank, L)
                got = np.concatenate([host(run(bank, dev(sig[:2 * N]))), host(run(bank, dev(sig[2 * N:])))])
                assert _took_run_form(G, bank)
                assert np.array_equal(got, ref, equal_nan=True), (P, L, power)
            if sig is x:
                assert PO.rel(ref, np.abs(t) ** 2 if power else t) <= TOL
            else:
                assert not np.isfinite(ref[1:1 + P]).any() and np.isfinite(ref[0]).all() and np.isfinite(ref[1 + P:]).all()


def test_run_form_is_taken_only_where_asked_for(G):
    """measured slower than the simple form (PFB.md), so a long call runs the simple form unless a run length is set; P = 8 does not have it"""
    N, P, M = 8192, 4, 300
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.view_as_complex(torch.randn(M * N, 2, device="cuda", generator=g))
    bank, run = G.PolyphaseFilterBank(N, P), G.PolyphaseFilterBank(N, P)
    _run_length(G, run, 64)  # 4 full runs and one of 44 frames
    want = bank.power(x)
    assert not _took_run_form(G, bank)
    assert torch.equal(run.power(x), want) and _took_run_form(G, run)
    other = G.PolyphaseFilterBank(N, 8)
    _run_length(G, other, 64)
    other.power(x[:64 * N])
    assert not _took_run_form(G, other)


def test_refusals(G):
    L, cap = G.capi.lib(), G.capi
    st = torch.cuda.current_stream().cuda_stream
    N, P, M = 256, 4, 6
    h = PO.design(N, P)
    hp = h.ctypes.data

    def create(dtype, n, p, taps):
        hd = C.c_void_p()
        rc = L.gr4hip_pfb_create(C.byref(hd), dtype, n, p, taps, 0)
        assert (rc == 0) == bool(hd.value)
        if hd.value:
            L.gr4hip_pfb_destroy(hd)
        return rc

    assert create(cap.C32, N, P, hp) == cap.OK
    assert L.gr4hip_pfb_create(None, cap.C32, N, P, hp, 0) == cap.INVALID_ARGUMENT
    assert create(cap.C32, 1, P, hp) == cap.INVALID_ARGUMENT
    assert create(cap.C32, 0, P, hp) == cap.INVALID_ARGUMENT
    assert create(cap.C32, N, 0, hp) == cap.INVALID_ARGUMENT
    for v in (np.nan, np.inf):
        bad = h.copy()
        bad[5] = v
        assert create(cap.C32, N, P, bad.ctypes.data) == cap.INVALID_ARGUMENT
    assert create(cap.F32, N, P, hp) == cap.UNSUPPORTED
    for n in (16384, 1000, 768):  # gr4hip_fft_plan kinds 1, 2, 3
        kind, rad, npass = C.c_int(-1), (C.c_int * 16)(), C.c_int(0)
        assert L.gr4hip_fft_plan(n, C.byref(kind), rad, C.byref(npass)) == 0 and kind.value != 0
        big = np.ones(n * 2, np.float32)
        assert create(cap.C32, n, 2, big.ctypes.data) == cap.UNSUPPORTED
    big = np.ones(N * 33, np.float32)
    assert create(cap.C32, N, 33, big.ctypes.data) == cap.UNSUPPORTED

    bank = G.PolyphaseFilterBank(N, P, taps=h)
    x = dev(signal(M * N + 8, 5))
    sent = 12345.0
    spec = torch.full((M * N + 8,), sent, dtype=torch.complex64, device="cuda")
    mag2 = torch.full((M * N + 8,), sent, dtype=torch.float32, device="cuda")
    xp, sp, mp = x.data_ptr(), spec.data_ptr(), mag2.data_ptr()
    bad = h.copy()
    bad[-1] = np.nan
    refused = [
        L.gr4hip_pfb_process(None, xp, M, sp, mp, st),
        L.gr4hip_pfb_process(bank._h, None, M, sp, mp, st),
        L.gr4hip_pfb_process(bank._h, xp, M, None, None, st),
        L.gr4hip_pfb_process(bank._h, xp + 4, M, sp, mp, st),
        L.gr4hip_pfb_process(bank._h, xp, M, sp + 4, mp, st),
        L.gr4hip_pfb_process(bank._h, xp, M, sp, mp + 2, st),
        L.gr4hip_pfb_process(bank._h, xp, M, xp, mp, st),              # the spectrum over the input
        L.gr4hip_pfb_process(bank._h, xp, M, sp, xp + 8 * N, st),      # |X|^2 inside the input
        L.gr4hip_pfb_process(bank._h, sp + 8 * N, M, sp, None, st),    # the input inside the spectrum
        L.gr4hip_pfb_set_taps(bank._h, hp, N * P - 1),
        L.gr4hip_pfb_set_taps(bank._h, hp, N * P + 1),
        L.gr4hip_pfb_set_taps(bank._h, None, N * P),
        L.gr4hip_pfb_set_taps(bank._h, bad.ctypes.data, N * P),
        L.gr4hip_pfb_set_taps(None, hp, N * P),
        L.gr4hip_pfb_reset(None),
    ]
    assert refused == [cap.INVALID_ARGUMENT] * len(refused), refused
    assert L.gr4hip_pfb_process(bank._h, xp, 0, sp, mp, st) == cap.OK   # no frames: a no-op
    assert L.gr4hip_pfb_process(bank._h, None, 0, None, None, st) == cap.OK
    torch.cuda.synchronize()
    assert bool((spec == sent).all()) and bool((mag2 == sent).all()), "a refused call wrote to its outputs"
    # nothing above touched the handle's state: it still computes the first call of a fresh one
    want = host(G.PolyphaseFilterBank(N, P, taps=h).process_bulk(x[:M * N]))
    assert np.array_equal(host(bank.process_bulk(x[:M * N])), want)
    with pytest.raises(G.capi.Gr4HipError):
        bank.process_bulk(x[:M * N + 1])  # not whole frames
    with pytest.raises(G.capi.Gr4HipError):
        G.PolyphaseFilterBank(N, P, taps=h[:-1])


def test_device_graph(G):
    """VectorSource -> PfbPowerSpectrum / PfbChannelizer (gpu:hip:0) -> VectorSink through the host layer: the planned run is one pfb stage and its output is the C-ABI's"""
    assert os.path.exists(BIN), "build() compiles host/tests/test_host_pfb.cpp"
    out = os.path.join(O.ROOT, "build", "host", "pfb_device")
    r = subprocess.run([BIN, "device", PLUGIN, out], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "1 stage(s): pfb_mag2_c32" in r.stdout and "1 stage(s): pfb_c32" in r.stdout
    N, P, M = 256, 4, 40  # the program's shape; its input is float32 pairs in <out>.in
    x = np.fromfile(out + ".in", np.float32).view(np.complex64)
    assert len(x) == M * N
    xd = dev(x)
    want_m = host(G.PolyphaseFilterBank(N, P).power(xd)).ravel()
    want_s = host(G.PolyphaseFilterBank(N, P).process_bulk(xd)).ravel()
    for tag in ("seam", "planned"):
        assert np.array_equal(np.fromfile(f"{out}.mag2.{tag}", np.float32), want_m), tag
        assert np.array_equal(np.fromfile(f"{out}.spec.{tag}", np.float32).view(np.complex64), want_s), tag
