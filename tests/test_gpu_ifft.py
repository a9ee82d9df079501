"""The inverse transform and the polyphase synthesis bank on the device (gr4hip_ifft_* / gr4hip_pfb_synth_*, csrc/ifft.hip, csrc/ifft_kernels.hpp) against their
float64 oracle (tests/synthesis_oracle.py): every kernel plan, the forward kernels' own arithmetic, scale, window, the packed complex-to-real form, the
reference's round trip, and the bank's sums value for value, its chunking, reset, new taps, non-finite reach and refusals.  TOL is the parity contract's 1e-5
(include/gr4hip.h).

Shapes: N = 2, 8 and 64 run the LDS kernel (one and several lanes per frame), 256 / 1024 / 4096 / 8192 one fast-kernel plan each (no third pass, R3 < 16,
R3 = 16, the extra radix-2).  2 FPB + 3 frames (FPB frames per workgroup) make three workgroups with a ragged last one; the bank gets at least P + 3 frames, so
that its sums lie wholly in the history, across it, and wholly in the call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
import pfb_oracle as PO
import synthesis_oracle as SO

pytestmark = pytest.mark.gpu
TOL = 1e-5
BACK_TOL = 1e-6
SIZES = [2, 8, 64, 256, 1024, 4096, 8192]
BANK_SHAPES = [(N, P) for N in (8, 64, 256, 1024, 8192) for P in (1, 2, 3, 8, 32)]
BIN = os.path.join(O.ROOT, "build", "host", "test_host_ifft")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


def n_frames(N, P=1):
    fpb = max(1, 8192 // N) if N >= 256 else 64 // max(1, N // 8)
    return max(2 * fpb + 3, P + 3)


def signal(n, seed):
    """unit complex noise plus a tone of amplitude 4 at 0.2137 fs (the input of tests/test_gpu_pfb.py, here read as spectra)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0) + 4.0 * np.exp(2j * np.pi * 0.2137 * np.arange(n))
    return x.astype(np.complex64)


_spectra, _banks = {}, {}


def spectra(N):
    """the frames of one size and their float64 transforms: computed once, shared by the tests, never written to"""
    if N not in _spectra:
        X = signal(n_frames(N) * N, 77 + N).reshape(-1, N)
        c2c, c2r = SO.ifft_c2c(X, N), SO.ifft_c2r(X, N)
        for a in (X, c2c, c2r):
            a.setflags(write=False)
        _spectra[N] = (X, c2c, c2r)
    return _spectra[N]


def bank_case(N, P):
    if (N, P) not in _banks:
        g = PO.design(N, P, "Hamming")
        Y = signal(n_frames(N, P) * N, 1000 * P + N).reshape(-1, N)
        t = SO.synth(g, Y, N, P)
        for a in (g, Y, t):
            a.setflags(write=False)
        _banks[(N, P)] = (g, Y, t)
    return _banks[(N, P)]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared cases are read-only)


def host(t):
    return t.cpu().numpy()


def window(G, name, N):
    w = np.empty(N, np.float32)
    assert G.capi.lib().gr4hip_window_create(G.capi.WINDOWS.index(name), w.ctypes.data, N, 1.6) == 0
    return w


@pytest.mark.parametrize("N", SIZES)
def test_parity(G, N):
    X, c2c, c2r = spectra(N)
    got_c, got_r = host(G.InverseFFT(N).process_bulk(dev(X))), host(G.InverseFFT(N, torch.float32).process_bulk(dev(X)))
    assert got_c.shape == c2c.shape and got_c.dtype == np.complex64 and got_r.shape == c2r.shape and got_r.dtype == np.float32
    e_c, e_r = SO.rel(got_c, c2c), SO.rel(got_r, c2r)
    print(f"N {N}: C2C {e_c:.2e}, C2R {e_r:.2e}")
    assert e_c <= TOL and e_r <= TOL


@pytest.mark.parametrize("N", SIZES)
def test_shared_arithmetic_with_the_forward_transform(G, N):
    """no window, no scale: conj(forward(conj X)) of the FFT block, value for value (fewer than 256 frames: the forward entry runs its own kernel at 8192 too)"""
    X, _, _ = spectra(N)
    assert len(X) < 256
    want = np.conj(host(G.FFT(N, "None").spectrum(dev(np.conj(X)))))
    assert np.array_equal(host(G.InverseFFT(N).process_bulk(dev(X))), want)


@pytest.mark.parametrize("N", SIZES)
def test_scale_and_window(G, N):
    X, _, _ = spectra(N)
    xd = dev(X)
    w = window(G, "Hann", N)
    for dtype in (torch.complex64, torch.float32):
        plain = host(G.InverseFFT(N, dtype).process_bulk(xd))
        scaled = host(G.InverseFFT(N, dtype, scale=True).process_bulk(xd))
        assert np.array_equal(scaled, plain * np.float32(1.0 / N))
        assert np.array_equal(host(G.InverseFFT(N, dtype, window="Hann").process_bulk(xd)), plain * w)
        assert np.array_equal(host(G.InverseFFT(N, dtype, window="Hann", scale=True).process_bulk(xd)), scaled * w)
        assert np.array_equal(host(G.InverseFFT(N, dtype, window="Rectangular").process_bulk(xd)), plain)


@pytest.mark.parametrize("N", SIZES)
def test_c2r_against_c2c(G, N):
    """the real parts of the C2C form on the explicitly Hermitian-expanded frames, value for value; what the C2R form ignores may hold anything"""
    X, _, _ = spectra(N)
    c2r = G.InverseFFT(N, torch.float32)
    got = host(c2r.process_bulk(dev(X)))
    assert np.array_equal(got, host(G.InverseFFT(N).process_bulk(dev(SO.hermitian(X, N)))).real)
    junk = np.array(X)
    junk[:, N // 2 + 1:] = np.nan
    junk.imag[:, 0] = np.nan
    junk.imag[:, N // 2] = np.nan
    assert np.array_equal(host(c2r.process_bulk(dev(junk))), got)


@pytest.mark.parametrize("N", [1024, 8192])
def test_round_trip(G, N):
    """the reference's forward -> backward round trip (qa_SimdFFT.cpp:122-185) at this project's tolerance"""
    x = signal(n_frames(N) * N, 5 + N)
    spec = G.FFT(N, "None").spectrum(dev(x))
    back = host(G.InverseFFT(N, scale=True).process_bulk(spec)).ravel()
    e = SO.rel(back, x.astype(np.complex128))
    print(f"N {N}: round trip {e:.2e}")
    assert e <= TOL


@pytest.mark.parametrize("N,P", BANK_SHAPES)
def test_bank_parity(G, N, P):
    g, Y, t = bank_case(N, P)
    e_back = SO.rel(SO.back_end_u32(g, SO.ifft_c2c(Y, N).astype(np.complex64), N, P), t)
    print(f"N {N} P {P}: exact transform + float32 sums {e_back:.2e}")
    assert e_back <= BACK_TOL
    bank = G.PolyphaseSynthesisBank(N, P)  # the library's own default design
    assert np.array_equal(G.design_pfb(N, P), g)
    got = host(bank.process_bulk(dev(Y)))
    assert got.shape == t.shape and got.dtype == np.complex64
    e = SO.rel(got, t)
    print(f"N {N} P {P}: bank {e:.2e}")
    assert e <= TOL
    # the sums alone, value for value, on the device's own transform: an error in one weak tap cannot hide in the transform's rounding
    V = host(G.InverseFFT(N).process_bulk(dev(Y)))
    assert np.array_equal(got, SO.back_end_u32(g, V, N, P))
    # 1 / N in the transform, before the sums: exact, so the scaled bank is the bank times 1 / N
    assert np.array_equal(host(G.PolyphaseSynthesisBank(N, P, scale=True).process_bulk(dev(Y))), got * np.float32(1.0 / N))


@pytest.mark.parametrize("N", [8, 64, 256, 1024, 8192])
def test_one_tap_per_channel_is_the_windowed_transform(G, N):
    _, Y, _ = bank_case(N, 1)
    yd = dev(Y)
    assert np.array_equal(host(G.PolyphaseSynthesisBank(N, 1, taps=window(G, "Hann", N)).process_bulk(yd)), host(G.InverseFFT(N, window="Hann").process_bulk(yd)))


@pytest.mark.parametrize("N,P", BANK_SHAPES)
def test_bank_chunking(G, N, P):
    """one call = calls of 1, 2, P - 2, P - 1 frames (where positive) and the rest, value for value: calls shorter than the history, several in a row"""
    g, Y, _ = bank_case(N, P)
    M = len(Y)
    yd = dev(Y)
    whole = host(G.PolyphaseSynthesisBank(N, P, taps=g).process_bulk(yd))
    bank, parts, at = G.PolyphaseSynthesisBank(N, P, taps=g), [], 0
    for n in [c for c in (1, 2, P - 2, P - 1) if c > 0] + [M]:
        n = min(n, M - at)
        parts.append(host(bank.process_bulk(yd[at:at + n])))
        at += n
    assert at == M
    got = np.concatenate(parts)
    assert got.shape == whole.shape and np.array_equal(got, whole)
    # an output that is only 8-byte aligned takes the narrower stores: the same values
    buf = torch.empty(M * N + 1, dtype=torch.complex64, device="cuda")
    assert buf[1:].data_ptr() % 16 == 8
    assert np.array_equal(host(G.PolyphaseSynthesisBank(N, P, taps=g).process_bulk(yd, out=buf[1:])[:M * N]).reshape(M, N), whole)


@pytest.mark.parametrize("N,P", [(8, 3), (64, 32), (256, 2), (1024, 8), (8192, 2)])
def test_bank_reset_and_set_taps(G, N, P):
    g, Y, t = bank_case(N, P)
    g2 = PO.design(N, P, "Hann")
    yd = dev(Y)
    bank = G.PolyphaseSynthesisBank(N, P, taps=g)
    first = host(bank.process_bulk(yd))
    carried = host(bank.process_bulk(yd))
    bank.reset()
    again = host(bank.process_bulk(yd))
    assert SO.rel(first, t) <= TOL  # (the oracle starts from zeros)
    assert np.array_equal(again, first)
    assert not np.array_equal(carried[:P - 1], first[:P - 1]) and np.array_equal(carried[P - 1:], first[P - 1:])
    assert SO.rel(carried, SO.synth(g, Y, N, P, history=Y)) <= TOL
    # new taps, old history: the second call's first P - 1 frames mix the new prototype with the first call's transformed frames
    bank.set_taps(g2)
    swapped = host(bank.process_bulk(yd))
    assert SO.rel(swapped, SO.synth(g2, Y, N, P, history=Y)) <= TOL
    other = G.PolyphaseSynthesisBank(N, P, taps=g2)
    other.process_bulk(yd)
    assert np.array_equal(host(other.process_bulk(yd)), swapped)  # (the history does not depend on the taps)
    with pytest.raises(G.capi.Gr4HipError) as e:
        bank.set_taps(g2[:-1])
    assert e.value.status == G.capi.INVALID_ARGUMENT


@pytest.mark.parametrize("N,P", [(8, 3), (64, 2), (256, 32), (1024, 3), (8192, 1), (8192, 8)])
def test_bank_non_finite_reach(G, N, P):
    """one NaN in frame m: exactly frames m .. m + P - 1 are non-finite, in every sample; every other frame is the run without it"""
    g, Y, _ = bank_case(N, P)
    M = len(Y)
    clean = host(G.PolyphaseSynthesisBank(N, P, taps=g).process_bulk(dev(Y)))
    for frame, cut in ((1, 0), (M - P - 1, 0), (1, 2)):  # cut > 0: the NaN arrives in the call before
        bad = np.array(Y)
        bad[frame, (3 * N) // 4 + 1] = np.nan
        bank = G.PolyphaseSynthesisBank(N, P, taps=g)
        got = np.concatenate([host(bank.process_bulk(dev(bad[:cut]))), host(bank.process_bulk(dev(bad[cut:])))]) if cut else host(bank.process_bulk(dev(bad)))
        hit = np.zeros(M, bool)
        hit[frame:frame + P] = True
        assert not np.isfinite(got[hit]).any(), (N, P, frame, cut)  # (a sample is finite when both components are)
        assert np.array_equal(got[~hit], clean[~hit]), (N, P, frame, cut)


def test_refusals(G):
    L, cap = G.capi.lib(), G.capi
    st = torch.cuda.current_stream().cuda_stream
    N, P, M = 256, 4, 6
    g = PO.design(N, P)
    gp = g.ctypes.data

    def create_ifft(dtype, n, win=0, flags=0):
        hd = C.c_void_p()
        rc = L.gr4hip_ifft_create(C.byref(hd), dtype, n, win, flags)
        assert (rc == 0) == bool(hd.value)
        if hd.value:
            L.gr4hip_ifft_destroy(hd)
        return rc

    def create_bank(n, p, taps, flags=0):
        hd = C.c_void_p()
        rc = L.gr4hip_pfb_synth_create(C.byref(hd), n, p, taps, flags)
        assert (rc == 0) == bool(hd.value)
        if hd.value:
            L.gr4hip_pfb_synth_destroy(hd)
        return rc

    assert create_ifft(cap.C32, N) == cap.OK and create_ifft(cap.F32, N, 3, cap.IFFT_SCALE) == cap.OK and create_bank(N, P, gp, cap.IFFT_SCALE) == cap.OK
    assert L.gr4hip_ifft_create(None, cap.C32, N, 0, 0) == cap.INVALID_ARGUMENT
    assert L.gr4hip_pfb_synth_create(None, N, P, gp, 0) == cap.INVALID_ARGUMENT
    for bad in (create_ifft(cap.F64, N), create_ifft(cap.C64, N), create_ifft(cap.C32, 1), create_ifft(cap.C32, 0), create_ifft(cap.C32, N, 0, 2), create_ifft(cap.C32, N, 99),
                create_bank(1, P, gp), create_bank(0, P, gp), create_bank(N, 0, gp), create_bank(N, P, gp, 2)):
        assert bad == cap.INVALID_ARGUMENT
    for v in (np.nan, np.inf):
        bad = g.copy()
        bad[5] = v
        assert create_bank(N, P, bad.ctypes.data) == cap.INVALID_ARGUMENT
    for n in (16384, 1000, 768):  # gr4hip_fft_plan kinds 1, 2, 3
        kind, rad, npass = C.c_int(-1), (C.c_int * 16)(), C.c_int(0)
        assert L.gr4hip_fft_plan(n, C.byref(kind), rad, C.byref(npass)) == 0 and kind.value != 0
        assert create_ifft(cap.C32, n) == cap.UNSUPPORTED and create_ifft(cap.F32, n) == cap.UNSUPPORTED
        assert create_bank(n, 2, np.ones(n * 2, np.float32).ctypes.data) == cap.UNSUPPORTED
    assert create_bank(N, 33, np.ones(N * 33, np.float32).ctypes.data) == cap.UNSUPPORTED

    c2c, c2r, bank = G.InverseFFT(N), G.InverseFFT(N, torch.float32), G.PolyphaseSynthesisBank(N, P, taps=g)
    x = dev(signal(M * N + 8, 5))
    sent = 12345.0
    outc = torch.full((M * N + 8,), sent, dtype=torch.complex64, device="cuda")
    outr = torch.full((M * N + 8,), sent, dtype=torch.float32, device="cuda")
    xp, cp, rp = x.data_ptr(), outc.data_ptr(), outr.data_ptr()
    bad = g.copy()
    bad[-1] = np.nan
    refused = [
        L.gr4hip_ifft_process(None, xp, M, cp, st),
        L.gr4hip_ifft_process(c2c._h, None, M, cp, st),
        L.gr4hip_ifft_process(c2c._h, xp, M, None, st),
        L.gr4hip_ifft_process(c2c._h, xp + 4, M, cp, st),
        L.gr4hip_ifft_process(c2c._h, xp, M, cp + 4, st),
        L.gr4hip_ifft_process(c2r._h, xp, M, rp + 2, st),
        L.gr4hip_ifft_process(c2c._h, xp, M, xp, st),                 # in place
        L.gr4hip_ifft_process(c2c._h, xp, M, xp + 8 * N, st),         # the output inside the input
        L.gr4hip_ifft_process(c2r._h, cp + 8 * N, M, cp, st),         # the input inside the (real) output's span
        L.gr4hip_ifft_process(c2c._h, xp, (1 << 40) // N + 1, cp, st),
        L.gr4hip_pfb_synth_process(None, xp, M, cp, st),
        L.gr4hip_pfb_synth_process(bank._h, None, M, cp, st),
        L.gr4hip_pfb_synth_process(bank._h, xp, M, None, st),
        L.gr4hip_pfb_synth_process(bank._h, xp + 4, M, cp, st),
        L.gr4hip_pfb_synth_process(bank._h, xp, M, cp + 4, st),
        L.gr4hip_pfb_synth_process(bank._h, xp, M, xp, st),
        L.gr4hip_pfb_synth_process(bank._h, cp + 8 * N, M, cp, st),
        L.gr4hip_pfb_synth_process(bank._h, xp, (1 << 40) // N + 1, cp, st),
        L.gr4hip_pfb_synth_set_taps(bank._h, gp, N * P - 1),
        L.gr4hip_pfb_synth_set_taps(bank._h, gp, N * P + 1),
        L.gr4hip_pfb_synth_set_taps(bank._h, None, N * P),
        L.gr4hip_pfb_synth_set_taps(bank._h, bad.ctypes.data, N * P),
        L.gr4hip_pfb_synth_set_taps(None, gp, N * P),
        L.gr4hip_pfb_synth_reset(None),
    ]
    assert refused == [cap.INVALID_ARGUMENT] * len(refused), refused
    assert L.gr4hip_ifft_process(c2c._h, None, 0, None, st) == cap.OK  # no frames: a no-op
    assert L.gr4hip_pfb_synth_process(bank._h, None, 0, None, st) == cap.OK
    torch.cuda.synchronize()
    assert bool((outc == sent).all()) and bool((outr == sent).all()), "a refused call wrote to its outputs"
    # nothing above touched the bank's state: it still computes the first call of a fresh one
    want = host(G.PolyphaseSynthesisBank(N, P, taps=g).process_bulk(x[:M * N]))
    assert np.array_equal(host(bank.process_bulk(x[:M * N])), want)
    for blk in (c2c, bank):
        with pytest.raises(G.capi.Gr4HipError):
            blk.process_bulk(x[:M * N + 1])  # not whole frames
        with pytest.raises(G.capi.Gr4HipError):
            blk.process_bulk(x[:M * N].real.contiguous())  # not complex64
    with pytest.raises(G.capi.Gr4HipError):
        G.PolyphaseSynthesisBank(N, P, taps=g[:-1])
    with pytest.raises(G.capi.Gr4HipError):
        G.InverseFFT(N, torch.float64)


def test_device_graph(G):
    """VectorSource -> PfbChannelizer -> PfbSynthesizer -> VectorSink through the host layer: on gpu:hip:0 the planner makes one run of the two stages, and its
    output is the CPU graph's within the contract and the C-ABI's value for value; InverseFFT behind the compute_domain seam likewise"""
    assert os.path.exists(BIN), "build() compiles host/tests/test_host_ifft.cpp"
    out = os.path.join(O.ROOT, "build", "host", "ifft_device")
    r = subprocess.run([BIN, "device", PLUGIN, out], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ifft device: ok" in r.stdout
    assert "2 stage(s)" in r.stdout and "pfb_c32" in r.stdout and "pfb_synth_c32" in r.stdout
    N, P, M = 256, 4, 40  # the program's shape; its input is float32 pairs in <out>.in
    x = np.fromfile(out + ".in", np.float32).view(np.complex64)
    assert len(x) == M * N
    xd = dev(x)
    cpu = np.fromfile(out + ".bank.host", np.float32).view(np.complex64)
    planned = np.fromfile(out + ".bank.planned", np.float32).view(np.complex64)
    e = SO.rel(planned, cpu.astype(np.complex128))
    print(f"analysis -> synthesis, device run against the CPU graph: {e:.2e}")
    assert e <= TOL
    want = host(G.PolyphaseSynthesisBank(N, P, scale=True).process_bulk(G.PolyphaseFilterBank(N, P).process_bulk(xd))).ravel()
    assert np.array_equal(planned, want)
    assert np.array_equal(np.fromfile(out + ".c2c.seam", np.float32).view(np.complex64), host(G.InverseFFT(N, window="Hann", scale=True).process_bulk(xd)).ravel())
    assert np.array_equal(np.fromfile(out + ".c2r.seam", np.float32), host(G.InverseFFT(N, torch.float32, window="Hann", scale=True).process_bulk(xd)).ravel())
