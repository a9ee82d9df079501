"""Overlapped and skipped FFT frames on the device (gr4hip_stft_*, csrc/stft.hip, csrc/stft_kernels.hpp; OVERLAPPED_FFT.md) against the FFT block on the explicitly
materialised frames (value for value: the feature adds no arithmetic) and against the float64 oracle (tests/stft_oracle.py) under the parity contract's 1e-5
(include/gr4hip.h) with the relative measure of tests/test_gpu_pfb.py -- the FFT block's own bar, no margin over it.

Shapes: M = 2 FPB + 3 frames, FPB = 8192 / N frames per workgroup for N >= 256 (three workgroups, a ragged last one; 5 frames at 8192 and above), for N < 256
FPB = 64 / max(1, N / 8) as the run-time kernel groups them.  The input carries a tail of min(S, N) - 1 samples that must not yield a frame.  Native sizes run the
hop front end, gather sizes (N < 256, {2,3,5}-smooth, chirp, four-step, float32 input) the gather kernel in front of the FFT block's kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
import pfb_oracle as PO
import stft_oracle as SO

pytestmark = pytest.mark.gpu
TOL = 1e-5
GATHER = "GR4HIP_STFT_GATHER"
NATIVE_SIZES = [256, 1024, 4096, 8192]
GATHER_SIZES = [8, 64, 1000, 1009, 16384]


def native_strides(N):
    return ([1] if N == 256 else []) + [N // 4, N // 2, N - 1, N, N + 1, N + 3, 2 * N + 5]


NATIVE = [(N, S) for N in NATIVE_SIZES for S in native_strides(N)]
GATHERED = [(N, S) for N in GATHER_SIZES for S in ((N + 1) // 2, N, N + 3)]
REAL = [(64, 32), (64, 64), (64, 67), (1024, 512), (1024, 1024), (1024, 1027)]


def seam_gather_values(N):
    """csrc/stft.hip stft_seam_gather_values: a call with a seam and at most this many frames x points takes the gather path by default"""
    return 1 << 17 if N >= 8192 else 1 << 21


BIN = os.path.join(O.ROOT, "build", "host", "test_host_stft")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
HOP, GATHERED_ALL = 2, 1      # values of the switch: the hop kernels wherever they exist / the gather path everywhere


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


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


def n_frames(N):
    fpb = max(1, 8192 // N) if N >= 256 else 64 // max(1, N // 8)
    return 2 * fpb + 3


_inputs = {}


def signal(N, S, real=False):
    """M frames' worth of the oracle's signal plus a tail of min(S, N) - 1 samples: computed once, shared, never written to"""
    key = (N, S, real)
    if key not in _inputs:
        n = (n_frames(N) - 1) * S + N + min(S, N) - 1
        x = (O.signal_f32 if real else O.signal_c32)(1000 + N + S, n)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def materialise(xd, N, S, M):
    """[M, N]: the frames as contiguous memory, what a caller without the feature has to build"""
    idx = torch.from_numpy(SO.frame_index(M, N, S)).to(xd.device)
    return xd[idx].contiguous()


def last_path(G, st):
    fn = G.capi.lib().gr4hip_internal_stft_last_path  # (test hook, not in include/gr4hip.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]
    rec = (C.c_longlong * 4)(*([-1] * 4))
    assert fn(st._h, rec) == 0
    return tuple(rec)


def expect_path(native, off, n_in, N, S, piece_frames=None, hop_forced=False):
    """the dispatch rule restated: {frames the hop kernel reads from the input, frames it reads from the seam's staging span, gathered frames, launches}"""
    if n_in == 0:
        return (0, 0, 0, 0)
    k = SO.count(off, n_in, N, S)
    if native and not hop_forced and off < 0 and 0 < k * N <= seam_gather_values(N):
        native = False  # a short call with a seam: one launch fewer on the gather path
    if native:
        seam = min(k, -(off // S)) if off < 0 else 0  # ceil(-off / S) frames begin in the history
        return (k - seam, seam, 0, (2 if seam else 0) + (1 if k > seam else 0) + 1)  # staging + hop, hop, history carry
    pieces = 0 if k == 0 else -(-k // (piece_frames or k))
    return (0, 0, k, 2 * pieces + 1)  # per piece: gather + the FFT block's kernels; history carry


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))


def check_identity(G, N, S, window, real=False, **flags):
    x = signal(N, S, real)
    M = n_frames(N)
    dtype = torch.float32 if real else torch.complex64
    xd = dev(x)
    assert SO.n_frames_total(len(x), N, S) == M and SO.n_frames_total(len(x) + 1, N, S) == (M + 1 if S <= N else M)
    fr = materialise(xd, N, S, M)
    fft = G.FFT(N, window, dtype=dtype, **flags)
    st = G.STFT(N, S, window, dtype=dtype, **flags)
    assert st.pending(len(x)) == M
    got = st.spectrum(xd)
    assert same(got, fft.spectrum(fr)), "spectrum"
    st.reset()
    assert same(st.mag2(xd), fft.mag2(fr)), "|X|^2"
    st.reset()
    a, b = st.process_bulk(xd), fft.process_bulk(fr)
    for key in ("magnitude", "phase", "re", "im", "ranges"):
        assert same(a[key], b[key]), key
    assert np.array_equal(a["frequency"], b["frequency"]) and np.array_equal(a["time"], np.arange(M) * float(S))
    if S == N:  # back-to-back frames: the input itself is the materialised form
        assert same(got, fft.spectrum(xd[:M * N]))
    return got


@pytest.mark.parametrize("window", ["None", "Hann"])
@pytest.mark.parametrize("N,S", NATIVE + GATHERED)
def test_identity(G, N, S, window):
    check_identity(G, N, S, window)


@pytest.mark.parametrize("N,S", REAL)
def test_identity_real_input(G, N, S):
    check_identity(G, N, S, "Hann", real=True)


@pytest.mark.parametrize("flag", ["outputInDb", "outputInDeg", "unwrapPhase"])
@pytest.mark.parametrize("N,S,real", [(1024, 512, False), (64, 32, False), (64, 32, True)])
def test_identity_flags(G, N, S, real, flag):
    check_identity(G, N, S, "Hann", real=real, **{flag: True})


@pytest.mark.parametrize("N,S", NATIVE + GATHERED)
def test_parity(G, N, S):
    x = signal(N, S)
    t = SO.spectrum(x, N, S)
    st = G.STFT(N, S, "Hann")
    spec = host(st.spectrum(dev(x)))
    st.reset()
    mag2 = host(st.mag2(dev(x)))
    assert spec.shape == t.shape
    e_s, e_m = PO.rel(spec, t), PO.rel(mag2, np.abs(t) ** 2)
    print(f"N {N} S {S}: spectrum {e_s:.2e}, |X|^2 {e_m:.2e}")
    assert e_s <= TOL and e_m <= TOL


def run_cut(G, st, xd, sizes, N, S, native, hop_forced=False):
    """the stream in calls of the given sizes (the rest in one more): every call's frame count is what pending said and what the rule says, its record the rule's"""
    pos, outs, off = 0, [], 0
    for n in list(sizes) + [None]:
        n = len(xd) - pos if n is None else min(n, len(xd) - pos)
        want = st.pending(n)
        assert want == SO.count(off, n, N, S)
        y = st.spectrum(xd[pos:pos + n])
        assert y.shape == (want, N)
        assert last_path(G, st) == expect_path(native, off, n, N, S, hop_forced=hop_forced)
        outs.append(y)
        off += want * S - n
        pos += n
    return torch.cat(outs)


@pytest.mark.parametrize("N,S,real", [(N, S, False) for N, S in NATIVE + GATHERED] + [(N, S, True) for N, S in REAL])
def test_chunking(G, devsw, N, S, real):
    sizes = [0, 1, S - 1, S, N - 1, N, N + 1]
    n = sum(sizes) + N + 2 * S + min(S, N) - 1  # every cut, then a rest with frames of its own and a tail without
    xd = dev((O.signal_f32 if real else O.signal_c32)(2000 + N + S, n))
    native = (N, S) in NATIVE and not real
    st = G.STFT(N, S, "Hann", dtype=torch.float32 if real else torch.complex64)
    one = st.spectrum(xd)
    assert one.shape[0] == SO.n_frames_total(n, N, S)
    st.reset()
    cut = run_cut(G, st, xd, sizes, N, S, native)
    assert same(cut, one)
    if native:  # the same cuts with the seams on the hop kernels (the default sends these short calls to the gather path)
        devsw(GATHER, HOP)
        st.reset()
        assert same(run_cut(G, st, xd, sizes, N, S, native, hop_forced=True), one)
        devsw(GATHER, 0)
    if N in (8, 64):  # the first 2 N + 3 samples one at a time
        st.reset()
        assert same(run_cut(G, st, xd, [1] * (2 * N + 3), N, S, native), one)


@pytest.mark.parametrize("N,S", NATIVE)
def test_native_equals_gather(G, devsw, N, S):
    xd = dev(signal(N, S))
    M = n_frames(N)
    cutpoint = N + min(S, N) // 2 + 1  # two calls: one frame in the first, and the second one's first frames begin in the history where S < N
    res = {}
    for gather in (HOP, GATHERED_ALL, 0):
        devsw(GATHER, gather)
        st = G.STFT(N, S, "Hann")
        spec = torch.cat([st.spectrum(xd[:cutpoint]), st.spectrum(xd[cutpoint:])])
        rec = last_path(G, st)
        if gather:
            assert (rec[2] > 0) == (gather == GATHERED_ALL) and (rec[0] + rec[1] > 0) == (gather == HOP), rec
        st.reset()
        mag2 = torch.cat([st.mag2(xd[:cutpoint]), st.mag2(xd[cutpoint:])])
        st.reset()
        a = st.process_bulk(xd[:cutpoint])
        b = st.process_bulk(xd[cutpoint:])
        assert np.array_equal(np.concatenate([a["time"], b["time"]]), np.arange(M) * float(S))
        res[gather] = [spec, mag2] + [torch.cat([a[k], b[k]]) for k in ("magnitude", "phase", "re", "im", "ranges")]
    for other in (GATHERED_ALL, 0):
        for u, v in zip(res[HOP], res[other]):
            assert same(u, v) and u.shape[0] == M


def test_paths(G, devsw):
    """the record of what a call enqueued, exactly"""
    N, S = 1024, 256
    xd = dev(signal(N, S))
    st = G.STFT(N, S, "Hann")
    st.spectrum(xd[:N + 2 * S + 5])  # every frame lies in the input
    assert last_path(G, st) == (3, 0, 0, 2)
    off = 3 * S - (N + 2 * S + 5)    # = -(N - S + 5): the next frames begin in the history
    assert off == -773
    devsw(GATHER, HOP)                # the seam on the hop kernels (by default so short a call with a seam takes the gather path, below)
    st.spectrum(xd[N + 2 * S + 5:N + 2 * S + 5 + 2 * N])
    k = SO.count(off, 2 * N, N, S)
    assert k == 8 and last_path(G, st) == (k - 4, 4, 0, 4) == expect_path(True, off, 2 * N, N, S, hop_forced=True)  # ceil(773 / 256) = 4 seam frames
    off += k * S - 2 * N
    st.spectrum(xd[:3])              # too short for any frame: only the history moves
    assert last_path(G, st) == (0, 0, 0, 1) == expect_path(True, off, 3, N, S)
    st.reset()
    st.spectrum(xd[:S + 3])          # a call that ends inside the first frame, then one whose only frame is a seam frame
    assert last_path(G, st) == (0, 0, 0, 1)
    st.spectrum(xd[S + 3:N])
    assert last_path(G, st) == (0, 1, 0, 3) == expect_path(True, -(S + 3), N - S - 3, N, S, hop_forced=True)
    devsw(GATHER, 0)
    # the default: a call with a seam goes to the gather path up to seam_gather_values(N) frames x points, to the hop kernels beyond
    kbig = seam_gather_values(N) // N + 1
    big = dev(O.signal_c32(5, S + 3 + (kbig - 1) * S + N))
    for nk in (kbig - 1, kbig):
        st.reset()
        st.spectrum(big[:S + 3])
        n2 = (nk - 1) * S + N - (S + 3)
        assert st.pending(n2) == nk
        y = st.spectrum(big[S + 3:S + 3 + n2])
        want = (0, 0, nk, 3) if nk * N <= seam_gather_values(N) else (nk - 2, 2, 0, 4)  # ceil(259 / 256) = 2 seam frames
        assert last_path(G, st) == want == expect_path(True, -(S + 3), n2, N, S)
        st.reset()
        assert same(y, st.spectrum(big[:S + 3 + n2]))
    st.spectrum(xd[:0])              # an empty call enqueues nothing
    assert last_path(G, st) == (0, 0, 0, 0)
    # a gather size, and a native size under the switch
    g = G.STFT(1000, 500, "Hann")
    xg = dev(signal(1000, 500))
    g.mag2(xg)
    assert last_path(G, g) == (0, 0, n_frames(1000), 3)
    g.reset()
    g.process_bulk(xg[:7])
    assert last_path(G, g) == (0, 0, 0, 1)
    devsw(GATHER, 1)
    st.reset()
    st.spectrum(xd[:N + 2 * S + 5])
    assert last_path(G, st) == (0, 0, 3, 3)
    devsw(GATHER, 0)
    # a refused call enqueues nothing and leaves the stream where it was
    L, cap = G.capi.lib(), G.capi
    before = st.pending(5000)
    n = C.c_size_t(7)
    assert L.gr4hip_stft_spectrum(st._h, xd.data_ptr() + 4, 5000, xd.data_ptr(), C.byref(n), None) == cap.INVALID_ARGUMENT
    assert last_path(G, st) == (0, 0, 0, 0) and n.value == 0 and st.pending(5000) == before


@pytest.mark.parametrize("N,S", [(256, 64), (1024, 1027), (64, 32), (1000, 500)])
def test_reset_mid_stream(G, N, S):
    xd = dev(signal(N, S))
    st = G.STFT(N, S, "Hann")
    want = st.spectrum(xd)
    st.reset()
    st.spectrum(xd[:N + S + 3])  # leaves a history and an offset behind
    st.reset()
    assert st.pending(len(xd)) == n_frames(N)
    out = st.process_bulk(xd[:N])
    assert out["time"][0] == 0.0
    st.reset()
    assert same(st.spectrum(xd), want)


@pytest.mark.parametrize("A", [3, 40])
@pytest.mark.parametrize("N", [256, 1024])
def test_welch(G, N, A):
    S = N // 2
    K = 2 * A + 1  # two whole integrations and the first frame of a third; A = 40 crosses a leaf of 32 frames
    x = dev(O.signal_c32(77 + N + A, (K - 1) * S + N + S - 1))
    cutpoint = (A + 3) * S + 17  # A + 2 frames in the first call: the cut lies inside the second integration, and inside a frame
    st, si = G.STFT(N, S, "Hann"), G.SpectrumIntegrator(N, A)
    want = torch.cat([si.process_bulk(st.mag2(x[:cutpoint])), si.process_bulk(st.mag2(x[cutpoint:]))])
    st2, si2 = G.STFT(N, S, "Hann"), G.SpectrumIntegrator(N, A)
    got = torch.cat([st2.power_integrated(x[:cutpoint], si2), st2.power_integrated(x[cutpoint:], si2)])
    assert want.shape == (2, N) and same(got, want)
    # and in one call
    st2.reset()
    si2.reset()
    assert same(st2.power_integrated(x, si2), want)


@pytest.mark.parametrize("N,S", [(256, 64), (1024, 512), (1024, 1027), (8192, 4096), (64, 32), (1000, 1003)])
def test_non_finite_reach(G, N, S):
    x = np.array(signal(N, S))
    M = n_frames(N)
    clean = dev(x)
    st = G.STFT(N, S, "Hann")
    want = st.spectrum(clean)
    for i in (0, N - 1, N, (M // 2) * S + N // 3, len(x) - 1):
        bad = x.copy()
        bad[i] = np.nan
        hit = np.array([m * S <= i < m * S + N for m in range(M)])
        cutpoint = min(len(x), i + 2)  # the sample sits at the end of a call: it reaches the next call's frames through the history
        for sizes in ([len(x)], [cutpoint, len(x) - cutpoint]):
            st.reset()
            xd, pos, outs = dev(bad), 0, []
            for n in sizes:
                outs.append(st.spectrum(xd[pos:pos + n]))
                pos += n
            got = torch.cat(outs)
            fin = host(torch.isfinite(torch.view_as_real(got)).all(dim=2).all(dim=1))
            assert np.array_equal(~fin, hit), (i, sizes)
            keep = torch.from_numpy(~hit).cuda()
            assert same(got[keep], want[keep]), (i, sizes)


def test_refusals(G):
    L, cap = G.capi.lib(), G.capi
    s = torch.cuda.current_stream().cuda_stream
    N, S = 256, 64
    M = n_frames(N)
    x = dev(signal(N, S))
    n_in = len(x)

    def create(dtype, n, stride):
        hd = C.c_void_p()
        rc = L.gr4hip_stft_create(C.byref(hd), dtype, n, stride, 3, 0)
        assert (rc == 0) == bool(hd.value)
        if hd.value:
            L.gr4hip_stft_destroy(hd)
        return rc

    assert create(cap.C32, N, S) == cap.OK and create(cap.F32, N, S) == cap.OK and create(cap.C32, N, 0) == cap.OK
    assert create(cap.C32, N, 1 << 20) == cap.OK and create(cap.C32, N, (1 << 20) + 1) == cap.UNSUPPORTED
    assert create(cap.C32, 1 << 21, S) == cap.UNSUPPORTED and create(cap.C32, 600000, S) == cap.UNSUPPORTED  # the sizes gr4hip_fft_create refuses
    assert create(cap.C64, N, S) == cap.INVALID_ARGUMENT and create(cap.C32, 1, 1) == cap.INVALID_ARGUMENT
    hd = C.c_void_p()
    assert L.gr4hip_stft_create(C.byref(hd), cap.C32, N, S, 99, 0) == cap.INVALID_ARGUMENT and not hd.value  # the FFT block's window check

    st = G.STFT(N, S, "Hann")
    sent = 12345.0
    spec = torch.full((M * N + 8,), sent, dtype=torch.complex64, device="cuda")
    f = [torch.full((M * N + 8,), sent, dtype=torch.float32, device="cuda") for _ in range(5)]
    xp, sp = x.data_ptr(), spec.data_ptr()
    mp, pp, rp, ip, gp = (t.data_ptr() for t in f)
    k = C.c_size_t(0)
    kb = C.byref(k)
    huge = G.STFT(8, 1, "None")
    si = G.SpectrumIntegrator(N, 3)
    refused = [
        L.gr4hip_stft_spectrum(None, xp, n_in, sp, kb, s),
        L.gr4hip_stft_spectrum(st._h, xp, n_in, sp, None, s),
        L.gr4hip_stft_spectrum(st._h, None, n_in, sp, kb, s),
        L.gr4hip_stft_spectrum(st._h, xp, n_in, None, kb, s),
        L.gr4hip_stft_spectrum(st._h, xp, 5, None, kb, s),                   # every output null also where the call is too short for a frame
        L.gr4hip_stft_process(st._h, xp, 5, None, None, None, None, None, kb, s),
        L.gr4hip_stft_mag2(st._h, xp, n_in, None, kb, s),
        L.gr4hip_stft_process(st._h, xp, n_in, None, None, None, None, None, kb, s),
        L.gr4hip_stft_spectrum(st._h, xp + 4, n_in - 1, sp, kb, s),
        L.gr4hip_stft_spectrum(st._h, xp, n_in, sp + 4, kb, s),
        L.gr4hip_stft_mag2(st._h, xp, n_in, mp + 2, kb, s),
        L.gr4hip_stft_process(st._h, xp, n_in, mp, pp + 2, rp, ip, gp, kb, s),
        L.gr4hip_stft_process(st._h, xp, n_in, mp, pp, rp, ip, gp + 1, kb, s),
        L.gr4hip_stft_spectrum(st._h, xp, n_in, xp, kb, s),                  # the spectrum over the input
        L.gr4hip_stft_mag2(st._h, xp, n_in, xp + 8 * N, kb, s),              # |X|^2 inside the input
        L.gr4hip_stft_spectrum(st._h, sp + 8 * N, n_in, sp, kb, s),          # the input inside the spectrum
        L.gr4hip_stft_process(st._h, xp, n_in, mp, pp, rp, xp + 8 * (n_in - 1), gp, kb, s),  # one signal over the input's last sample
        L.gr4hip_stft_spectrum(st._h, xp, (1 << 40) + 1, sp, kb, s),         # more than 2^40 samples
        L.gr4hip_stft_spectrum(huge._h, xp, 1 << 38, sp, kb, s),             # 2^38 frames of 8 points: more than 2^40 values per output
        L.gr4hip_stft_mag2_integrate(None, si._h, xp, n_in, mp, kb, s),
        L.gr4hip_stft_mag2_integrate(st._h, None, xp, n_in, mp, kb, s),
        L.gr4hip_stft_mag2_integrate(st._h, si._h, None, n_in, mp, kb, s),
        L.gr4hip_stft_mag2_integrate(st._h, si._h, xp, n_in, None, kb, s),
        L.gr4hip_stft_mag2_integrate(st._h, si._h, xp + 4, n_in - 1, mp, kb, s),
        L.gr4hip_stft_mag2_integrate(st._h, si._h, xp, n_in, xp, kb, s),
        L.gr4hip_stft_mag2_integrate(st._h, G.SpectrumIntegrator(N // 2, 3)._h, xp, n_in, mp, kb, s),
        L.gr4hip_stft_reset(None),
        L.gr4hip_stft_pending(None, 5, kb),
        L.gr4hip_stft_pending(st._h, 5, None),
    ]
    assert refused == [cap.INVALID_ARGUMENT] * len(refused), refused
    assert last_path(G, st) == (0, 0, 0, 0) and last_path(G, huge) == (0, 0, 0, 0)
    k.value = 9
    assert L.gr4hip_stft_spectrum(st._h, xp, 0, sp, kb, s) == cap.OK and k.value == 0  # no samples: a no-op
    k.value = 9
    assert L.gr4hip_stft_process(st._h, None, 0, None, None, None, None, None, kb, s) == cap.OK and k.value == 0
    torch.cuda.synchronize()
    assert bool((spec == sent).all()) and all(bool((t == sent).all()) for t in f), "a refused call wrote to its outputs"
    # nothing above touched the handles' state: they still compute the first call of a fresh one
    assert same(st.spectrum(x), G.STFT(N, S, "Hann").spectrum(x)) and si.pending(3) == 1
    with pytest.raises(G.capi.Gr4HipError):
        st.spectrum(x.real.contiguous())  # float32 samples into a complex64 handle
    with pytest.raises(G.capi.Gr4HipError):
        G.STFT(N, S, dtype=torch.float64)


def test_8192_points_never_take_the_frame_pipeline(G, devsw):
    """256 frames of 8192 points in one call -- where gr4hip_fft_spectrum / gr4hip_fft_mag2 switch to the frame pipeline, which equals the block kernels to rounding
    only -- equal the same stream in two calls of 128 frames and the FFT block on the materialised frames, 128 at a time, bit for bit"""
    N, S, K = 8192, 4096, 256
    xd = dev(O.signal_c32(8192, (K - 1) * S + N))
    fft = G.FFT(N, "Hann")
    want_s, want_m = [], []
    for f0 in (0, K // 2):
        fr = materialise(xd[f0 * S:], N, S, K // 2)
        want_s.append(fft.spectrum(fr))
        want_m.append(fft.mag2(fr))
    want_s, want_m = torch.cat(want_s), torch.cat(want_m)
    cutpoint = (K // 2 - 1) * S + N
    for sw in (0, HOP, GATHERED_ALL):
        devsw(GATHER, sw)
        st = G.STFT(N, S, "Hann")
        assert st.pending(len(xd)) == K
        assert same(st.spectrum(xd), want_s)
        st.reset()
        assert same(st.mag2(xd), want_m)
        st.reset()
        assert st.pending(cutpoint) == K // 2
        assert same(torch.cat([st.mag2(xd[:cutpoint]), st.mag2(xd[cutpoint:])]), want_m)


def test_device_graph(G, tmp_path):
    """VectorSource -> PowerSpectrum{stride} (gpu:hip:0) -> VectorSink through the host layer, unplanned and planned (an active stride stays out of the runs), against
    the CPU path within the mirror's PowerSpectrum tolerance (EXPECTs of host/tests/test_host_stft.cpp) and against the C-ABI value for value; the same graph from
    YAML with `stride:` through the plugin"""
    assert os.path.exists(BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_stft.cpp and the plugin"
    prefix = str(tmp_path / "dev")
    r = subprocess.run([BIN, "device", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "stft device: ok" in r.stdout and "FAIL" not in r.stdout and "yaml: stride 64 -> 77 frames" in r.stdout
    for N in (64, 1024):
        x = np.fromfile(f"{prefix}.N{N}.in", np.float32).view(np.complex64)
        for S in (N // 2, N + 3, 0):
            got = np.fromfile(f"{prefix}.N{N}.S{S}.mag2.seam", np.float32).reshape(-1, N)
            want = host(G.STFT(N, S, "Hann").mag2(dev(x)))
            assert got.shape == want.shape and np.array_equal(got, want), (N, S)
