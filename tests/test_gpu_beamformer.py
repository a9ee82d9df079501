"""The beamformer on the device (gr4hip_beamform_*; csrc/beamformer.hip) against its oracle (tests/beamformer_oracle.py).  Every comparison is uint32 equality
with the ordered definition: the streaming VALU form (S <= 8 with B <= 8), the matrix-pipe form (every shape), every output layout and every cut of the stream have
to land on the same bits.  Inputs are cross_spectrum_oracle.streams, weights complex Gaussian of variance 1 / S.  Every output is filled with a canary first, and
what lies behind the written region is checked untouched.

Shapes: (S, B) on both sides of a k-step (2 streams), of a row tile (8 beams), of the VALU form's limits and an odd S, at N = 64 and 35 frames; N = 2, 7, 8, 1028 at
(3, 5) (below one 16-bin tile, an odd row length, no multiple of the tile); 1, 15, 16, 17, 35 frames at (5, 3) (below, at and above a column tile of 16 frames)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import beamformer_oracle as BO
import cross_spectrum_oracle as XO
import oracle_lib as O

pytestmark = pytest.mark.gpu
CANARY = -77.25
HOST_BIN = os.path.join(O.ROOT, "build", "host", "test_host_beamformer")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
INV = -101


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    assert G.capi.INVALID_ARGUMENT == INV
    return G


_cases = {}


def case(S, B, N, frames):
    """(weights complex64 [B, S, N], input complex64 [S, frames, N], the ordered definition's beams [B, frames, N]): computed once, shared, read-only"""
    key = (S, B, N, frames)
    if key not in _cases:
        W = BO.weights(B, S, N, 100 * S + B)
        X = XO.streams(S, frames, N, 7 * S + B)
        Y = BO.beams_ordered(W, X)
        for a in (W, X, Y):
            a.setflags(write=False)
        _cases[key] = (W, X, Y)
    return _cases[key]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def has_valu(S, B):
    return S <= 8 and B <= 8


def stream():
    return torch.cuda.current_stream().cuda_stream


def set_path(G, blk, path):
    L = C.CDLL(G.capi.LIB_PATH)
    assert L.gr4hip_internal_beamform_set_path(blk._h, path) == 0


def last_path(G, blk):
    L = C.CDLL(G.capi.LIB_PATH)
    p = C.c_int(-1)
    assert L.gr4hip_internal_beamform_last_path(blk._h, C.byref(p)) == 0
    return p.value


def make(G, W, path=0, N=None):
    W = np.array(W)
    blk = G.Beamformer(W.shape[1], W.shape[0], W.shape[2] if N is None else N)
    if path:
        set_path(G, blk, path)
    blk.set_weights(W)
    return blk


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def run(G, W, X, path=0):
    """the voltage beams through the Python block, into a canary-filled tensor with one spare row"""
    B, (S, frames, N) = W.shape[0], X.shape
    blk = make(G, W, path)
    out = torch.full((B * frames * N + N,), CANARY, dtype=torch.complex64, device="cuda")
    got = blk.process_bulk(dev(X), out=out)
    assert got.shape == (B, frames, N)
    assert bool((out[B * frames * N:] == CANARY).all())
    return got.cpu().numpy(), last_path(G, blk)


@pytest.mark.parametrize("S,B", [(1, 1), (2, 1), (3, 5), (8, 4), (8, 5), (9, 4), (15, 16), (16, 17), (17, 8), (32, 32)])
def test_every_stream_and_beam_count_is_the_definition_bit_for_bit(G, S, B):
    W, X, want = case(S, B, 64, 35)
    got, path = run(G, W, X)
    assert path in (1, 2) and (path == 2 or has_valu(S, B)) and np.array_equal(u32(got), u32(want))
    mp, ran = run(G, W, X, path=2)
    assert ran == 2 and np.array_equal(u32(mp), u32(want))
    va, ran = run(G, W, X, path=1)  # where there is no VALU kernel the hook leaves the matrix pipe, and last_path says so
    assert ran == (1 if has_valu(S, B) else 2) and np.array_equal(u32(va), u32(mp))


@pytest.mark.parametrize("N", [2, 7, 8, 1028])
@pytest.mark.parametrize("path", [1, 2])
def test_every_kind_of_bin_count(G, N, path):
    W, X, want = case(3, 5, N, 35)
    got, ran = run(G, W, X, path=path)
    assert ran == path and np.array_equal(u32(got), u32(want))


@pytest.mark.parametrize("frames", [1, 15, 16, 17, 35])
@pytest.mark.parametrize("path", [1, 2])
def test_every_kind_of_frame_count(G, frames, path):
    W, X, want = case(5, 3, 64, frames)
    got, ran = run(G, W, X, path=path)
    assert ran == path and np.array_equal(u32(got), u32(want))


def raw_process(G, blk, ins, outs, frames, stride):
    a = (C.c_void_p * len(ins))(*ins)
    b = (C.c_void_p * len(outs))(*outs)
    return G.capi.lib().gr4hip_beamform_process(blk._h, a, frames, b, stride, stream())


@pytest.mark.parametrize("path", [1, 2])
def test_output_layouts(G, path):
    S, B, N, frames = 3, 5, 64, 17
    W, X, want = case(S, B, N, frames)
    blk = make(G, W, path)
    d = dev(X)
    ins = [d[s].data_ptr() for s in range(S)]
    # stride N: one dense stream per beam, here at scattered places of one buffer (every other slot)
    buf = torch.full((2 * B + 1, frames, N), CANARY, dtype=torch.complex64, device="cuda")
    assert raw_process(G, blk, ins, [buf[2 * b].data_ptr() for b in range(B)], frames, N) == 0
    h = buf.cpu().numpy()
    assert np.array_equal(u32(h[0:2 * B:2]), u32(want)) and np.all(h[1::2] == CANARY) and np.all(h[2 * B] == CANARY)
    # stride B N, d_beams[b] = base + b N: frames [f][b][c] in one buffer
    buf = torch.full((frames + 1, B, N), CANARY, dtype=torch.complex64, device="cuda")
    assert raw_process(G, blk, ins, [buf.data_ptr() + b * N * 8 for b in range(B)], frames, B * N) == 0
    h = buf.cpu().numpy()
    assert np.array_equal(u32(h[:frames]), u32(want.transpose(1, 0, 2))) and np.all(h[frames] == CANARY)
    # stride N + 3: the gap keeps its canary
    buf = torch.full((B, frames + 1, N + 3), CANARY, dtype=torch.complex64, device="cuda")
    assert raw_process(G, blk, ins, [buf[b].data_ptr() for b in range(B)], frames, N + 3) == 0
    h = buf.cpu().numpy()
    assert np.array_equal(u32(h[:, :frames, :N]), u32(want)) and np.all(h[:, :frames, N:] == CANARY) and np.all(h[:, frames] == CANARY)
    assert last_path(G, blk) == path


def integrate(G, blk, si, parts, B, N):
    """power_integrated over a list of cuts; a cut that completes nothing goes through the C-ABI with d_out NULL"""
    L = G.capi.lib()
    pieces = []
    for part in parts:
        n = part[0].shape[0]
        expect = si.pending(n)
        if expect == 0:
            ptrs = (C.c_void_p * len(part))(*[p.data_ptr() for p in part])
            got_n = C.c_size_t(99)
            assert L.gr4hip_beamform_power_integrate(blk._h, si._h, ptrs, n, None, C.byref(got_n), stream()) == 0 and got_n.value == 0
        else:
            out = torch.full((expect * B * N + N,), CANARY, dtype=torch.float32, device="cuda")
            got = blk.power_integrated(part, si, out=out)
            assert got.shape == (expect, B, N) and bool((out[expect * B * N:] == CANARY).all())
            pieces.append(got.cpu().numpy())
    return np.concatenate(pieces) if pieces else np.zeros((0, B, N), np.float32)


@pytest.mark.parametrize("A", [1, 31, 32, 70])
@pytest.mark.parametrize("path", [1, 2])
def test_cuts_do_not_change_a_bit_of_the_integrated_power(G, A, path):
    """5 A frames cut as (1, A - 1, 32, 33, rest), each cut clipped to what is left of the stream (A = 1 has 5 frames: cuts of 1, 0 and 4)"""
    S, B, N = 5, 3, 64
    W, X, Y = case(S, B, N, 5 * A)
    want = BO.power_integrated_ordered(W, X, A)
    d = dev(X)
    blk = make(G, W, path)
    si = G.SpectrumIntegrator(B * N, A)
    parts, at = [], 0
    for n in (1, A - 1, 32, 33, 5 * A):
        n = min(n, 5 * A - at)
        parts.append([d[s, at:at + n].contiguous() for s in range(S)])
        at += n
    assert at == 5 * A
    got = integrate(G, blk, si, parts, B, N)
    assert last_path(G, blk) == path
    assert got.shape == want.shape == (5, B, N) and np.array_equal(u32(got), u32(want))
    whole = integrate(G, blk, G.SpectrumIntegrator(B * N, A), [[d[s] for s in range(S)]], B, N)
    assert np.array_equal(u32(whole), u32(got))
    # the integrator block fed with |.|^2 (the fmaf form) of the device's own voltage output
    volt = blk.process_bulk(d).cpu().numpy()
    assert np.array_equal(u32(volt), u32(Y))
    p = BO.power(volt).reshape(5 * A, B * N)
    composed = G.SpectrumIntegrator(B * N, A).process_bulk(dev(p)).cpu().numpy().reshape(5, B, N)
    assert np.array_equal(u32(composed), u32(got))


@pytest.mark.parametrize("path", [1, 2])
def test_mean_mode_and_a_dropped_tail(G, path):
    S, B, N, A = 3, 5, 16, 33
    W, X, _ = case(S, B, N, 2 * A + 3)
    want = BO.power_integrated_ordered(W, X, A, mean=True)
    got = integrate(G, make(G, W, path), G.SpectrumIntegrator(B * N, A, mean=True), [[t for t in dev(X)]], B, N)
    assert got.shape == want.shape == (2, B, N) and np.array_equal(u32(got), u32(want))


@pytest.mark.parametrize("path", [1, 2])
def test_a_call_longer_than_one_piece_of_the_leaf_scratch(G, path):
    """the integrating entry is worked off in pieces of 2^25 / (n_bins max(S, B)) frames: only a size that large has more than one piece.  N = 2^18 with three beams
    makes a piece 42 frames: 50 frames are two pieces, the cut inside the second leaf of an integration of 33 frames"""
    S, B, N, A, frames, block = 1, 3, 1 << 18, 33, 50, 4096
    W, X = BO.weights(B, S, block, 3), XO.streams(S, frames, block, 5)
    want = BO.power_integrated_ordered(W, X, A)
    blk = make(G, np.tile(W, (1, 1, N // block)), path)  # the same 4096 bins 64 times over
    got = integrate(G, blk, G.SpectrumIntegrator(B * N, A), [[t for t in dev(np.tile(X, (1, 1, N // block)))]], B, N)
    assert last_path(G, blk) == path
    assert got.shape == (1, B, N) and np.array_equal(u32(got), u32(np.tile(want, (1, 1, N // block))))


@pytest.mark.parametrize("path", [1, 2])
def test_new_weights_apply_to_every_later_call_and_to_nothing_earlier(G, path):
    S, B, N, frames = 3, 5, 64, 17
    W, X, want = case(S, B, N, frames)
    W2 = BO.weights(B, S, N, 999)
    d = dev(X)
    blk = G.Beamformer(S, B, N)
    set_path(G, blk, path)
    with pytest.raises(G.capi.Gr4HipError):  # no weights yet
        blk.process_bulk(d)
    blk.set_weights(W)
    a = blk.process_bulk(d)  # (no synchronisation in between: the copy is stream-ordered)
    blk.set_weights(W2)
    b = blk.process_bulk(d)
    c = blk.process_bulk(d)
    assert np.array_equal(u32(a.cpu().numpy()), u32(want))
    want2 = BO.beams_ordered(W2, X)
    assert np.array_equal(u32(b.cpu().numpy()), u32(want2)) and np.array_equal(u32(c.cpu().numpy()), u32(want2))
    blk.set_weights(np.ascontiguousarray(W2[:, :, 0]))  # the short form: the same weight in every bin
    assert np.array_equal(u32(blk.process_bulk(d).cpu().numpy()), u32(BO.beams_ordered(W2[:, :, 0], X)))


@pytest.mark.parametrize("path", [1, 2])
def test_the_same_pointer_for_two_streams(G, path):
    W, X, _ = case(3, 5, 64, 17)
    want = BO.beams_ordered(W, np.stack([X[0], X[1], X[0]]))
    d = dev(X)
    a, b = d[0].contiguous(), d[1].contiguous()
    got = make(G, W, path).process_bulk([a, b, a]).cpu().numpy()
    assert np.array_equal(u32(got), u32(want))


@pytest.mark.parametrize("S,B,path", [(4, 3, 1), (4, 3, 2), (17, 8, 2)])
def test_a_nan_reaches_every_beam_in_its_frame_bin_and_integration_only(G, S, B, path):
    N, A = 64, 33
    W0, X0, clean = case(S, B, N, 2 * A + 3)
    W = np.array(W0)
    W[1, 2] = 0  # beam 1 ignores stream 2 -- but 0 NaN = NaN
    X = np.array(X0)
    clean = BO.beams_ordered(W, X)
    X[2, A + 7, 13] = np.nan  # stream 2, second integration, bin 13
    got, _ = run(G, W, X, path=path)
    hit = np.zeros(got.shape, bool)
    hit[:, A + 7, 13] = True
    assert np.all(np.isnan(got.real[hit])) and np.all(np.isnan(got.imag[hit]))
    assert np.array_equal(u32(got[~hit]), u32(clean[~hit]))
    power = integrate(G, make(G, W, path), G.SpectrumIntegrator(B * N, A), [[t for t in dev(X)]], B, N)
    want = BO.power_integrated_ordered(W, X0, A)
    hit = np.zeros(power.shape, bool)
    hit[1, :, 13] = True
    assert power.shape == (2, B, N) and np.all(np.isnan(power[hit])) and np.array_equal(u32(power[~hit]), u32(want[~hit]))


def test_refusals_leave_the_outputs_untouched(G):
    L = G.capi.lib()
    S, B, N, frames, A = 3, 2, 64, 8, 4
    W, X, _ = case(S, B, N, frames)
    blk = make(G, W)
    d = dev(X)
    ins = [d[s].data_ptr() for s in range(S)]
    buf = torch.full((B + 1, frames, N), CANARY, dtype=torch.complex64, device="cuda")
    outs = [buf[b].data_ptr() for b in range(B)]
    proc = lambda i, o, n=frames, stride=N: raw_process(G, blk, i, o, n, stride)
    assert L.gr4hip_beamform_process(blk._h, None, frames, (C.c_void_p * B)(*outs), N, stream()) == INV
    assert L.gr4hip_beamform_process(blk._h, (C.c_void_p * S)(*ins), frames, None, N, stream()) == INV
    assert proc([ins[0], None, ins[2]], outs) == INV and proc(ins, [outs[0], None]) == INV
    assert proc([ins[0], ins[1] + 4, ins[2]], outs) == INV and proc(ins, [outs[0], outs[1] + 4]) == INV  # not aligned to 8 bytes
    assert proc(ins, outs, stride=N - 1) == INV
    assert proc(ins, [outs[0], ins[2] + 64]) == INV and b"overlaps" in L.gr4hip_last_error()  # an output inside an input
    assert proc([ins[0], ins[1], outs[1] + 8], outs) == INV  # an input inside an output
    assert proc(ins, [outs[0], outs[0]]) == INV and proc(ins, [outs[0], outs[0] + 8 * (N - 1)]) == INV  # two beams that share rows
    assert proc(ins, [outs[0], outs[0] + 8 * N], stride=2 * N - 1) == INV  # interleaved rows, but the stride is one short of two rows
    assert proc(ins, outs, n=(1 << 40) // N + 1) == INV
    # the integrating entry
    si = G.SpectrumIntegrator(B * N, A)
    out = torch.full((3, B, N), CANARY, dtype=torch.float32, device="cuda")
    n = C.c_size_t(777)
    integ = lambda i, s, o, frames=frames, n_out=C.byref(n): L.gr4hip_beamform_power_integrate(blk._h, s, (C.c_void_p * S)(*i) if i else None, frames, o, n_out, stream())
    assert integ(ins, None, out.data_ptr()) == INV and integ(None, si._h, out.data_ptr()) == INV and integ(ins, si._h, out.data_ptr(), n_out=None) == INV
    assert integ([ins[0], None, ins[2]], si._h, out.data_ptr()) == INV and integ([ins[0], ins[1] + 4, ins[2]], si._h, out.data_ptr()) == INV
    assert integ(ins, si._h, None) == INV and b"completes 2" in L.gr4hip_last_error()  # 8 frames complete two integrations
    assert integ(ins, si._h, out.data_ptr() + 2) == INV  # the float output: 4 bytes
    assert integ(ins, si._h, ins[1] + 64) == INV and b"overlaps" in L.gr4hip_last_error()
    other = G.SpectrumIntegrator(B * N + 1, A)
    assert integ(ins, other._h, out.data_ptr()) == INV  # an integrator of another width
    assert integ(ins, si._h, out.data_ptr(), frames=(1 << 40) // N + 1) == INV
    assert n.value == 777 and si.pending(A) == 1  # nothing was counted
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and bool((out == CANARY).all())
    assert np.array_equal(d.cpu().numpy().view(np.uint32), u32(X))
    # and the accepted forms right behind them: interleaved rows at a stride of two rows, no frames
    assert proc(ins, [outs[0], outs[0] + 8 * N], n=4, stride=2 * N) == 0
    assert proc(ins, outs, n=0) == 0 and integ(ins, si._h, None, frames=0) == 0 and n.value == 0


def test_a_steered_beam_collects_the_tone_an_anti_steered_one_does_not(G):
    """the Python block fed from G.FFT(...).spectrum and Beamformer.delay_weights: plumbing, no threshold beyond the ordering"""
    N, A, tone, delay = 256, 8, 37, 3
    rng = np.random.default_rng(4)
    t = np.arange(N * A)
    noise = lambda: 0.1 * (rng.standard_normal(N * A) + 1j * rng.standard_normal(N * A))
    x = [(np.exp(2j * np.pi * tone / N * (t - k * delay)) + noise()).astype(np.complex64) for k in range(2)]  # stream 1 lags stream 0 by three samples
    fft = G.FFT(N, "None")
    spectra = [fft.spectrum(torch.from_numpy(v).cuda()) for v in x]
    freqs = np.arange(N) / N  # cycles per sample
    steer = [0.0, -float(delay)]  # advance stream 1 by its lag
    anti = [0.0, -float(delay) + N / (2.0 * tone)]  # half a period of the tone further: the two cancel
    w = G.Beamformer.delay_weights([steer, anti], freqs)
    assert w.shape == (2, 2, N)
    blk = G.Beamformer(2, 2, N)
    blk.set_weights(w)
    y = blk.process_bulk(spectra)
    assert y.shape == (2, A, N)
    p = blk.power_integrated(spectra, G.SpectrumIntegrator(2 * N, A)).cpu().numpy()
    assert p.shape == (1, 2, N)
    at = int(np.argmax(p[0, 0]))  # the tone's bin, whichever order the spectrum comes in
    assert p[0, 0, at] > p[0, 1, at]


def test_the_host_block_on_the_device_is_the_definition(tmp_path):
    """gr::blocks::fft::Beamformer<float> behind compute_domain gpu:hip:0: the seam onto gr4hip_beamform_process (gr4/hip.hpp)"""
    prefix = str(tmp_path / "dev")
    r = subprocess.run([HOST_BIN, "device", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "beamformer device: ok" in r.stdout
    assert "weights again with the handle kept (new weights by settings): 64 values, device == host" in r.stdout  # new weights between two work() calls
    for S, B, N in ((1, 1, 8), (3, 5, 16), (9, 2, 8)):
        for form in ("full", "short"):
            tag = f"{prefix}.S{S}.B{B}.N{N}.{form}"
            X = np.fromfile(tag + ".in", np.complex64).reshape(S, -1, N)
            W = np.fromfile(tag + ".w", np.complex64).reshape((B, S, N) if form == "full" else (B, S))
            got = np.fromfile(tag + ".out", np.complex64).reshape(-1, B, N)
            assert np.array_equal(u32(got), u32(BO.beams_ordered(W, X).transpose(1, 0, 2)))
