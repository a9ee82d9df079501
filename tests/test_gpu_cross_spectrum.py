"""The cross-spectrum correlator on the device (gr4hip_xcorr_*; csrc/cross_spectrum.hip) against its oracle (tests/cross_spectrum_oracle.py).  Every comparison of
emitted matrices is uint32 equality with the ordered definition: the streaming VALU form (S <= 8), the matrix-pipe form (every S) and every cut of the stream
have to land on the same bits.  Inputs are unit complex noise plus a common component, so the cross terms neither vanish nor dominate.

Shapes: S = 2, 3, 8, 9, 16, 17, 32 (a tile edge on both sides of 8 and of 16) at N = 64, A = 65 and 2 A + 3 frames (a ragged leaf, a dropped tail); N = 2, 8, 1028
at S = 3 (the smallest, below one 16-bin workgroup tile, no multiple of it); A = 1, 63, 64, 130 at S = 4 (below, at and above a leaf)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import cross_spectrum_oracle as XO
import oracle_lib as O

pytestmark = pytest.mark.gpu
CANARY = -77.25
HOST_BIN = os.path.join(O.ROOT, "build", "host", "test_host_cross_spectrum")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


_cases = {}


def case(S, N, A, frames=None, mean=False):
    """(input complex64 [S, frames, N], the ordered definition's matrices): computed once, shared, read-only"""
    frames = 2 * A + 3 if frames is None else frames
    key = (S, N, A, frames, mean)
    if key not in _cases:
        X = XO.streams(S, frames, N, 1000 * S + 10 * N + A)
        V = XO.cross_ordered(X, A, mean)
        X.setflags(write=False)
        V.setflags(write=False)
        _cases[key] = (X, V)
    return _cases[key]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def set_path(G, blk, path):
    L = C.CDLL(G.capi.LIB_PATH)
    assert L.gr4hip_internal_xcorr_set_path(blk._h, path) == 0


def last_path(G, blk):
    L = C.CDLL(G.capi.LIB_PATH)
    p = C.c_int(-1)
    assert L.gr4hip_internal_xcorr_last_path(blk._h, C.byref(p)) == 0
    return p.value


def run(G, X, A, mean=False, path=0):
    S, frames, N = X.shape
    blk = G.CrossSpectrum(S, N, A, mean)
    if path:
        set_path(G, blk, path)
    got = blk.process_bulk(torch.from_numpy(np.array(X)).cuda())
    return got.cpu().numpy(), last_path(G, blk)


@pytest.mark.parametrize("S", [2, 3, 8, 9, 16, 17, 32])
def test_every_stream_count_is_the_definition_bit_for_bit(G, S):
    X, want = case(S, 64, 65)
    got, path = run(G, X, 65)
    assert got.shape == want.shape == (2, S * (S + 1) // 2, 64)
    assert np.array_equal(u32(got), u32(want))
    assert path in (1, 2) and (path == 2 or S <= 8)  # the VALU form exists for S <= 8 only


@pytest.mark.parametrize("N", [2, 7, 8, 1028])  # 7: an odd row length, where the matrix-pipe form's 16-byte leaf stores give way to 8-byte ones
@pytest.mark.parametrize("path", [1, 2])
def test_every_kind_of_bin_count(G, N, path):
    X, want = case(3, N, 65)
    got, ran = run(G, X, 65, path=path)
    assert ran == path and np.array_equal(u32(got), u32(want))


@pytest.mark.parametrize("A", [1, 63, 64, 130])
@pytest.mark.parametrize("path", [1, 2])
def test_every_kind_of_integration_length(G, A, path):
    X, want = case(4, 64, A)
    got, ran = run(G, X, A, path=path)
    assert ran == path and got.shape == want.shape == ((2 * A + 3) // A, 10, 64) and np.array_equal(u32(got), u32(want))


@pytest.mark.parametrize("S", [2, 5, 8])
def test_both_forms_give_the_same_bits(G, S):
    X, want = case(S, 64, 65)
    a, pa = run(G, X, 65, path=1)
    b, pb = run(G, X, 65, path=2)
    assert (pa, pb) == (1, 2)
    assert np.array_equal(u32(a), u32(want)) and np.array_equal(u32(b), u32(want))


def test_the_hook_above_eight_streams_reports_the_matrix_pipe(G):
    X, want = case(9, 64, 65)
    got, ran = run(G, X, 65, path=1)  # there is no VALU kernel for nine streams
    assert ran == 2 and np.array_equal(u32(got), u32(want))


@pytest.mark.parametrize("path", [1, 2])
def test_cuts_do_not_change_a_bit(G, path):
    S, N, A = 5, 64, 70
    X, want = case(S, N, A, frames=5 * A)
    d = torch.from_numpy(np.array(X)).cuda()
    blk = G.CrossSpectrum(S, N, A)
    set_path(G, blk, path)
    L = G.capi.lib()
    pieces, at = [], 0
    for n in (1, A - 1, 64, 65, 5 * A - (1 + A - 1 + 64 + 65)):
        expect = blk.pending(n)
        part = [d[s, at:at + n].contiguous() for s in range(S)]
        if expect == 0:  # a call that completes nothing is accepted without an output
            ptrs = (C.c_void_p * S)(*[p.data_ptr() for p in part])
            got_n = C.c_size_t(99)
            assert L.gr4hip_xcorr_process(blk._h, ptrs, n, None, C.byref(got_n), torch.cuda.current_stream().cuda_stream) == 0 and got_n.value == 0
        else:
            out = blk.process_bulk(part)
            assert out.shape[0] == expect
            pieces.append(out.cpu().numpy())
        at += n
    assert at == 5 * A
    got = np.concatenate(pieces)
    assert got.shape == want.shape == (5, 15, N) and np.array_equal(u32(got), u32(want))
    whole, _ = run(G, X, A, path=path)
    assert np.array_equal(u32(whole), u32(got))


def test_a_call_longer_than_one_piece_of_the_leaf_scratch(G):
    """the call is worked off in pieces of 2^25 input values (all streams): only a size that large has more than one piece.  N = 2^19 at S = 2 makes a piece 32
    frames: 40 frames are two pieces, the cut inside the first leaf of an integration of 33 frames"""
    S, N, A, frames, block = 2, 1 << 19, 33, 40, 4096
    X = np.tile(XO.streams(S, frames, block, 5), (1, 1, N // block))  # the same 4096 bins 128 times over
    got, _ = run(G, X, A)
    want = XO.cross_ordered(X[:, :, :block], A)
    assert got.shape == (1, 3, N) and np.array_equal(u32(got), u32(np.tile(want, (1, 1, N // block))))


def test_reset_and_set_length_clear_the_carry(G):
    S, N, A = 3, 64, 65
    X, want = case(S, N, A)
    d = torch.from_numpy(np.array(X)).cuda()
    blk = G.CrossSpectrum(S, N, A)
    assert blk.process_bulk(d[:, :40].contiguous()).shape[0] == 0 and blk.pending(25) == 1
    blk.reset()
    assert blk.pending(64) == 0
    assert np.array_equal(u32(blk.process_bulk(d).cpu().numpy()), u32(want))  # 2 A + 3 frames from a clean start; three frames stay behind
    blk.set_length(63)
    assert blk.pending(63) == 1
    X2, want2 = case(S, N, 63)
    assert np.array_equal(u32(blk.process_bulk(torch.from_numpy(np.array(X2)).cuda()).cpu().numpy()), u32(want2))


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("path", [1, 2])
def test_the_carried_state_through_cuts_set_length_and_reset(G, path, mean):
    """the state the integrating blocks share (csrc/leaf_integrator.hpp) behind the public entries alone, at S = 3, N = 7 (rows of 84 floats) and A = 65: calls of
    1, 63, 1, 0, 65, 2 frames, set_length(2) in mid-integration, 3 frames, one more, reset(), 4 frames -- every call returns what pending said, the rows are the
    ordered definition of the segments between the drops, bit for bit, and the diagonal's imaginary parts are +0"""
    S, N, A = 3, 7, 65
    X = XO.streams(S, 140, N, 77)
    d = torch.from_numpy(X).cuda()
    blk, at, got = G.CrossSpectrum(S, N, A, mean), 0, []
    set_path(G, blk, path)

    def feed(n):
        nonlocal at
        want = blk.pending(n)
        out = blk.process_bulk([d[s, at:at + n].contiguous() for s in range(S)])
        assert out.shape == (want, 6, N) and (n == 0 or last_path(G, blk) == path)
        got.append(out.cpu().numpy())
        at += n

    for n in (1, 63, 1, 0, 65, 2):
        feed(n)
    assert at == 132 and blk.pending(A - 2) == 1
    blk.set_length(2)  # frames 130, 131 are dropped
    assert blk.pending(1) == 0 and blk.pending(2) == 1
    feed(3)
    feed(1)
    blk.reset()
    assert blk.pending(1) == 0
    feed(4)
    assert at == 140
    want = np.concatenate([XO.cross_ordered(X[:, :132], A, mean), XO.cross_ordered(X[:, 132:136], 2, mean), XO.cross_ordered(X[:, 136:], 2, mean)])
    got = np.concatenate(got)
    assert got.shape == want.shape == (6, 6, N) and np.array_equal(u32(got), u32(want))
    diag = [XO.baseline(i, i) for i in range(S)]
    assert not u32(got.imag[:, diag]).any() and u32(got.imag[:, [XO.baseline(1, 0), XO.baseline(2, 0), XO.baseline(2, 1)]]).all()


@pytest.mark.parametrize("path", [1, 2])
def test_mean_mode(G, path):
    X, want = case(4, 64, 130, mean=True)
    got, _ = run(G, X, 130, mean=True, path=path)
    assert np.array_equal(u32(got), u32(want))


def test_the_same_pointer_for_two_streams(G):
    X, _ = case(3, 64, 65)
    Y = np.stack([X[0], X[1], X[0]])
    want = XO.cross_ordered(Y, 65)
    d = torch.from_numpy(np.array(X)).cuda()
    blk = G.CrossSpectrum(3, 64, 65)
    a, b = d[0].contiguous(), d[1].contiguous()
    got = blk.process_bulk([a, b, a]).cpu().numpy()
    assert np.array_equal(u32(got), u32(want))
    assert np.array_equal(u32(got[:, XO.baseline(2, 0)].real), u32(got[:, XO.baseline(0, 0)].real))


@pytest.mark.parametrize("S,path", [(4, 1), (4, 2), (17, 2)])
def test_a_nan_reaches_only_its_stream_integration_and_bin(G, S, path):
    N, A = 64, 65
    X0, _ = case(S, N, A)
    X = np.array(X0)
    X[2, A + 7, 13] = np.nan  # stream 2, second integration, bin 13
    want = XO.cross_ordered(X, A)
    got, _ = run(G, X, A, path=path)
    hit = np.zeros(got.shape, bool)
    for i in range(S):
        for j in range(i + 1):
            if i == 2 or j == 2:
                hit[1, XO.baseline(i, j), 13] = True
    # the imaginary part of a diagonal element is +0 by definition, also here
    finite = np.isfinite(got.real) & np.isfinite(got.imag)
    assert not finite[hit].any() and finite[~hit].all()
    assert got[1, XO.baseline(2, 2), 13].imag == 0 and np.isnan(got[1, XO.baseline(2, 2), 13].real)
    assert np.array_equal(u32(got[~hit]), u32(want[~hit]))


def test_coherence_is_the_float64_formula_bit_for_bit(G):
    S, N, A = 4, 64, 65
    X, V = case(S, N, A)
    V = np.array(V)
    V[1, :, 5] = 0  # a bin without power in the second matrix: IEEE's 0 / 0
    V[1, XO.baseline(3, 3), 6] = 0  # zero auto-power of one stream only: x / 0
    blk = G.CrossSpectrum(S, N, A)
    d = torch.from_numpy(V).cuda()
    for i, j in ((2, 1), (1, 2), (3, 0), (0, 3), (3, 3)):
        msc, h1 = blk.coherence(d, i, j)
        wm, wh = XO.coherence(V, S, i, j)
        assert msc.shape == (2, N) and h1.shape == (2, N)
        gm, gh = msc.cpu().numpy(), h1.cpu().numpy()
        same = lambda a, b: np.array_equal(u32(a)[~np.isnan(b)], u32(b)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))
        assert same(gm, wm) and same(gh.real, wh.real) and same(gh.imag, wh.imag), (i, j)
        assert np.isnan(gm[1, 5])
    msc, h1 = blk.coherence(d[0], 3, 3)
    assert msc.shape == (N,) and bool((msc == 1).all()) and bool((h1 == 1).all())
    msc, _ = blk.coherence(d, 3, 0)
    assert np.isinf(msc.cpu().numpy()[1, 6])
    with pytest.raises(G.capi.Gr4HipError):
        blk.coherence(d, 4, 0)


def test_two_spectra_that_share_a_tone_are_coherent_at_its_bin(G):
    """the Python block fed from G.FFT(...).spectrum: plumbing, no threshold beyond the ordering"""
    N, A, tone = 256, 32, 37
    rng = np.random.default_rng(3)
    t = np.arange(N * A)
    s = np.exp(2j * np.pi * tone / N * t)
    x = [(s * a + (rng.standard_normal(N * A) + 1j * rng.standard_normal(N * A)) / np.sqrt(2)).astype(np.complex64) for a in (1.0, 0.5j)]
    fft = G.FFT(N, "Hann")
    spectra = [fft.spectrum(torch.from_numpy(v).cuda()) for v in x]
    blk = G.CrossSpectrum(2, N, A, mean=True)
    vis = blk.process_bulk(spectra)
    assert vis.shape == (1, 3, N)
    msc, h1 = blk.coherence(vis, 1, 0)
    m = msc.cpu().numpy()[0]
    at = int(np.argmax(vis.cpu().numpy()[0, blk.baseline(0, 0)].real))  # the tone's bin, whichever order the spectra come in
    quiet = (at + N // 2) % N
    assert m[at] > m[quiet]
    assert h1.shape == (1, N)


def test_the_host_block_on_the_device_is_the_definition(tmp_path):
    """gr::blocks::fft::CrossSpectrum<float> behind compute_domain gpu:hip:0: the seam onto gr4hip_xcorr_process (gr4/hip.hpp)"""
    prefix = str(tmp_path / "dev")
    r = subprocess.run([HOST_BIN, "device", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "cross spectrum device: ok" in r.stdout
    assert "handle re-make (n_integrate 2 -> 4 by settings): 96 values, device == host" in r.stdout  # the seam makes the handle anew between two work() calls
    for S, N, A in ((2, 8, 1), (3, 16, 63), (5, 8, 65), (4, 8, 130)):
        for mean in (False, True):
            tag = f"{prefix}.S{S}.N{N}.A{A}.{'mean' if mean else 'sum'}"
            X = np.fromfile(tag + ".in", np.complex64).reshape(S, -1, N)
            got = np.fromfile(tag + ".out", np.complex64).reshape(-1, S * (S + 1) // 2, N)
            assert np.array_equal(u32(got), u32(XO.cross_ordered(X, A, mean)))
