"""GPU tests of round 8's trim of the radix-16 layers (csrc/fft_radix.hpp): the internal W_16 twiddles of every 16-point DFT folded into its second-step butterflies
(fft16_fold, fft16_tw_fold) -- the fused chain's passes A, B, C and the tail correction's B', C', the windowed modes' further transforms and the FFT-only frame pipeline
(the FFT block's own kernels keep the plain butterflies: with the fold their 2^18-point parity test read 1.77e-5 against its bar of 1e-5, so no case here runs them
at 256 or 4096 points -- nothing in them changed; their 8192-point frames reach the changed code through the frame pipeline, below).

Everything goes through the public handles and is judged against float64 with the parity metric (`_rel` is tests/test_gpu_parity.py's) at the project's bar 1e-5 AND at
three times the error the build before the change measured on the same inputs (BEFORE; round 7's rule for a fold that adds one rounding per butterfly; both columns are in
profiles/r08_headline_trim.txt section 5).  Shapes are the smallest that reach each pass; every case prints its figure (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 8192
# unit impulses at these samples sit in rows 0, 1, 16 and 31 of pass A's 32 x 256 image, in its first and last columns, on both lanes of a lane pair
IMPULSES = (0, 1, 255, 256, 257, 16 * 256, 16 * 256 + 1, 31 * 256, 8191)

# the same cases on the build before the change (parity metric against float64)
BEFORE = {
    "pipeline-impulses": 2.350e-07,
    "pipeline-hann-mag2": 2.883e-07,
    "chain-rect": 2.337e-07,
    "chain-hann": 5.536e-07,
    "chain-1024-hann": 7.935e-07,
    "fir-output": 8.205e-07,
    "multi-fold": 1.663e-07,
    "multi-own": 2.337e-07,
    "guard": 3.506e-07,
}


def _rel(got, truth):
    got = np.asarray(got).astype(np.complex128 if np.iscomplexobj(got) else np.float64).ravel()
    truth = np.asarray(truth).ravel()
    rms = np.sqrt(np.mean(np.abs(truth) ** 2))
    return float(np.max(np.abs(got - truth) / np.maximum(np.abs(truth), rms if rms > 0 else 1.0)))


def _judge(name, err):
    before = BEFORE[name]
    print(f"trim-test {name} err {err:.3e} (before {before:.3e})")
    assert err <= TOL
    assert err <= 3.0 * before


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


@pytest.fixture(scope="module")
def stream(G):
    """the stream the chain cases share: 3 frames of 8192, noise + a tone inside the pass band of a 256-tap Hamming low-pass at 0.1 (the headline's input and taps)"""
    x = G.synth_c32(3 * N, seed=42)
    return O.design_taps_hamming_lowpass(256, 0.1), x, x.cpu().numpy()


def test_frame_pipeline_impulses(G):
    """(a) the FFT-only frame pipeline (chain_fd_kernel without its filter; the FFT block hands it calls of 256 frames or more, so 256 it is): a unit impulse per frame,
    raw spectrum; a slot or sign slip in a 16-point DFT moves whole groups of bins, which an impulse shows in every bin"""
    frames = 256
    x = np.zeros((frames, N), np.complex64)
    pos = [IMPULSES[f % len(IMPULSES)] for f in range(frames)]
    x[np.arange(frames), pos] = 1.0
    got = G.FFT(N, "None").spectrum(torch.from_numpy(x.reshape(-1)).cuda()).cpu().numpy()
    k = np.arange(N)
    worst = 0.0
    for f in list(range(2 * len(IMPULSES))) + [frames - 1]:
        worst = max(worst, _rel(got[f], np.exp(-2j * np.pi * ((k * pos[f]) % N) / N)))
    _judge("pipeline-impulses", worst)


def test_frame_pipeline_windowed(G):
    """(a) the windowed FFT-only mode of the same pipeline, |X|^2 of noise frames under a Hann window"""
    frames = 256
    xd = G.synth_c32(frames * N, seed=7)
    got = G.FFT(N, "Hann").mag2(xd).cpu().numpy()
    xh, w = xd.cpu().numpy().reshape(frames, N), O.window(3, N)
    worst = max(_rel(got[f], np.abs(np.fft.fft(xh[f].astype(np.complex128) * w)) ** 2) for f in (0, 1, frames - 1))
    _judge("pipeline-hann-mag2", worst)


@pytest.mark.parametrize("fft_size,window,name", [(8192, "None", "chain-rect"), (8192, "Hann", "chain-hann"), (1024, "Hann", "chain-1024-hann")])
def test_chain_modes(G, stream, fft_size, window, name):
    """(b), (c) the headline instantiation, Hann (three transforms: passA_inplace) and fftSize 1024 (the block's FIR part, its inverse, the 16 x 16 x 4 plan): 3 frames in
    two calls of 1 + 2, so the carried history, the tail correction E and the deferred stores are live"""
    b, xd, xh = stream
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    truth, _ = O.chain(b, xh, fft_size, wid, truth=True)
    ch = G.Chain(b, fft_size, window)
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    parts = []
    for lo, hi in ((0, N), (N, 3 * N)):
        parts.append(ch.process_bulk(xd[lo:hi]).cpu().numpy().ravel())
        if name == "chain-rect":
            assert ch.last_guard_fractions()[0] == 0.0  # the headline input is a clean stream: not one frame marked
    _judge(name, _rel(np.concatenate(parts), truth))


def test_fir_output_mode(G):
    """(d) the FIR-output mode (two transforms, y itself stored): spans of 64 frames or more whose start is only 8-byte aligned take it, so 64 it is; a first call of one
    frame on the direct form leaves the history it starts from.  Judged on the fast convolution's span"""
    frames = 64
    b = O.design_taps_hamming_lowpass(256, 0.1)
    buf = torch.empty((1 + frames) * N + 1, dtype=torch.complex64, device="cuda")
    xd = buf[1:]
    xd.copy_(G.synth_c32((1 + frames) * N, seed=42))
    truth, _ = O.fir(b, xd.cpu().numpy())
    f = G.fir_filter(b, torch.complex64)
    f.process_bulk(xd[:N])
    got = f.process_bulk(xd[N:]).cpu().numpy()
    paths = G.capi.lib().gr4hip_internal_fir_last_paths  # (the library's test hook, as in tests/test_gpu_fir_dispatch.py: bit 1 = the fast convolution)
    paths.restype, paths.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint)]
    mask = C.c_uint(0)
    assert paths(f._h, C.byref(mask)) == 0 and mask.value >> 1 & 1, "the span did not run on the fused kernel's FIR-output mode"
    _judge("fir-output", _rel(got, truth[N:]))


def test_multi_two_channels(G, stream):
    """(e) two channels in one launch (chain_fd_multi_kernel): the shared-taps fold and own spectra per channel, in calls of 1 + 2 frames"""
    from gnuradio4_amd.blocks import chain_process_multi
    b, xd, xh = stream
    x1 = G.synth_c32(3 * N, seed=43, tone_frel=0.05)
    xs, truths = [xd, x1], [O.chain(b, xh, N, 0, truth=True)[0], O.chain(b, x1.cpu().numpy(), N, 0, truth=True)[0]]
    fold = [G.Chain(b, N, "None") for _ in range(2)]
    own = [G.Chain(b, N, "None") for _ in range(2)]
    sums, outs = [], [[], []]
    for lo, hi in ((0, N), (N, 3 * N)):
        sums.append(chain_process_multi(fold, [x[lo:hi] for x in xs], want_outs=False)[1].cpu().numpy().ravel())
        o, _ = chain_process_multi(own, [x[lo:hi] for x in xs])
        for c in range(2):
            outs[c].append(o[c].cpu().numpy().ravel())
    _judge("multi-fold", _rel(np.concatenate(sums), truths[0] + truths[1]))
    _judge("multi-own", max(_rel(np.concatenate(outs[c]), truths[c]) for c in range(2)))


def test_guard_marks_every_frame(G):
    """(f) a stream the guard marks in every frame -- a tone 50 dB above the noise that a narrow low-pass removes: the marked fraction is what it was before the change
    (1.0: both frames), and the result, evaluated again behind the launch, meets the bar"""
    b = O.design_taps_hamming_lowpass(256, 0.02)
    x = O.signal_c32(6, 2 * N, tone_frel=0.31, tone_amp=300.0)
    truth, _ = O.chain(b, x, N, 0, truth=True)
    ch = G.Chain(b, N, "None")
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    got = ch.process_bulk(torch.from_numpy(x).cuda()).cpu().numpy().ravel()
    marked, _ = ch.last_guard_fractions()
    print(f"trim-test guard marked {marked:.2f}")
    assert marked == 1.0
    _judge("guard", _rel(got, truth))
