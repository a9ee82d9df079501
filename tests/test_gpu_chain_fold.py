"""GPU tests of the fused chain's radix-16 layers after two instruction trims (csrc/fft_radix.hpp): pass A's lane-pair exchange (lane_xor1 without the dead `old`
operand) and the twiddle products folded into the first butterflies of the radix-16 behind them (fft16_tw: s = a + w b as fma chains, d = 2 a - s).  Everything
goes through the public handles and is judged against float64 with the parity metric (include/gr4hip.h; `_rel` is tests/test_gpu_parity.py's) at the project's bar
1e-5.  Shapes are the smallest that reach each changed pass; every case prints its measured error (pytest -s), recorded in profiles/r07_headline_fold.txt beside the
figures of the build before the change."""
import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 8192
IMPULSES = (0, 1, 255, 256, 257, 511, 4097, 8191)  # both lane parities of pass A's pair (rows 2 m / 2 m + 1), first and last column, a row change


def _rel(got, truth):
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


@pytest.fixture(scope="module")
def stream(G):
    """the stream every parity case shares: 3 frames of 8192, noise + a tone inside the pass band of a 256-tap Hamming low-pass at 0.1 (the headline's input and taps)"""
    x = G.synth_c32(3 * N, seed=42)
    return O.design_taps_hamming_lowpass(256, 0.1), x, x.cpu().numpy()


def _impulses(pairs):
    x = np.zeros((len(pairs), 2, N), np.complex64)
    for i, (a, b) in enumerate(pairs):
        x[i, 0, a] = 1.0
        x[i, 1, b] = 1.0
    return x


def test_pair_exchange_signs_fft_block(G):
    """unit impulses through the FFT block's raw spectrum, 8192 points, 2 frames per call (the block kernel: its last pass is the same lane-pair exchange): a sign or
    parity slip moves a whole column of bins, which an impulse shows in every bin"""
    F = G.FFT(N, "None")
    x = _impulses(list(zip(IMPULSES[0::2], IMPULSES[1::2])))
    worst = 0.0
    for call in x:
        got = F.spectrum(torch.from_numpy(call.reshape(-1)).cuda()).cpu().numpy()
        truth = np.fft.fft(call.astype(np.complex128), axis=1)
        for f in range(2):
            worst = max(worst, _rel(got[f], truth[f]))
    print(f"fold-test impulses fft-block err {worst:.3e}")
    assert worst <= TOL


def test_pair_exchange_signs_frame_pipeline(G):
    """the same impulses through the fused kernel's own pass A: the FFT block hands 256 frames or more to the frame pipeline (chain_fd_kernel, complex output)"""
    frames = 256
    x = np.zeros((frames, N), np.complex64)
    pos = [IMPULSES[f % len(IMPULSES)] for f in range(frames)]
    x[np.arange(frames), pos] = 1.0
    got = G.FFT(N, "None").spectrum(torch.from_numpy(x.reshape(-1)).cuda()).cpu().numpy()
    k = np.arange(N)
    worst = 0.0
    for f in list(range(len(IMPULSES))) + [frames - 1]:
        worst = max(worst, _rel(got[f], np.exp(-2j * np.pi * ((k * pos[f]) % N) / N)))
    print(f"fold-test impulses frame-pipeline err {worst:.3e}")
    assert worst <= TOL
    assert np.array_equal(got[len(IMPULSES):2 * len(IMPULSES)], got[:len(IMPULSES)])  # (every workgroup computes the same frame the same way)


def test_pair_exchange_signs_chain(G):
    """taps = delta[0] (256 taps, the first one 1): y = x, the spectrum of a unit impulse has |Y|^2 = 1 in every bin of every frame, through every layer of the
    headline instantiation (X's passes A, B, C and the tail correction's B', C')"""
    taps = np.zeros(256, np.float32)
    taps[0] = 1.0
    worst = 0.0
    for call in _impulses(list(zip(IMPULSES[0::2], IMPULSES[1::2]))):
        ch = G.Chain(taps, N, "None")
        assert ch.algo == G.capi.CHAIN_FUSED_FD
        got = ch.process_bulk(torch.from_numpy(call.reshape(-1)).cuda()).cpu().numpy()
        assert got.shape == (2, N)
        worst = max(worst, _rel(got, np.ones(2 * N)))
    print(f"fold-test impulses chain err {worst:.3e}")
    assert worst <= TOL


@pytest.mark.parametrize("fft_size,window", [(8192, "None"), (8192, "Hann"), (1024, "Hann")], ids=["rect-mag2", "hann", "small-1024"])
def test_chain_modes(G, stream, fft_size, window):
    """rectangular |Y|^2 (the headline instantiation), Hann (three transforms: passA_inplace + passB_table_store) and fftSize 1024 (the block's FIR part and its inverse),
    in two calls of 1 + 2 blocks: history, tail correction and the deferred stores are live"""
    b, xd, xh = stream
    wid = [w.lower() for w in O.WINDOWS].index(window.lower())
    truth, _ = O.chain(b, xh, fft_size, wid, truth=True)
    ch = G.Chain(b, fft_size, window)
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    parts = []
    for lo, hi in ((0, N), (N, 3 * N)):
        parts.append(ch.process_bulk(xd[lo:hi]).cpu().numpy().ravel())
        if fft_size == N and window == "None":
            assert ch.last_guard_fractions()[0] == 0.0  # the headline input is a clean stream: not one frame marked
    err = _rel(np.concatenate(parts), truth)
    print(f"fold-test chain {fft_size} {window} err {err:.3e}")
    assert err <= TOL


def test_fir_output_mode(G):
    """the FIR-output mode (fir_filter<complex<float>> as a fast convolution: two transforms, y itself stored): spans of 64 frames or more whose start is only 8-byte
    aligned take it; a first short call on the direct form leaves the history it starts from"""
    frames = 64
    b = O.design_taps_hamming_lowpass(256, 0.1)
    buf = torch.empty((1 + frames) * N + 1, dtype=torch.complex64, device="cuda")
    xd = buf[1:]
    xd.copy_(G.synth_c32((1 + frames) * N, seed=42))
    truth, _ = O.fir(b, xd.cpu().numpy())
    f = G.fir_filter(b, torch.complex64)
    got = np.concatenate([f.process_bulk(xd[:N]).cpu().numpy(), f.process_bulk(xd[N:]).cpu().numpy()])  # (both spans start at an odd element of the buffer: 8-byte aligned)
    err, err_fd = _rel(got, truth), _rel(got[N:], truth[N:])  # (the whole stream; the fast convolution's 64 frames by themselves)
    print(f"fold-test fir-output err {err:.3e} fast-convolution span {err_fd:.3e}")
    assert err <= TOL and err_fd <= TOL


def test_multi_two_channels(G, stream):
    """chain_process_multi with 2 channels (chain_fd_multi_kernel): the shared-taps fold kept in registers, and own spectra per channel, in calls of 1 + 2 frames"""
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
    e_fold = _rel(np.concatenate(sums), truths[0] + truths[1])
    e_own = max(_rel(np.concatenate(outs[c]), truths[c]) for c in range(2))
    print(f"fold-test multi fold err {e_fold:.3e} own err {e_own:.3e}")
    assert e_fold <= TOL and e_own <= TOL


def test_guard_still_marks_and_repairs(G):
    """a stream the guard marks -- a tone 50 dB above the noise that a narrow low-pass removes -- in two frames: the kernel still reports its marked frames
    (gr4hip_chain_last_guard_fractions) and the result, evaluated again behind the launch, still meets the bar"""
    b = O.design_taps_hamming_lowpass(256, 0.02)
    x = O.signal_c32(6, 2 * N, tone_frel=0.31, tone_amp=300.0)
    truth, _ = O.chain(b, x, N, 0, truth=True)
    ch = G.Chain(b, N, "None")
    assert ch.algo == G.capi.CHAIN_FUSED_FD
    got = ch.process_bulk(torch.from_numpy(x).cuda()).cpu().numpy().ravel()
    marked, _ = ch.last_guard_fractions()
    err = _rel(got, truth)
    print(f"fold-test guard marked {marked:.2f} err {err:.3e}")
    assert marked > 0.0
    assert err <= TOL
