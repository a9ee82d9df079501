"""float64 oracle of the overlapped / skipped FFT frames (include/gr4hip.h, gr4hip_stft_*; OVERLAPPED_FFT.md): the reference's `stride` stated for a stream.

    frame m of a stream = samples [m S, m S + N); emitted once its last sample has arrived; nothing synthetic is transformed
    per frame: the FFT block -- float32 window (the block's _window member) -> forward DFT -> outputs

count / cut restate the handle's rule (k frames for a call of n_in samples at offset off, then off += k S - n_in); starts_brute walks a stream sample by sample
without it."""
import numpy as np

import oracle_lib as O


def n_frames_total(n, N, S):
    """frames of a stream of n samples"""
    return 0 if n < N else (n - N) // S + 1


def frame_index(M, N, S):
    return np.arange(M)[:, None] * S + np.arange(N)[None, :]


def frames(x, N, S):
    """the frames of the whole stream x by the definition: [M, N]"""
    x = np.asarray(x).ravel()
    return x[frame_index(n_frames_total(len(x), N, S), N, S)]


def spectrum(x, N, S, window_id=3):
    """complex128 [M, N]: float32 window times the float32 samples, exactly, then a float64 transform (oracle_lib.dft64 up to 1024 points, numpy's above)"""
    f = frames(x, N, S).astype(np.complex128)
    if O.WINDOWS[window_id] not in ("None", "Rectangular"):
        f = f * O.window(window_id, N, np.float32).astype(np.float64)
    if N <= 1024:
        return np.stack([O.dft64(r) for r in f]) if len(f) else np.zeros((0, N), np.complex128)
    return np.fft.fft(f, axis=1)


def block_truth(x, N, S, window_id=3, **flags):
    """the FFT block's four signals per frame (oracle_lib.fft_block_truth): [4][M, n_out]"""
    per = [O.fft_block_truth(r, window_id, **flags) for r in frames(x, N, S)]
    return [np.stack([p[i] for p in per]) for i in range(4)]


def count(off, n_in, N, S):
    """frames a call of n_in samples emits when the next frame starts at `off` relative to its first sample"""
    return 0 if n_in - off < N else (n_in - N - off) // S + 1


def cut(sizes, N, S):
    """the handle's rule over a list of call sizes: [(k, off before the call)], and the final off"""
    off, out = 0, []
    for n in sizes:
        k = count(off, n, N, S)
        out.append((k, off))
        off += k * S - n
        assert off >= -(N - 1)
    return out, off


def starts_brute(sizes, N, S):
    """per call, the stream positions of the frames whose last sample arrives in it -- sample by sample, no rule"""
    pos, nxt, out = 0, 0, []
    for n in sizes:
        got = []
        for _ in range(n):
            pos += 1  # samples [0, pos) have arrived
            while nxt + N <= pos:
                got.append(nxt)
                nxt += S
        out.append(got)
    return out
