"""Cross-spectrum correlator rates on one MI355X (gr4hip_xcorr_process; inputs and output resident in device memory).

    python tools/cross_spectrum_rates.py [--out profiles/cross_spectrum_rates.txt] [--log2 27] [--rounds 5]

2^27 complex input samples in total per call (2^27 / S per stream); N = 1024 at S = 2, 4, 8, 16, 32 and N = 8192 at S = 2 and 16; A = 64 and 1024 frames per
integration.  Per shape, measured in the same run and alternated round by round:
  (v) the streaming VALU form (test hook gr4hip_internal_xcorr_set_path = 1), where it exists (S <= 8);
  (m) the matrix-pipe form (hook = 2);
  (t) S = 2 and 4: the torch expression (X_i * X_j.conj()).view(Q, A, N).sum(1) over all pairs j <= i -- what a user can do today;
  (c) once: a one-op gr4hip_ewise_process float program (4 B in + 4 B out per value): the bytes/s that define the read bound of 8 B per input sample.
Each figure is back-to-back calls at settled clocks (tools/_timing.py); every configuration is measured `rounds` times, min / median / max are recorded, in G
input samples/s (all streams).  Shares: of the read bound, and (m) of the 155 TFLOP/s f32 matrix peak against the flop the form executes (1024 per frame of a stream, bin
and 16 x 16 tile, a frame of S input samples: 1, 2, 4, 6 tiles at S <= 8, 16, 24, 32).  "wins": a form's median exceeds the other's by more than the two spreads (max - min) combined -- the
rule by which a stream count gets its default form (xcorr_path in csrc/cross_spectrum.hip; SPECTRUM_INTEGRATOR.md's dispatch rule)."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402

MATRIX_PEAK = 155e12


def set_path(blk, path):
    assert ctypes.CDLL(G.capi.LIB_PATH).gr4hip_internal_xcorr_set_path(blk._h, ctypes.c_int(path)) == 0


def last_path(blk):
    v = ctypes.c_int(-1)
    assert ctypes.CDLL(G.capi.LIB_PATH).gr4hip_internal_xcorr_last_path(blk._h, ctypes.byref(v)) == 0
    return v.value


def tiles(S):
    return 1 if S <= 8 else 2 if S <= 16 else 4 if S <= 24 else 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_spectrum_rates.txt"))
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lengths", type=int, nargs="+", default=[64, 1024])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the rates are measured on the GPU or not at all"
    n = 1 << a.log2
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=g) * 0.70710678)
    out = torch.empty(n // 64 * 17, dtype=torch.complex64, device="cuda")  # room for S = 32 at A = 64: n / (S A) matrices of P values per bin

    # (c) the streaming yardstick: n floats in, n floats out
    fin, fout = torch.view_as_real(x).reshape(-1)[:n], torch.empty(n, dtype=torch.float32, device="cuda")
    prog = G.Merged(torch.float32, [("Multiply", 2.0)])
    sec = sorted(steady(lambda: prog.process_bulk(fin, out=fout)) for _ in range(a.rounds))
    del fout
    bw = [8.0 * n / s for s in sec]
    bw_med = statistics.median(bw)
    bound = bw_med / 8.0 / 1e9  # G samples/s of a path that reads 8 B per input sample and writes next to nothing
    say(f"one-op float program, 2^{a.log2} values: {min(bw) / 1e12:5.2f} / {bw_med / 1e12:5.2f} / {max(bw) / 1e12:5.2f} TB/s (min / median / max of {a.rounds})"
        f"   -> read bound {bound:6.1f} G samples/s")

    for N, streams in ((1024, (2, 4, 8, 16, 32)), (8192, (2, 16))):
        for S in streams:
            frames = n // (S * N)
            xs = x.view(S, frames, N)
            for A in a.lengths:
                Q = frames // A
                cases = []
                for tag, path in (("(v) VALU form", 1), ("(m) matrix-pipe form", 2)):
                    if path == 1 and S > 8:
                        continue
                    blk = G.CrossSpectrum(S, N, A)
                    set_path(blk, path)

                    def call(blk=blk):
                        blk.reset()
                        blk.process_bulk(xs, out=out)
                    cases.append((tag, call, blk))
                if S <= 4:
                    def today(xs=xs, S=S, Q=Q, A=A, N=N):
                        return [(xs[i] * xs[j].conj()).view(Q, A, N).sum(1) for i in range(S) for j in range(i + 1)]
                    cases.append(("(t) torch, all pairs", today, None))
                sec = {name: [] for name, _, _ in cases}
                for _ in range(a.rounds):  # alternated: a drift of the machine reaches every configuration alike
                    for name, fn, _ in cases:
                        sec[name].append(steady(fn))
                rate = {name: sorted(n / s / 1e9 for s in v) for name, v in sec.items()}
                for name, _, blk in cases:
                    r = rate[name]
                    med = statistics.median(r)
                    tail = f"   {med / bound:5.3f} of the read bound"
                    if blk is not None:
                        tail = f"   path {last_path(blk)}" + tail
                    if name.startswith("(m)"):
                        tail += f"   {tiles(S) * 1024 * med * 1e9 / S / 1e12:6.1f} TFLOP/s executed = {tiles(S) * 1024 * med * 1e9 / S / MATRIX_PEAK:5.3f} of the f32 matrix peak"
                        if "(v) VALU form" in rate:
                            v = rate["(v) VALU form"]
                            gain, spreads = med - statistics.median(v), (r[-1] - r[0]) + (v[-1] - v[0])
                            verdict = "the matrix pipe wins" if gain > spreads else "VALU wins" if -gain > spreads else "no winner"
                            tail += f"   {med / statistics.median(v):5.3f} of VALU: {verdict} (median gain {gain:+.1f}, spreads {spreads:.1f})"
                    say(f"N {N:5d} S {S:2d} A {A:5d} {name:<22} {r[0]:7.2f} / {med:7.2f} / {r[-1]:7.2f} G samples/s (min / median / max of {a.rounds}){tail}")
                for _, _, blk in cases:
                    if blk is not None:
                        blk.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/cross_spectrum_rates.py on %s: 2^%d complex input samples per call over all streams, back-to-back calls at settled clocks, configurations alternated round by round\n"
                 % (torch.cuda.get_device_name(0), a.log2))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
