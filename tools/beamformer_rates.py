"""Beamformer rates on one MI355X (gr4hip_beamform_process, gr4hip_beamform_power_integrate; inputs, weights and outputs resident in device memory).

    python tools/beamformer_rates.py [--out profiles/beamformer_rates.txt] [--log2 27] [--rounds 5]

2^27 complex input samples in total per call (2^27 / S per stream) at N = 1024, for (S, B) = (2, 1), (4, 4), (8, 4), (16, 16), (32, 32), and for both entries: the
voltage beams (stride N, one dense stream per beam) and the integrated power with A = 1024.  Per shape and entry, measured in the same run and alternated round
by round:
  (v) the streaming VALU form (test hook gr4hip_internal_beamform_set_path = 1), where it exists (S <= 8 with B <= 8);
  (m) the matrix-pipe form (hook = 2);
  (t) torch.einsum('bsc,sfc->bfc', W, X), for the integrated power followed by abs()^2 and .view(Q, A, B N).sum(1) -- what a user can do today;
  (c) once: a one-op gr4hip_ewise_process float program (4 B in + 4 B out per value): the bytes/s behind the memory term of the bound.
Each figure is back-to-back calls at settled clocks (tools/_timing.py); every configuration is measured `rounds` times, min / median / max are recorded, in G
input samples/s (all streams).  The bound of a shape is the larger of two times per input sample: the bytes moved (8 (S + B) / S voltage, 8 integrated, the
latter's output being 1 / A of a frame) over the yardstick's bytes/s, and 8 B flop over the 155 TFLOP/s f32 matrix peak.  "wins": a form's median exceeds the
other's by more than the two spreads (max - min) combined -- the rule by which a shape gets its default form (bf_path in csrc/beamformer.hip;
SPECTRUM_INTEGRATOR.md's dispatch rule)."""
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
    assert ctypes.CDLL(G.capi.LIB_PATH).gr4hip_internal_beamform_set_path(blk._h, ctypes.c_int(path)) == 0


def last_path(blk):
    v = ctypes.c_int(-1)
    assert ctypes.CDLL(G.capi.LIB_PATH).gr4hip_internal_beamform_last_path(blk._h, ctypes.byref(v)) == 0
    return v.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beamformer_rates.txt"))
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--integrate", type=int, default=1024)
    ap.add_argument("--shapes", type=str, default="2x1,4x4,8x4,16x16,32x32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the rates are measured on the GPU or not at all"
    n, N, A = 1 << a.log2, 1024, a.integrate
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=g) * 0.70710678)

    # (c) the streaming yardstick: n floats in, n floats out
    fin, fout = torch.view_as_real(x).reshape(-1)[:n], torch.empty(n, dtype=torch.float32, device="cuda")
    prog = G.Merged(torch.float32, [("Multiply", 2.0)])
    bw = sorted(8.0 * n / steady(lambda: prog.process_bulk(fin, out=fout)) for _ in range(a.rounds))
    del fout
    bw_med = statistics.median(bw)
    say(f"one-op float program, 2^{a.log2} values: {bw[0] / 1e12:5.2f} / {bw_med / 1e12:5.2f} / {bw[-1] / 1e12:5.2f} TB/s (min / median / max of {a.rounds})")

    for S, B in shapes:
        frames = n // (S * N * A) * A  # whole integrations; S = 6 or 7 leaves a few samples of the 2^27 unused
        used = S * frames * N
        xs = x[:used].view(S, frames, N)
        w = torch.view_as_complex(torch.randn(B, S, N, 2, device="cuda", generator=g) * (0.5 / S) ** 0.5)
        volt = torch.empty(B * frames * N, dtype=torch.complex64, device="cuda")
        Q = frames // A
        power = torch.empty(max(Q, 1) * B * N, dtype=torch.float32, device="cuda")
        for entry in ("voltage", "power"):
            bytes_per_sample = 8.0 * (S + B) / S if entry == "voltage" else 8.0 + 4.0 * B / (S * A)
            t_mem, t_mat = bytes_per_sample / bw_med, 8.0 * B / MATRIX_PEAK
            bound = 1.0 / max(t_mem, t_mat) / 1e9
            limit = "memory" if t_mem >= t_mat else "matrix pipe"
            cases = []
            for tag, path in (("(v) VALU form", 1), ("(m) matrix-pipe form", 2)):
                if path == 1 and (S > 8 or B > 8):
                    continue
                blk = G.Beamformer(S, B, N)
                set_path(blk, path)
                blk.set_weights(w)
                if entry == "voltage":
                    def call(blk=blk):
                        blk.process_bulk(xs, out=volt)
                else:
                    si = G.SpectrumIntegrator(B * N, A)

                    def call(blk=blk, si=si):
                        si.reset()
                        blk.power_integrated(xs, si, out=power)
                cases.append((tag, call, blk))
            if entry == "voltage":
                def today():
                    return torch.einsum("bsc,sfc->bfc", w, xs)
            else:
                def today():
                    return torch.einsum("bsc,sfc->bfc", w, xs).abs().square().permute(1, 0, 2).reshape(Q, A, B * N).sum(1)
            cases.append(("(t) torch.einsum", today, None))
            sec = {name: [] for name, _, _ in cases}
            for _ in range(a.rounds):  # alternated: a drift of the machine reaches every configuration alike
                for name, fn, _ in cases:
                    sec[name].append(steady(fn))
            rate = {name: sorted(used / s / 1e9 for s in v) for name, v in sec.items()}
            for name, _, blk in cases:
                r = rate[name]
                med = statistics.median(r)
                tail = f"   {med / bound:5.3f} of the bound {bound:6.1f} ({limit})"
                if blk is not None:
                    tail = f"   path {last_path(blk)}" + tail
                if name.startswith("(m)") and "(v) VALU form" in rate:
                    v = rate["(v) VALU form"]
                    gain, spreads = med - statistics.median(v), (r[-1] - r[0]) + (v[-1] - v[0])
                    verdict = "the matrix pipe wins" if gain > spreads else "VALU wins" if -gain > spreads else "no winner"
                    tail += f"   {med / statistics.median(v):5.3f} of VALU: {verdict} (median gain {gain:+.1f}, spreads {spreads:.1f})"
                say(f"S {S:2d} B {B:2d} {entry:<7} {name:<22} {r[0]:7.2f} / {med:7.2f} / {r[-1]:7.2f} G samples/s (min / median / max of {a.rounds}){tail}")
            for _, _, blk in cases:
                if blk is not None:
                    blk.close()
        del volt, power, w

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/beamformer_rates.py on %s: 2^%d complex input samples per call over all streams, N = %d, A = %d, back-to-back calls at settled clocks, configurations alternated round by round\n"
                 % (torch.cuda.get_device_name(0), a.log2, N, A))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
