"""Spectrum integrator rates on one MI355X (gr4hip_fft_mag2_integrate / gr4hip_pfb_power_integrate; input and outputs resident in device memory).

    python tools/spectrum_integrator_rates.py [--out profiles/spectrum_integrator_rates.txt] [--log2 27] [--rounds 5] [--sizes 1024 8192] [--lengths 32 1024 65536]

2^27 complex samples per call, N in {1024, 8192} points, A in {32, 1024, 65536} frames per integration; the FFT block with the Hann window and the polyphase
filter bank at P = 1 and 4.  Per transform, measured in the same run and alternated round by round:
  (a) the transform's |X|^2 alone (gr4hip_fft_mag2 / gr4hip_pfb_process): 8 B in + 4 B out per sample;
  (b) the composition: (a) followed by gr4hip_specint_process on its output (every |X|^2 goes through HBM once more);
  (p) the integrating entry held to the composition in pieces (test hook gr4hip_internal_specint_set_path = 2: the |X|^2 goes through a 32 MiB scratch);
  (s) the integrating entry held to its sink kernel (hook = 1: the sum in the transform's launch);
  (f) the integrating entry as it runs by default (the path is printed: 1 = the sink, 2 = the composition in pieces);
  (c) once: a one-op gr4hip_ewise_process float program (4 B in + 4 B out per value): the bytes/s that define the 8 B/sample bound of the fused form.
Each figure is back-to-back calls at settled clocks (tools/_timing.py); every configuration is measured `rounds` times, min / median / max are recorded.  "wins":
the sink's median exceeds the better composition's ((b) or (p)) by more than the two spreads (max - min) combined -- the rule by which a size keeps the sink as
its default (specint_takes_sink in csrc/spectrum_integrator.hip)."""
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


def last_path(si):
    v = ctypes.c_int(-1)
    assert G.capi.lib().gr4hip_internal_specint_last_path(si._h, ctypes.byref(v)) == 0
    return v.value


def set_path(si, path):
    """the library's test hook: 1 = the sink wherever a kernel exists, 2 = the composition in pieces, 0 = the default"""
    assert G.capi.lib().gr4hip_internal_specint_set_path(si._h, ctypes.c_int(path)) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_integrator_rates.txt"))
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--lengths", type=int, nargs="+", default=[32, 1024, 65536])
    ap.add_argument("--taps", type=int, nargs="+", default=[1, 4], help="taps per channel of the banks")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the rates are measured on the GPU or not at all"
    n = 1 << a.log2
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=g) * 0.70710678)
    mag2 = torch.empty(n, dtype=torch.float32, device="cuda")
    out = torch.empty(n, dtype=torch.float32, device="cuda")  # room for A = 1

    # (c) the streaming yardstick: n floats in, n floats out
    prog = G.Merged(torch.float32, [("Multiply", 2.0)])
    sec = sorted(steady(lambda: prog.process_bulk(mag2, out=out)) for _ in range(a.rounds))
    bw = [8.0 * n / s for s in sec]  # bytes/s, slowest last
    bw_med = statistics.median(bw)
    bound = bw_med / 8.0 / 1e9  # G samples/s of a path that moves 8 B per sample
    say(f"one-op float program, 2^{a.log2} values: {min(bw) / 1e12:5.2f} / {bw_med / 1e12:5.2f} / {max(bw) / 1e12:5.2f} TB/s (min / median / max of {a.rounds})"
        f"   -> 8 B/sample bound {bound:6.1f} G samples/s, 12 B/sample bound {bw_med / 12.0 / 1e9:6.1f}")

    for N in a.sizes:
        frames = n // N
        transforms = [("FFT block, Hann", G.FFT(N, "Hann"), lambda t: t.mag2(x, out=mag2))]
        for P in a.taps:
            transforms.append((f"polyphase filter bank P {P}", G.PolyphaseFilterBank(N, P), lambda t: t.power(x, out=mag2)))
        for tname, t, alone in transforms:
            cases = [("(a) |X|^2 alone", lambda t=t, alone=alone: alone(t), None)]
            for A in a.lengths:
                if A > frames:
                    continue
                sb = G.SpectrumIntegrator(N, A)

                def comp(t=t, alone=alone, sb=sb):
                    alone(t)
                    sb.reset()
                    sb.process_bulk(mag2, out=out)
                cases.append((f"(b) composition, A {A}", comp, None))
                for tag, path in (("(p) entry, composition in pieces", 2), ("(s) entry, sink", 1), ("(f) entry, default", 0)):
                    sf = G.SpectrumIntegrator(N, A)
                    set_path(sf, path)

                    def entry(t=t, sf=sf):
                        sf.reset()
                        t.power_integrated(x, sf, out=out)
                    cases.append((f"{tag}, A {A}", entry, sf))
            sec = {name: [] for name, _, _ in cases}
            for _ in range(a.rounds):  # alternated: a drift of the machine reaches every configuration alike
                for name, fn, _ in cases:
                    sec[name].append(steady(fn))
            rate = {name: sorted(n / s / 1e9 for s in v) for name, v in sec.items()}
            for name, _, si in cases:
                r = rate[name]
                tail = ""
                if si is not None:
                    A = name.rsplit(" ", 1)[1]
                    tail = f"   path {last_path(si)}   {statistics.median(r) / bound:5.3f} of the 8 B/sample bound"
                    if name.startswith("(s)"):  # the sink against the better of the two compositions
                        c = max((rate[f"(b) composition, A {A}"], rate[f"(p) entry, composition in pieces, A {A}"]), key=statistics.median)
                        gain = statistics.median(r) - statistics.median(c)
                        spreads = (r[-1] - r[0]) + (c[-1] - c[0])
                        tail += (f"   {statistics.median(r) / statistics.median(c):5.3f} of the better composition: {'wins' if gain > spreads else 'does not win'}"
                                 f" (median gain {gain:+.1f}, spreads {spreads:.1f})")
                say(f"N {N:5d} {tname:<28} {name:<44} {r[0]:7.1f} / {statistics.median(r):7.1f} / {r[-1]:7.1f} G samples/s (min / median / max of {a.rounds}){tail}")
            t.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/spectrum_integrator_rates.py on %s: 2^%d complex samples per call, back-to-back calls at settled clocks, configurations alternated round by round\n"
                 % (torch.cuda.get_device_name(0), a.log2))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
