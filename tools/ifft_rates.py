"""Inverse transform and synthesis bank rates on one MI355X (gr4hip_ifft_process / gr4hip_pfb_synth_process; input and outputs resident in device memory).

    python tools/ifft_rates.py [--out profiles/ifft_synthesis_rates.txt] [--log2 27] [--rounds 5] [--sizes 1024 8192]

2^27 values per call at N in {1024, 8192}.  Every row is compared with existing code measured in the same run, alternated round by round:
  - the forward yardstick: gr4hip_fft_spectrum, no window, the same N -- the same 16 bytes per sample through the same kernel body.  (At N = 8192 the FFT block
    sends calls of >= 256 frames to the frame pipeline of the fused chain kernel; the row "fft_fast_kernel" is the FFT block with that pipeline switched off,
    GR4HIP_FFT_NO_PIPELINE: the kernel whose passes the inverse runs.)
  - C2C and C2R (8 + 4 bytes per output sample against 16);
  - the synthesis bank at P in {1, 4, 8} (required form: 32 bytes per sample through HBM plus 8 P through the L2) beside gr4hip_pfb_process(d_spectrum) at the
    same (N, P), the analysis direction;
  - what a user could do before: torch.fft.ifft(X, norm="forward"), and for the bank that plus a torch expression for the P-term sums.
Each figure is back-to-back calls at settled clocks (tools/_timing.py); every configuration is measured `rounds` times, min / median / max are recorded, and the
ratio is median over median.  FIRST MEASUREMENTS: no threshold decides anything."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402


def torch_bank(X, g, N, P):
    """the bank with torch alone: the unnormalised inverse transform, then y[m] = sum_k g[k] v[m - k] (zeros in front)"""
    v = torch.fft.ifft(X.view(-1, N), norm="forward")
    y = v * g[0]
    for k in range(1, P):
        y[k:] += v[:-k] * g[k]
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ifft_synthesis_rates.txt"))
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 8192])
    a = ap.parse_args()
    n = 1 << a.log2
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=gen) * 0.70710678)
    outc = torch.empty(n, dtype=torch.complex64, device="cuda")
    outr = torch.empty(n, dtype=torch.float32, device="cuda")

    for N in a.sizes:
        fft, c2c, c2r = G.FFT(N, "None"), G.InverseFFT(N), G.InverseFFT(N, torch.float32)
        synth = {P: G.PolyphaseSynthesisBank(N, P) for P in (1, 4, 8)}
        ana = {P: G.PolyphaseFilterBank(N, P) for P in (1, 4, 8)}
        taps = {P: torch.from_numpy(G.design_pfb(N, P)).cuda().view(P, N) for P in (1, 4, 8)}
        cases = [("forward: gr4hip_fft_spectrum, no window", lambda: fft.spectrum(x, out=outc), None)]
        if N == 8192:
            cases.append(("forward: fft_fast_kernel (frame pipeline off)", lambda: fft.spectrum(x, out=outc), "GR4HIP_FFT_NO_PIPELINE"))
        cases.append(("gr4hip_ifft_process C2C", lambda: c2c.process_bulk(x, out=outc), None))
        cases.append(("gr4hip_ifft_process C2R", lambda: c2r.process_bulk(x, out=outr), None))
        cases.append(("torch.fft.ifft(norm='forward')", lambda: torch.fft.ifft(x.view(-1, N), norm="forward"), None))
        for P in (1, 4, 8):
            cases.append((f"synthesis bank P {P}", lambda b=synth[P]: b.process_bulk(x, out=outc), None))
            cases.append((f"analysis bank P {P} (gr4hip_pfb_process, spectrum)", lambda b=ana[P]: b.process_bulk(x, out=outc), None))
            cases.append((f"torch: ifft + {P}-term sums", lambda P=P: torch_bank(x, taps[P], N, P), None))
        sec = {name: [] for name, _, _ in cases}
        for _ in range(a.rounds):  # alternated: a drift of the machine reaches every configuration alike
            for name, fn, switch in cases:
                if switch:
                    G.capi.developer_switch(switch, 1)
                sec[name].append(steady(fn))
                if switch:
                    G.capi.developer_switch(switch, 0)
        base = statistics.median(sec[cases[0][0]])
        for name, _, _ in cases:
            r = sorted(n / s / 1e9 for s in sec[name])
            say(f"N {N:5d} {name:<52} {r[0]:7.1f} / {statistics.median(r):7.1f} / {r[-1]:7.1f} G samples/s (min / median / max of {a.rounds})"
                f"   {base / statistics.median(sec[name]):5.3f} of the forward transform")
        for h in [fft, c2c, c2r, *synth.values(), *ana.values()]:
            h.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/ifft_rates.py on %s: 2^%d values per call, back-to-back calls at settled clocks, configurations alternated round by round\n" % (torch.cuda.get_device_name(0), a.log2))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
