"""Rational resampler rates on one MI355X (gr4hip_resamp_process; input and output resident in device memory).

    python tools/rational_resampler_rates.py [--out profiles/rational_resampler_rates.txt] [--log2 26] [--rounds 5] [--mid-gib 8]

The new path against the composition it replaces, fir_interpolator(L) -> gr4hip_decimate(M), in the same run, float and complex<float>, 2^26 input samples per call,
(L, M, K) in (3, 4, 96), (2, 3, 256), (25, 32, 800), (147, 160, 3528), (160, 147, 3840).  The composition's intermediate stream is L times the input; where that
passes --mid-gib it walks the call in pieces of whole cycles (the interpolator carries its history), which is what a user of the composition has to do as well.
Each figure is back-to-back calls at settled clocks (tools/_timing.py); the configurations are alternated round by round, min / median / max of `rounds` are
recorded, the ratio is median over median, and a shape passes when the resampler's median exceeds the composition's by more than the two spreads (max - min) combined.
The yardstick for bytes/s is a one-op gr4hip_ewise_process float program measured first.  Beside each ratio: the shape's share of its own bound -- the HBM bound
(4 + 4 M / L) S bytes per output at the yardstick's rate, or the LDS-read bound, (1 + 1 / R) Kp reads per output and lane (2 / R in the window form, decimate <= 4)
at 32 lanes per clock and CU, whichever is longer (R = 4 cycles per tap read; CU count and clock from the device properties)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402

SHAPES = [(3, 4, 96), (2, 3, 256), (25, 32, 800), (147, 160, 3528), (160, 147, 3840)]
R = 4  # cycles per lane and tap read in fir_resamp_kernel


def lowpass(K, L, M):
    k = np.arange(K, dtype=np.float64)
    fc = 0.4 / max(L, M)
    h = (0.54 - 0.46 * np.cos(2 * np.pi * k / (K - 1))) * 2 * fc * np.sinc(2 * fc * (k - (K - 1) / 2))
    return (h / h.sum()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rational_resampler_rates.txt"))
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mid-gib", type=float, default=8.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a rate is measured on the GPU or not at all"
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    props = torch.cuda.get_device_properties(0)
    lds_lanes_per_s = props.multi_processor_count * 32 * getattr(props, "clock_rate", 2400000) * 1e3  # ds_read_b32 / b64: 32 lanes per clock and CU (clock in kHz; 2.4 GHz where torch does not say)
    n0 = 1 << a.log2
    xf = torch.randn(n0, device="cuda")
    yf = torch.empty_like(xf)
    ew = G.Merged(torch.float32, [("Multiply", 1.0001)])
    ys = sorted(8 * n0 / steady(lambda: ew.process_bulk(xf, out=yf)) for _ in range(a.rounds))
    hbm = statistics.median(ys)
    say(f"yardstick: one-op ewise program, float, 2^{a.log2} samples: {ys[0] / 1e12:.3f} / {hbm / 1e12:.3f} / {ys[-1] / 1e12:.3f} TB/s (min / median / max of {a.rounds})")
    del xf, yf

    all_pass = True
    for dtype, S, tname in ((torch.float32, 1, "float"), (torch.complex64, 2, "complex<float>")):
        for L, M, K in SHAPES:
            n = n0 // M * M
            n_out = n // M * L
            b = lowpass(K, L, M)
            g = torch.Generator(device="cuda").manual_seed(1)
            x = torch.randn(n, device="cuda", generator=g) if S == 1 else torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=g) * 0.70710678)
            y = torch.empty(n_out, dtype=dtype, device="cuda")
            rs = G.rational_resampler(b, L, M, dtype)
            ip = G.fir_interpolator(b, L, dtype)
            piece = max(M, min(n, int(a.mid_gib * 2 ** 30 / (4 * S * L)) // M * M))  # inputs per piece of the composition
            mid = torch.empty(piece * L, dtype=dtype, device="cuda")
            lib, did, st = G.capi.lib(), G.blocks._DTYPE_ID[dtype], torch.cuda.current_stream().cuda_stream

            def composed():
                for at in range(0, n, piece):
                    m = min(piece, n - at)
                    ip.process_bulk(x[at:at + m], out=mid)
                    G.capi.check(lib.gr4hip_decimate(did, mid.data_ptr(), m * L, M, y[at // M * L:].data_ptr(), None, st), "decimate")

            cases = [("rational_resampler", lambda: rs.process_bulk(x, out=y)), ("fir_interpolator -> decimate", composed)]
            sec = {name: [] for name, _ in cases}
            for _ in range(a.rounds):  # alternated: a drift of the machine reaches both alike
                for name, fn in cases:
                    sec[name].append(steady(fn))
            new, old = sorted(sec[cases[0][0]]), sorted(sec[cases[1][0]])
            mn, mo = statistics.median(new), statistics.median(old)
            # rates in outputs/s: spread = max - min of the rate
            rn, ro = sorted(n_out / s for s in new), sorted(n_out / s for s in old)
            ok = n_out / mn - n_out / mo > (rn[-1] - rn[0]) + (ro[-1] - ro[0])
            all_pass = all_pass and ok
            Kp = -(-K // L)
            t_hbm = n_out * (4 + 4 * M / L) * S / hbm
            t_lds = n_out * Kp * (2 / R if M <= 4 else 1 + 1 / R) / lds_lanes_per_s  # the window form (decimate <= 4) / the gather form
            bound, which = (t_hbm, "HBM") if t_hbm >= t_lds else (t_lds, "LDS reads")
            for name, r in ((cases[0][0], rn), (cases[1][0], ro)):
                say(f"{tname:<14} L {L:3d} M {M:3d} K {K:4d}  {name:<29} {r[0] / 1e9:8.2f} / {statistics.median(r) / 1e9:8.2f} / {r[-1] / 1e9:8.2f} G outputs/s (min / median / max of {a.rounds})")
            say(f"{tname:<14} L {L:3d} M {M:3d} K {K:4d}  ratio {mo / mn:6.2f}x  {'exceeds' if ok else 'DOES NOT exceed'} the composition by more than both spreads;"
                f"  {bound / mn:5.3f} of its {which} bound ({n_out / bound / 1e9:.1f} G outputs/s; HBM {n_out / t_hbm / 1e9:.1f}, LDS reads {n_out / t_lds / 1e9:.1f});"
                f"  composition in {-(-n // piece)} piece(s)")
            rs.close()
            ip.close()
            del x, y, mid
    say("every shape passes" if all_pass else "NOT every shape passes")

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/rational_resampler_rates.py on %s: 2^%d input samples per call, back-to-back calls at settled clocks, configurations alternated round by round\n"
                 % (torch.cuda.get_device_name(0), a.log2))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
