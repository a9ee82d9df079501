"""Complex-tap FIR rates on one MI355X (gr4hip_cfir_process; input and output resident in device memory).

    python tools/complex_fir_rates.py [--out profiles/complex_fir_rates.txt] [--log2 24 26]

complex_fir_filter at K in {64, 256, 1024} taps, decimate 1 and 8, on 2^24 and 2^26 samples (unit noise: no segment is marked), G INPUT samples/s and the useful
TFLOP/s (8 K / D flop per input sample); the same with every segment marked (a stop-band tone 60 dB up: the float64 second evaluation runs everywhere).
Measured in the same run, from the library's unchanged real-tap paths:
 (i)  fir_filter<complex> under GR4HIP_FIR_TIME_DOMAIN_F32 with 2 K real taps: the same flop count per sample on the same arithmetic tier (f32 matrix pipe);
 (ii) Rotator -> real-tap decimate-by-8 fir_filter<complex> (rotation at the input rate, the f16-split decimator) against complex taps h[k] e^{jwk} -> Rotator at the
      output rate (complex_fir_filter + Rotator on an eighth of the samples).
Each rate is back-to-back calls at settled clocks (tools/_timing.py).  FIRST MEASUREMENTS: no threshold decides anything."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402


def lowpass(K, fc):
    i = np.arange(K) - (K - 1) / 2.0
    h = (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(K) / max(K - 1, 1))) * 2 * fc * np.sinc(2 * fc * i)
    return (h / h.sum()).astype(np.float32)


def ctaps(K, D, shift=0.2):
    return (lowpass(K, 0.4 / (2 * D)).astype(np.float64) * np.exp(2j * np.pi * shift * np.arange(K))).astype(np.complex64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complex_fir_rates.txt"))
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    a = ap.parse_args()
    lines = []

    def row(name, sec, n_in, flop_per_in):
        lines.append(f"{name:<86} {n_in / sec / 1e9:9.2f} G input samples/s {flop_per_in * n_in / sec / 1e12:7.2f} TFLOP/s")
        print(lines[-1], flush=True)

    nmax = 1 << max(a.log2)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn(nmax, 2, device="cuda", generator=g) * 0.70710678)
    tone = torch.polar(torch.full((nmax,), 1000.0, device="cuda"), (torch.arange(nmax, device="cuda") % 10).float() * (-0.6 * np.pi))  # -0.3 fs: ten samples per three turns
    y = torch.empty(nmax, dtype=torch.complex64, device="cuda")
    z = torch.empty(nmax, dtype=torch.complex64, device="cuda")

    for D in (1, 8):
        for K in (64, 256, 1024):
            f = G.complex_fir_filter(ctaps(K, D), D)
            for l in a.log2:
                n = 1 << l
                row(f"complex_fir_filter K {K:4d} D {D}, 2^{l}", steady(lambda: f.process_bulk(x[:n], out=y)), n, 8.0 * K / D)
            f.close()
    xt = x + tone  # every segment marked
    for D, K in ((1, 256), (8, 256)):
        f = G.complex_fir_filter(ctaps(K, 8), D)
        n = 1 << min(a.log2)
        row(f"complex_fir_filter K {K:4d} D {D}, 2^{min(a.log2)}, every segment marked (float64 redo)", steady(lambda: f.process_bulk(xt[:n], out=y)), n, 8.0 * K / D)
        f.close()
    del xt, tone

    # (i) the real-tap filter with 2 K taps on float32 products
    for K2 in (128, 512):
        f = G.fir_filter(lowpass(K2, 0.2), torch.complex64)
        f.set_algo(G.capi.FIR_TIME_DOMAIN_F32)
        for l in a.log2:
            n = 1 << l
            row(f"(i) fir_filter<complex> TIME_DOMAIN_F32, {K2} real taps (= K {K2 // 2}), 2^{l}", steady(lambda: f.process_bulk(x[:n], out=y)), n, 4.0 * K2)
        f.close()

    # (ii) the frequency-translating decimator, both ways
    w = np.float32(2 * np.pi * 0.2)
    for K in (128, 256):
        h = lowpass(K, 0.4 / 16)
        rot_in, fir = G.Rotator(phase_increment=float(-w)), G.fir_filter(h, torch.complex64, 8)
        cf = G.complex_fir_filter((h.astype(np.float64) * np.exp(1j * float(w) * np.arange(K))).astype(np.complex64), 8)
        rot_out = G.Rotator(phase_increment=float(np.float32(-8) * w), initial_phase=float(np.float32(7) * w))
        for l in a.log2:
            n = 1 << l

            def old():
                rot_in.process_bulk(x[:n], out=z)
                fir.process_bulk(z[:n], out=y)

            def new():
                cf.process_bulk(x[:n], out=z)
                rot_out.process_bulk(z[:n // 8], out=y)
            row(f"(ii) Rotator -> real-tap decimate-by-8 fir_filter<complex>, K {K}, 2^{l}", steady(old), n, 0.0)
            row(f"(ii) complex taps decimate-by-8 -> Rotator at the output rate, K {K}, 2^{l}", steady(new), n, 0.0)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/complex_fir_rates.py on %s: back-to-back calls at settled clocks; rates in INPUT samples; TFLOP/s = useful flop (8 K / D per input sample; (i): 4 taps)\n" % torch.cuda.get_device_name(0))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
