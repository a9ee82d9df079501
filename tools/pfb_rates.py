"""Polyphase filter bank rates on one MI355X (gr4hip_pfb_process; input and outputs resident in device memory).

    python tools/pfb_rates.py [--out profiles/pfb_rates.txt] [--log2 27] [--rounds 5] [--sizes 1024 8192]

|X|^2 and the spectrum at N in {1024, 8192} channels, P in {1, 4, 8} taps per channel, 2^27 samples per call.  The yardstick, measured in the same run and
alternated with the bank round by round: gr4hip_fft_mag2 / gr4hip_fft_spectrum with the Hann window at the same N -- existing code, the same HBM bytes per sample
(8 in; 4 or 8 out).  At N = 8192 the FFT block sends calls of >= 256 frames to the frame pipeline of the fused chain kernel; the row "fft_fast_kernel" is the
FFT block with that pipeline switched off (GR4HIP_FFT_NO_PIPELINE): the kernel whose passes the bank runs; and at P = 4 the run form of the same handle (test hook
gr4hip_internal_pfb_set_run_length) is measured beside the default.
Each figure is back-to-back calls at settled clocks (tools/_timing.py); every configuration is measured `rounds` times, min / median / max are recorded, and the
ratio is median over median.  The float64 oracle (tests/pfb_oracle.py) is timed on one host core at 2^20 samples.  FIRST MEASUREMENTS: no threshold decides anything."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
import pfb_oracle as PO  # noqa: E402
from _timing import steady  # noqa: E402


def run_length(bank, frames):
    """the library's test hook: frames per workgroup of the run form (0: the simple form, the default)"""
    fn = G.capi.lib().gr4hip_internal_pfb_set_run_length
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_long], ctypes.c_int
    assert fn(bank._h, frames) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfb_rates.txt"))
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 8192])
    a = ap.parse_args()
    n = 1 << a.log2
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=g) * 0.70710678)
    spec = torch.empty(n, dtype=torch.complex64, device="cuda")
    mag2 = torch.empty(n, dtype=torch.float32, device="cuda")

    for N in a.sizes:
        fft = G.FFT(N, "Hann")
        banks = {P: G.PolyphaseFilterBank(N, P) for P in (1, 4, 8)}
        for what, out in (("|X|^2", mag2), ("spectrum", spec)):
            power = what == "|X|^2"
            cases = [("FFT block, Hann", lambda: (fft.mag2 if power else fft.spectrum)(x, out=out), None)]
            if N == 8192:
                cases.append(("FFT block, Hann, fft_fast_kernel (frame pipeline off)", lambda: (fft.mag2 if power else fft.spectrum)(x, out=out), "GR4HIP_FFT_NO_PIPELINE"))
            for P, b in banks.items():
                cases.append((f"polyphase filter bank P {P}", lambda b=b: (b.power if power else b.process_bulk)(x, out=out), None))
                if N == 8192 and 2 <= P <= 4:  # the run form of the same handle beside it: the call's frames dealt evenly over one workgroup per CU
                    cases.append((f"polyphase filter bank P {P}, run form", lambda b=b: (b.power if power else b.process_bulk)(x, out=out), b))
            sec = {name: [] for name, _, _ in cases}
            for _ in range(a.rounds):  # alternated: a drift of the machine reaches every configuration alike
                for name, fn, switch in cases:
                    if isinstance(switch, str):
                        G.capi.developer_switch(switch, 1)
                    elif switch is not None:
                        run_length(switch, -(-(n // N) // torch.cuda.get_device_properties(0).multi_processor_count))
                    sec[name].append(steady(fn))
                    if isinstance(switch, str):
                        G.capi.developer_switch(switch, 0)
                    elif switch is not None:
                        run_length(switch, 0)
            base = statistics.median(sec[cases[0][0]])
            for name, _, _ in cases:
                r = sorted(n / s / 1e9 for s in sec[name])
                say(f"N {N:5d} {what:<8} {name:<56} {r[0]:7.1f} / {statistics.median(r):7.1f} / {r[-1]:7.1f} G samples/s (min / median / max of {a.rounds})"
                    f"   {base / statistics.median(sec[name]):5.3f} of the FFT block")
        fft.close()
        for b in banks.values():
            b.close()

    # the oracle on one host core (numpy's transform is single-threaded; the sums are numpy element-wise loops)
    m = 1 << 20
    xh = x[:m].cpu().numpy()
    for N, P in ((1024, 4), (8192, 8)):
        h = PO.design(N, P)
        t0 = time.perf_counter()
        PO.pfb(h, xh, N, P)
        dt = time.perf_counter() - t0
        say(f"N {N:5d} float64 oracle (tests/pfb_oracle.py), P {P}, 2^20 samples, one host core: {m / dt / 1e6:7.1f} M samples/s")

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/pfb_rates.py on %s: 2^%d samples per call, back-to-back calls at settled clocks, configurations alternated round by round\n" % (torch.cuda.get_device_name(0), a.log2))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
