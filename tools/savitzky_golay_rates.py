"""Savitzky-Golay rates on one MI355X (gr4hip_savgol_zp_process and the streaming block on the FIR handles; rows resident in device memory).

    python tools/savitzky_golay_rates.py [--out profiles/savitzky_golay_rates.txt] [--log2 20 24]

Zero-phase float and double at W in {5, 11, 25, 51, 101} (p = 4, smoothing), one row of 2^20 and of 2^24 samples, and 16 rows of 2^20 in one call; the streaming
block at W = 11 on 2^24 samples; the CPU body of the DataSet block (numpy's correlate, one core) for scale.  Gsamples/s, TB/s moved (one read and one write per
sample) and float64 TFLOP/s counted as 2 W multiply-adds per sample (the halo's extra work is not counted).  The yardstick, measured in the same run, is a one-op
gr4hip_ewise_process float program: the library's existing streaming kernel.  Each rate is back-to-back calls at settled clocks (tools/_timing.py).
FIRST MEASUREMENTS: no threshold decides anything."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "savitzky_golay_rates.txt"))
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 24])
    a = ap.parse_args()
    rows = []

    def row(name, sec, items, nbytes, flops=0.0):
        rows.append((name, items / sec / 1e9, nbytes / sec / 1e12, flops / sec / 1e12))
        print(f"{name:<72} {rows[-1][1]:9.2f} Gsamples/s {rows[-1][2]:7.3f} TB/s {rows[-1][3]:6.2f} TFLOP/s", flush=True)

    n = 1 << max(a.log2)
    xf = torch.randn(n, device="cuda")
    yf = torch.empty_like(xf)
    ew = G.Merged(torch.float32, [("Multiply", 1.0001)])
    row("yardstick: one-op ewise program, float, 2^%d" % max(a.log2), steady(lambda: ew.process_bulk(xf, out=yf)), n, 8 * n)
    del xf, yf

    for dtype, es in ((torch.float32, 4), (torch.float64, 8)):
        for W in (5, 11, 25, 51, 101):
            blk = G.SavitzkyGolayDataSetFilter(dtype, W, 4, 0, "Reflect")
            for shape in [(1, 1 << l) for l in a.log2] + [(16, 1 << min(a.log2))]:
                x = torch.randn(shape, device="cuda", dtype=dtype)
                y = torch.empty_like(x)
                items = x.numel()
                name = f"zero-phase {str(dtype).split('.')[1]} W {W:3d}, {shape[0]} x 2^{shape[1].bit_length() - 1}"
                row(name, steady(lambda: blk.process(x, out=y)), items, 2 * es * items, 4.0 * W * items)
                del x, y
            blk.close()

    n = 1 << max(a.log2)
    for dtype, es in ((torch.float32, 4), (torch.float64, 8)):
        blk = G.SavitzkyGolayFilter(dtype, 11, 4, 0, 1.0, "Centred")
        x = torch.randn(n, device="cuda", dtype=dtype)
        y = torch.empty_like(x)
        row(f"streaming {str(dtype).split('.')[1]} W  11, 2^{max(a.log2)}", steady(lambda: blk.process_bulk(x, out=y)), n, 2 * es * n, 2.0 * 11 * n)
        blk.close()
        del x, y

    # the CPU body for scale: two correlations of a float64 row on one core (numpy; the boundary samples are not the cost)
    m = 1 << min(a.log2)
    c, _ = G.design_savitzky_golay(torch.float64, 11, 4)
    xs = np.random.default_rng(1).standard_normal(m)
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        np.correlate(np.correlate(xs, c, "same"), c[::-1], "same")
    row("host: numpy correlate twice, float64 W 11, one core, 2^%d" % min(a.log2), (time.perf_counter() - t0) / reps, m, 16 * m, 2.0 * 2 * 11 * m)

    with open(a.out, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}; FIRST MEASUREMENTS, no threshold decides anything\n")
        fh.write(f"# yardstick bytes/s: {rows[0][2]:.3f} TB/s (one-op gr4hip_ewise_process float program, same run); TFLOP/s: 2 W float64 multiply-adds per sample (streaming: W)\n")
        for name, gs, tb, tf in rows:
            fh.write(f"{name:<72} {gs:9.3f} Gsamples/s {tb:7.3f} TB/s {tf:6.2f} TFLOP/s  ({100 * tb / rows[0][2]:5.1f} % of the yardstick's bytes/s)\n")


if __name__ == "__main__":
    main()
