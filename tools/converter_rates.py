"""Converter rates on one MI355X (gr4hip_convert_process; inputs and outputs resident in device memory).

    python tools/converter_rates.py [--out profiles/converter_rates.txt] [--log2 27]

Rows at 2^27 items: Gsamples/s and TB/s moved (bytes read + bytes written) for the int16 -> complex<float> ingest, Convert<float, int16>, ToMagPhase<complex<float>>,
Abs<complex<float>>, Convert<uint8, double>, two rows with ports whose misalignments disagree (the narrower port then moves element by element), and the ingest run with MultiplyConst -> Rotator absorbed against the same three blocks as three launches.  The
yardstick, measured in the same run, is a one-op gr4hip_ewise_process float program of the same size: the library's existing streaming kernel, "as fast as a copy
of these bytes can go".  The last rows feed the ingest from pinned host memory: int16 over the link with the converter on the device, against the same stream
converted on the host and fed as complex<float>.  Each rate is back-to-back calls at settled clocks (tools/_timing.py).  FIRST MEASUREMENTS: no threshold decides
anything."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "converter_rates.txt"))
    ap.add_argument("--log2", type=int, default=27)
    a = ap.parse_args()
    n = 1 << a.log2
    rows = []

    def row(name, fn, items, nbytes):
        sec = steady(fn)
        rows.append((name, items / sec / 1e9, nbytes / sec / 1e12))
        print(f"{name:<72} {rows[-1][1]:9.2f} Gsamples/s {rows[-1][2]:7.3f} TB/s", flush=True)

    xf = torch.randn(n, device="cuda")
    yf = torch.empty_like(xf)
    ew = G.Merged(torch.float32, [("Multiply", 1.0001)])
    row("yardstick: one-op ewise program, float", lambda: ew.process_bulk(xf, out=yf), n, 8 * n)

    xi = torch.randint(-32768, 32767, (2 * n,), dtype=torch.int16, device="cuda")
    yc = torch.empty(n, dtype=torch.complex64, device="cuda")
    ingest = G.InterleavedToComplex(torch.int16, torch.complex64)
    row("InterleavedToComplex<int16, complex<float>> (ingest)", lambda: ingest.process_bulk(xi, out=yc), n, 12 * n)
    row("the ingest, output one sample off its input's alignment (input element-wise)", lambda: ingest.process_bulk(xi[:2 * n - 2], out=yc[1:]), n - 1, 12 * (n - 1))
    yi = torch.empty(n, dtype=torch.int16, device="cuda")
    narrow = G.Convert(torch.float32, torch.int16)
    row("Convert<float, int16>", lambda: narrow.process_bulk(xf, out=yi), n, 6 * n)
    xc = torch.randn(n, dtype=torch.complex64, device="cuda")
    m, p = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    tmp = G.ToMagPhase(torch.complex64)
    row("Convert<float, int16>, output one element off (output element-wise)", lambda: narrow.process_bulk(xf[:n - 1], out=yi[1:]), n - 1, 6 * (n - 1))
    row("ToMagPhase<complex<float>>", lambda: tmp.process_bulk(xc, out=[m, p]), n, 16 * n)
    ab = G.Abs(torch.complex64)
    row("Abs<complex<float>>", lambda: ab.process_bulk(xc, out=m), n, 12 * n)
    del xc, m, p
    xb = torch.randint(0, 255, (n,), dtype=torch.uint8, device="cuda")
    yd = torch.empty(n, dtype=torch.float64, device="cuda")
    wide = G.Convert(torch.uint8, torch.float64)
    row("Convert<uint8, double>", lambda: wide.process_bulk(xb, out=yd), n, 9 * n)
    del xb, yd

    gain, rot = ("Multiply", 1.0 / 32768), ("Rotator", 0.0123)
    fused = G.InterleavedToComplex(torch.int16, torch.complex64)
    fused.set_epilogue(G.Merged(torch.complex64, [gain, rot]))
    row("ingest -> MultiplyConst -> Rotator, one launch", lambda: fused.process_bulk(xi, out=yc), n, 12 * n)
    g1, g2 = G.Merged(torch.complex64, [gain]), G.Merged(torch.complex64, [rot])
    y2 = torch.empty_like(yc)

    def three():
        ingest.process_bulk(xi, out=yc)
        g1.process_bulk(yc, out=y2)
        g2.process_bulk(y2, out=yc)
    row("ingest -> MultiplyConst -> Rotator, three launches", three, n, 12 * n + 32 * n)

    nh = min(n, 1 << 25)  # host-fed: pinned memory over the link
    hi = torch.randint(-32768, 32767, (2 * nh,), dtype=torch.int16).pin_memory()
    hc = torch.view_as_complex(hi.to(torch.float32).reshape(nh, 2).contiguous()).pin_memory()

    def fed_int16():
        xi[:2 * nh].copy_(hi, non_blocking=True)
        fused.process_bulk(xi[:2 * nh], out=yc[:nh])

    g12 = G.Merged(torch.complex64, [gain, rot])  # the same device work behind the link: gain and rotator as one program

    def fed_c32():
        y2[:nh].copy_(hc, non_blocking=True)
        g12.process_bulk(y2[:nh], out=yc[:nh])
    row("host-fed int16 I/Q (4 B/sample over the link), converter on the device", fed_int16, nh, 4 * nh)
    row("host-fed complex<float> (8 B/sample over the link), converted on the host", fed_c32, nh, 8 * nh)

    with open(a.out, "w") as f:
        f.write(f"# {torch.cuda.get_device_name(0)}; 2^{a.log2} items per call (host-fed rows: 2^{nh.bit_length() - 1}); FIRST MEASUREMENTS, no threshold decides anything\n")
        f.write(f"# yardstick bytes/s: {rows[0][2]:.3f} TB/s (one-op gr4hip_ewise_process float program, same run); host-fed rows count link bytes\n")
        for name, gs, tb in rows:
            f.write(f"{name:<72} {gs:9.2f} Gsamples/s {tb:7.3f} TB/s  ({100 * tb / rows[0][2]:5.1f} % of the yardstick's bytes/s)\n")


if __name__ == "__main__":
    main()
