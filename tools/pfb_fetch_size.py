"""FETCH_SIZE of the polyphase filter bank's kernels beside the FFT block's, in a counter run of its own (counters only, no tracing):

    rocprofv3 --pmc FETCH_SIZE -d DIR -o fetch --output-format csv -- python tools/pfb_fetch_size.py run
    python tools/pfb_fetch_size.py report DIR/fetch_counter_collection.csv [--out profiles/pfb_fetch_size.txt]

`run` is the workload: |X|^2 at N in {1024, 8192}, the FFT block (Hann, fft_fast_kernel: frame pipeline off) and the bank at P = 1 / 4 / 8, two calls of 2^25 samples
each; at N = 8192, P = 4 the simple form and then the run form (the call's frames dealt evenly over one workgroup per CU:
16 per run on 256 CUs).  `report` takes the second call of each and writes FETCH_SIZE as the tool gives it (KiB per dispatch)
and relative to the FFT block's kernel of the same N."""
import argparse
import csv
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOG2 = 25
SIZES, TAPS = (1024, 8192), (1, 4, 8)


def labels():
    out = []
    for N in SIZES:
        out.append((N, "FFT block (fft_fast_kernel)"))
        for P in TAPS:
            out.append((N, f"bank P {P}"))
            if N == 8192 and P == 4:
                out.append((N, f"bank P {P}, run form"))
    return out


def run():
    import torch
    import gnuradio4_amd as G
    n = 1 << LOG2
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=g) * 0.70710678)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    hook = G.capi.lib().gr4hip_internal_pfb_set_run_length
    hook.argtypes, hook.restype = [ctypes.c_void_p, ctypes.c_long], ctypes.c_int
    G.capi.developer_switch("GR4HIP_FFT_NO_PIPELINE", 1)
    for N in SIZES:
        f = G.FFT(N, "Hann")
        for _ in range(2):
            f.mag2(x, out=out)
        for P in TAPS:
            b = G.PolyphaseFilterBank(N, P)
            for form in ((0, -(-(n // N) // torch.cuda.get_device_properties(0).multi_processor_count)) if N == 8192 and P == 4 else (0,)):
                hook(b._h, form)
                for _ in range(2):
                    b.power(x, out=out)
    torch.cuda.synchronize()


def report(path, out):
    rows = [r for r in csv.DictReader(open(path)) if r["Counter_Name"] == "FETCH_SIZE" and any(k in r["Kernel_Name"] for k in ("fft_fast_kernel", "pfb_fast_kernel", "pfb_run_kernel"))]
    lab = labels()
    assert len(rows) == 2 * len(lab), (len(rows), len(lab))
    lines = ["# tools/pfb_fetch_size.py: rocprofv3 --pmc FETCH_SIZE (counters only), |X|^2, 2^%d samples per call, the second of two calls; KiB per dispatch as the tool reports it" % LOG2]
    base = {}
    for i, (N, name) in enumerate(lab):
        v = float(rows[2 * i + 1]["Counter_Value"])
        if name.startswith("FFT"):
            base[N] = v
        lines.append(f"N {N:5d} {name:<28} {rows[2 * i + 1]['Kernel_Name'].split('(')[0].replace('void ', ''):<34} FETCH_SIZE {v:10.0f} KiB   {v / base[N]:5.3f} of the FFT block")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report"])
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfb_fetch_size.txt"))
    a = ap.parse_args()
    run() if a.mode == "run" else report(a.csv, a.out)
