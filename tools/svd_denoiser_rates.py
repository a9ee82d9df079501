"""SvdDenoiser input rates on one MI355X (gr4hip_svddenoise_process; input and output resident in device memory) and the single-core rate of the numpy oracle.

    python tools/svd_denoiser_rates.py [--out profiles/svd_denoiser_rates.txt] [--quick [K]]

Rows: float and complex<float> at 2^20 and 2^24 samples with the default settings (W 64, 32 x 33, hop 16, full rank) and with W 64, max_rank 3,
energy_fraction 0.95; and hop_fraction 1 / 64 (one SVD per sample) at 2^20 samples.  The input is a sinusoid in noise (sin(2 pi 0.05 t) + 0.3 N; complex:
exp(2 pi i t / 16) + 0.1 CN).  Each rate is back-to-back calls at settled clocks (tools/_timing.py); every call continues the stream of the one before.
Sweeps per window come from the handle's counter.  The float64 operations per window are counted for the sweeps only: pairs x (three dot products + one rotation)
= n (n - 1) / 2 x 12 m for real samples, x 38 m for complex ones, per sweep; the share is of the 78.6 TFLOP/s FP64 vector peak.
The CPU rows, for scale: the oracle's per-window work (numpy.linalg.svd, the rank rule, the low-rank product and the anti-diagonal average;
tests/svd_denoiser_oracle.low_rank_window) on 2^16 samples of the same input, one core.  --quick [K]: the float default row at 2^K (default 2^20) only, nothing written."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
import svd_denoiser_oracle as SV  # noqa: E402
from _timing import steady  # noqa: E402
from gnuradio4_amd import capi  # noqa: E402

FP64_PEAK = 78.6e12
SETTINGS = {"defaults": dict(), "rank 3": dict(window_size=64, max_rank=3, energy_fraction=0.95), "hop 1": dict(hop_fraction=1.0 / 64)}


def stream(n, cplx):
    g = torch.Generator(device="cuda").manual_seed(7)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    if cplx:
        nz = torch.randn(n, 2, device="cuda", generator=g, dtype=torch.float64) * (0.1 / np.sqrt(2))
        return (torch.exp(2j * np.pi * t / 16) + torch.view_as_complex(nz)).to(torch.complex64)
    return (torch.sin(2 * np.pi * 0.05 * t) + 0.3 * torch.randn(n, device="cuda", generator=g, dtype=torch.float64)).to(torch.float32)


def flops_per_sweep(m, n, cplx):
    return n * (n - 1) // 2 * (38 if cplx else 12) * m


def cpu_rate(x, dtype, settings):
    s = SV.defaults(dtype)
    s.update(settings)
    g = SV.derive(dtype, **s)
    W, hop = g["W"], g["hop"]
    xp = np.concatenate([np.zeros(W - 1, dtype=x.dtype), x]).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    t0 = time.perf_counter()
    for n in range(0, x.size, hop):
        SV.low_rank_window(xp[n:n + W], g["L"], SV.REAL_OF[dtype], **s)
    return x.size / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_denoiser_rates.txt"))
    ap.add_argument("--quick", nargs="?", type=int, const=20, default=None, metavar="K")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.quick:
        rows = [("f32", 1 << a.quick, "defaults")]
    else:
        rows = [(dt, n, s) for dt in ("f32", "c32") for s in ("defaults", "rank 3") for n in (1 << 20, 1 << 24)] + [(dt, 1 << 20, "hop 1") for dt in ("f32", "c32")]
    lines = [f"# SvdDenoiser rates, MI355X ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}), input and output resident in device memory (tools/svd_denoiser_rates.py)",
             "# type | samples | settings | hop | windows per call | Msamples/s | ms per call | sweeps per window | Mflop (float64) per window in the sweeps | of the 78.6 TFLOP/s FP64 vector peak"]
    st = torch.cuda.current_stream().cuda_stream
    torch_of = {"f32": torch.float32, "c32": torch.complex64}
    for dt, n, sname in rows:
        x = stream(n, dt[0] == "c")
        y = torch.empty_like(x)
        blk = G.SvdDenoiser(torch_of[dt], **SETTINGS[sname])
        geom = SV.derive(dt, **{**SV.defaults(dt), **SETTINGS[sname]})

        def call():
            rc = capi.lib().gr4hip_svddenoise_process(blk._h, x.data_ptr(), n, y.data_ptr(), st)
            assert rc == 0, (rc, capi.lib().gr4hip_last_error().decode())
        sec = steady(call, warm_s=0.02, time_s=0.05, min_reps=2)
        windows, bad = blk.stats()
        assert bad == 0, bad
        sweeps = blk.sweeps() / windows
        m, nn = max(geom["L"], geom["K"]), min(geom["L"], geom["K"])
        mflop = sweeps * flops_per_sweep(m, nn, dt[0] == "c") / 1e6
        per_call = n // geom["hop"]
        lines.append(f"{'float' if dt == 'f32' else 'complex<float>'} | 2^{n.bit_length() - 1} | {sname} | {geom['hop']} | {per_call} | {n / sec / 1e6:.1f} | {sec * 1e3:.2f} | "
                     f"{sweeps:.2f} | {mflop:.2f} | {mflop * 1e6 * per_call / sec / FP64_PEAK:.3f}")
        print(lines[-1], flush=True)
        del x, y, blk
        torch.cuda.empty_cache()
    if not a.quick:
        for dt in ("f32", "c32"):
            xs = stream(1 << 16, dt[0] == "c").cpu().numpy()
            for sname in ("defaults", "rank 3"):
                r = cpu_rate(xs, dt, SETTINGS[sname])
                lines.append(f"numpy oracle, {'float' if dt == 'f32' else 'complex<float>'}, one CPU core | 2^16 | {sname} | - | - | {r / 1e6:.4f} | - | - | - | -")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
