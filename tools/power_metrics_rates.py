"""PowerMetrics input rates on one MI355X (gr4hip_powermetrics_process; inputs and outputs resident in device memory) and the single-core rate of the
reference's per-sample loop.

    python tools/power_metrics_rates.py [--out profiles/power_metrics_rates.txt] [--quick]

Rows: 2^24 and 2^27 samples per input row, decimate 1 and 100, one and three phases, at the defaults (10 kHz, 2 Hz, 90 Hz) on a 50 Hz system.  A phase-sample
is one voltage and one current value of one phase (8 B).  The HBM column is that traffic read ONCE over the ~6.3 TB/s MI355X_MICROARCH.md gives as
achievable; the three passes of a call read it three times, and decimate 1 also writes 20 B per phase-sample.  Each rate is back-to-back launches at settled
clocks (tools/_timing.py).  The CPU row, for scale, times the reference's loop (PowerEstimators.hpp:101-127, float, decimate 100) written out in C++, g++ -O2,
one core.  --quick [K]: the 2^K (default 2^24), decimate 100, one-phase row only, nothing written (for a rocprofv3 run)."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402
from gnuradio4_amd import capi  # noqa: E402

ACHIEVABLE = 6.3e12

CPU_LOOP = r"""
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>
struct Biquad { float b[3], a[3], w1 = 0, w2 = 0;
    float step(float x) { const float w = x - (a[1] * w1 + a[2] * w2); const float y = b[0] * w + b[1] * w1 + b[2] * w2; w2 = w1; w1 = w; return y; } };
int main() {
    const int n = 1 << 22, D = 100;
    std::vector<float> u(n), c(n), out(5 * (n / D));
    for (int i = 0; i < n; ++i) { u[i] = 325.f * std::sin(0.0314159f * i) + 1.f; c[i] = 14.1f * std::sin(0.0314159f * i - 0.1f) - 1.f; }
    Biquad hu{{0.99911183f, -1.99822366f, 0.99911183f}, {1.f, -1.99822283f, 0.99822438f}}, hi = hu;
    Biquad lp{{0.00096524f, 0.f, 0.f}, {1.f, -1.9555819f, 0.95654714f}}, lu = lp, li = lp;
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) {
        const float x = hu.step(u[i]), y = hi.step(c[i]);
        const float ep = lp.step(x * y), eu = lu.step(x * x), ei = li.step(y * y);
        if (i % D == 0) {
            const float ur = std::sqrt(eu), ir = std::sqrt(ei), S = ur * ir, Q = std::sqrt(std::max(S * S - ep * ep, 0.f));
            float* o = &out[5 * (i / D)];
            o[0] = ep; o[1] = Q; o[2] = S; o[3] = ur; o[4] = ir;
        }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double chk = 0; for (float v : out) chk += v;
    std::printf("%.6e %.3f\n", n / sec, chk);
}
"""


def cpu_rate():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "pm.cpp"), os.path.join(d, "pm")
        open(src, "w").write(CPU_LOOP)
        subprocess.check_call(["g++", "-O2", "-std=c++20", src, "-o", exe])
        return float(subprocess.check_output([exe], text=True).split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_metrics_rates.txt"))
    ap.add_argument("--quick", nargs="?", type=int, const=24, default=None, metavar="K")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = [(1 << a.quick, 100, 1)] if a.quick else [(n, D, ph) for n in (1 << 24, 1 << 27) for D in (100, 1) for ph in (1, 3)]
    lines = [f"# PowerMetrics rates, {torch.cuda.get_device_name(0)}, inputs and outputs resident in device memory (tools/power_metrics_rates.py)",
             "# samples per row | decimate | phases | Gsamples/s per phase-sample (one u + one i value) | ms per call | of 6.3 TB/s at 8 B per phase-sample read once"]
    st = torch.cuda.current_stream().cuda_stream
    for n2, D, ph in rows:
        n = n2 // D * D  # (a call takes whole chunks: 2^k rounded down to a multiple of decimate)
        t = torch.arange(n, device="cuda", dtype=torch.float64) * (2 * np.pi * 50.0 / 1e4)
        u = torch.stack([(325.0 * torch.sin(t + 2.1 * k) + 1.0).float() for k in range(ph)])
        i = torch.stack([(14.1 * torch.sin(t + 2.1 * k - 0.1 * (k + 1)) - 1.0).float() for k in range(ph)])
        del t
        blk = G.PowerMetrics(n_phases=ph, decimate=D)
        no = n // D
        outs = [torch.empty((ph, no), dtype=torch.float32, device="cuda") for _ in range(5)]
        ptr = [o.data_ptr() for o in outs]

        def call():
            rc = capi.lib().gr4hip_powermetrics_process(blk._h, u.data_ptr(), i.data_ptr(), n, n, *ptr, no, None, st)
            assert rc == 0, (rc, capi.lib().gr4hip_last_error().decode())
        sec = steady(call)
        rate = n * ph / sec
        lines.append(f"2^{n2.bit_length() - 1} | {D} | {ph} | {rate / 1e9:.2f} | {sec * 1e3:.3f} | {rate * 8 / ACHIEVABLE:.3f}")
        del u, i, outs, blk
        torch.cuda.empty_cache()
    if not a.quick:
        r = cpu_rate()
        lines.append(f"reference loop, float, decimate 100, one phase, one CPU core (g++ -O2) | 2^22 | - | {r / 1e9:.4f} | - | -")
    text = "\n".join(lines) + "\n"
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
