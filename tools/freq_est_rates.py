"""FrequencyEstimator input-sample rates on one MI355X (gr4hip_freqest_process; input resident in HBM) and the single-core rate of the reference's arithmetic.

    python tools/freq_est_rates.py [--out profiles/freq_est_rates.txt] [--n 4194304]

Rows: time domain C = 1 and C = 10 at the defaults (W = 100); frequency domain C = 1 at N = 256 (defaults) and N = 4096 (range 45-55 Hz, the reference QA's
setting); frequency domain C = N = 4096.  fraction of HBM peak = (4 B in + 4 B / C out) per input sample / time / 8 TB/s.  The CPU row, for scale, times the
time-domain block's per-sample loop (biquad + window sums, float) written out in C++ with the default geometry, g++ -O2, one core."""
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

HBM_PEAK = 8e12

# the time-domain estimator's per-sample loop (FrequencyEstimator.hpp:88-97, 120-164) in float, one core: the CPU scale for the device rows
CPU_TD = r"""
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>
int main() {
    const int W = 100, n = 1 << 18;
    const float b[3] = {0.0279f, 0.0558f, 0.0279f}, a[3] = {1.f, -1.48f, 0.59f}, eps = 1e-8f, fs = 1000.f;
    std::vector<float> x(n), y(n + 2, 0.f), out(n);
    for (int i = 0; i < n; ++i) x[i] = std::sin(0.316f * i);
    auto t0 = std::chrono::steady_clock::now();
    float prev = 50.f;
    for (int i = 2; i < n; ++i) {
        y[i] = (b[0] * x[i] + b[1] * x[i - 1] + b[2] * x[i - 2]) - (a[1] * y[i - 1] + a[2] * y[i - 2]);
        if (i < W) { out[i] = prev; continue; }
        float A = 0, B = 0, C = 0;
        for (int k = 1; k < W - 1; ++k) {
            const float s = y[i - k + 1] + y[i - k - 1], d = 4.f * y[i - k];
            if (std::fabs(d) < eps) continue;
            const float an = s * s / d, bn = y[i - k];
            A += an * an; B += bn * bn; C += 2.f * an * bn;
        }
        const float z = C / B - 1.f;
        if (B > eps && z < 1.f && z > -1.f) prev = fs / (4.f * 3.14159265f) * std::acos(z);
        out[i] = prev + 0.f * A;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double chk = 0; for (float v : out) chk += v;
    std::printf("%.6e %.3f\n", n / s, chk);
}
"""


def cpu_rate():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "td.cpp"), os.path.join(d, "td")
        open(src, "w").write(CPU_TD)
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe])
        return float(subprocess.check_output([exe], text=True).split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freq_est_rates.txt"))
    ap.add_argument("--n", type=int, default=1 << 22)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n = a.n
    x = (torch.sin(torch.arange(n, device="cuda", dtype=torch.float64) * (2 * np.pi * 50.3 / 1000.0)) + 0.01 * torch.randn(n, device="cuda", dtype=torch.float64)).float()
    rows = [
        ("time domain, C = 1 (defaults, W = 100)", G.FrequencyEstimatorTimeDomain, dict(chunk=1)),
        ("time domain, C = 10 (decimating)", G.FrequencyEstimatorTimeDomain, dict(chunk=10)),
        ("frequency domain, C = 1, N = 256 (defaults)", G.FrequencyEstimatorFrequencyDomain, dict(chunk=1)),
        ("frequency domain, C = 1, N = 4096 (45-55 Hz, QA setting)", G.FrequencyEstimatorFrequencyDomain, dict(chunk=1, min_fft_size=4096, f_min=45.0, f_max=55.0)),
        ("frequency domain, C = N = 4096 (decimating)", G.FrequencyEstimatorFrequencyDomain, dict(chunk=4096, min_fft_size=4096, f_min=45.0, f_max=55.0)),
    ]
    lines = [f"# FrequencyEstimator rates, {torch.cuda.get_device_name(0)}, {n} input samples per call, input resident in HBM (tools/freq_est_rates.py)",
             "# variant | Msamples/s (input) | ms per call | fraction of HBM peak (4 B in + 4 B / C out per sample, 8 TB/s)"]
    for name, cls, kw in rows:
        blk = cls(**kw)
        m = n // blk.chunk * blk.chunk
        out = torch.empty(m // blk.chunk, dtype=torch.float32, device="cuda")
        xs = x[:m]
        t = steady(lambda: blk.process_bulk(xs, out))
        frac = m * (4 + 4 / blk.chunk) / t / HBM_PEAK
        lines.append(f"{name} | {m / t / 1e6:.1f} | {t * 1e3:.3f} | {frac:.4f}")
    r = cpu_rate()
    lines.append(f"reference arithmetic, time domain C = 1, one CPU core (g++ -O2) | {r / 1e6:.2f} | - | -")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
