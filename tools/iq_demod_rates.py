"""IQDemodulator input-sample rates on one MI355X (gr4hip_iqdemod_process; both inputs resident in device memory) and the single-core rate of the reference's
per-sample loop.

    python tools/iq_demod_rates.py [--out profiles/iq_demod_rates.txt] [--quick]

Rows: float at C = 1024 (the registered Resampling<1024U>) on 2^20, 2^24 and 2^27 samples per input; float at C = 1 on 2^24; double at C = 1024 on 2^24;
all at the defaults (62.5 MHz, f_hp 100 Hz, f_lp 10 kHz, symmetric difference) on a 5 MHz carrier.  A sample is one ref and one resp value.  The traffic
column counts what the three passes read (3 x 2 inputs x sizeof(T)) plus the outputs; the fraction is that over the ~6.3 TB/s MI355X_MICROARCH.md gives as
achievable.  The CPU row, for scale, times the reference's loop (:519-567 and step 5 once per chunk, float, C = 1024) written out in C++, g++ -O2, one core.
--quick: the 2^24 float C = 1024 row only (for a rocprofv3 run)."""
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

ACHIEVABLE = 6.3e12

CPU_LOOP = r"""
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <numbers>
#include <vector>
int main() {
    const int n = 1 << 22, C = 1024;
    const float fs = 62.5e6f, eps = 1e-12f, pi = std::numbers::pi_v<float>;
    const float ahp = std::exp(-2.f * pi * 100.f / fs), alp = 1.f - std::exp(-2.f * pi * 10000.f / fs);
    std::vector<float> r(n), x(n), out(3 * (n / C));
    for (int i = 0; i < n; ++i) { r[i] = std::sin(0.5026f * i) + 0.1f; x[i] = 0.8f * std::sin(0.5026f * i + 0.5f) + 0.1f; }
    auto t0 = std::chrono::steady_clock::now();
    float hr = 0, hx = 0, vr = 0, vx = 0, s[5] = {}, h[4] = {}, g[4] = {};
    for (int i = 0; i < n; ++i) {
        hr = ahp * (hr + r[i] - vr); vr = r[i];
        hx = ahp * (hx + x[i] - vx); vx = x[i];
        h[3] = h[2]; h[2] = h[1]; h[1] = h[0]; h[0] = hr;
        g[3] = g[2]; g[2] = g[1]; g[1] = g[0]; g[0] = hx;
        const float rq = h[0] - h[2], ri = h[1], xi = g[1];
        const float p[5] = {xi * ri, xi * rq, ri * ri, rq * rq, xi * xi};
        for (int k = 0; k < 5; ++k) s[k] += alp * (p[k] - s[k]);
        if ((i + 1) % C == 0) {
            const float I = s[0], Q = s[1], Pr = s[2], Pd = s[3], Px = s[4];
            const float amp = (Pr > eps && Px > eps) ? std::sqrt(Px / Pr) : 0.f;
            float f = 0.f, ph = 0.f;
            if (Pr > eps && Pd > eps) {
                const float ratio = std::sqrt(Pd / Pr);
                float om0 = std::asin(std::clamp(ratio / 2.f, -1.f, 1.f));
                for (int it = 0; it < 3; ++it) {
                    const float om1 = std::asin(std::clamp(ratio / 2.f, -1.f, 1.f)), om2 = std::asin(std::clamp(ratio / 2.f, -1.f, 1.f)), om3 = std::asin(std::clamp(ratio / 2.f, -1.f, 1.f));
                    const float den = om3 - 2.f * om2 + om1;
                    om0 = std::abs(den) > eps ? om1 - (om2 - om1) * (om2 - om1) / den : om3;
                }
                f = om0 * fs / (2.f * pi);
                if (std::abs(I) > eps || std::abs(Q) > eps) ph = std::atan2(Q, I * ratio);
            }
            out[3 * (i / C)] = amp; out[3 * (i / C) + 1] = ph; out[3 * (i / C) + 2] = f;
        }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double chk = 0; for (float v : out) chk += v;
    std::printf("%.6e %.3f\n", n / sec, chk);
}
"""


def cpu_rate():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "iq.cpp"), os.path.join(d, "iq")
        open(src, "w").write(CPU_LOOP)
        subprocess.check_call(["g++", "-O2", "-std=c++20", src, "-o", exe])
        return float(subprocess.check_output([exe], text=True).split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_demod_rates.txt"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = [("float, C = 1024", torch.float32, 1024, 1 << 24)]
    if not a.quick:
        rows = [("float, C = 1024", torch.float32, 1024, 1 << 20), *rows, ("float, C = 1024", torch.float32, 1024, 1 << 27),
                 ("float, C = 1 (an output per sample)", torch.float32, 1, 1 << 24), ("double, C = 1024", torch.float64, 1024, 1 << 24)]
    lines = [f"# IQDemodulator rates, {torch.cuda.get_device_name(0)}, inputs resident in device memory (tools/iq_demod_rates.py)",
             "# variant | samples per call | Gsamples/s (one ref + one resp value per sample) | ms per call | traffic TB/s (3 reads of both inputs + outputs) | of 6.3 TB/s"]
    for name, dt, C, n in rows:
        w = 2 * np.pi * 5e6 / 62.5e6
        t = torch.arange(n, device="cuda", dtype=torch.float64) * w
        ref = (torch.sin(t) + 0.1).to(dt)
        resp = (0.8 * torch.sin(t + 0.5) + 0.1).to(dt)
        del t
        blk = G.IQDemodulator(dtype=dt, chunk=C)
        es = ref.element_size()
        outs = [torch.empty(n // C, dtype=dt, device="cuda") for _ in range(3)]
        sec = steady(lambda: blk.process_bulk(ref, resp, *outs))
        traffic = (3 * 2 * es + 3 * es / C) * n / sec
        lines.append(f"{name} | 2^{n.bit_length() - 1} | {n / sec / 1e9:.2f} | {sec * 1e3:.3f} | {traffic / 1e12:.2f} | {traffic / ACHIEVABLE:.3f}")
        del ref, resp, outs, blk
        torch.cuda.empty_cache()
    if not a.quick:
        r = cpu_rate()
        lines.append(f"reference loop, float, C = 1024, one CPU core (g++ -O2) | 2^22 | {r / 1e9:.4f} | - | - | -")
    text = "\n".join(lines) + "\n"
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
