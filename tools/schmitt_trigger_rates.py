"""SchmittTrigger input rates on one MI355X (gr4hip_schmitt_process; input and edge list resident in device memory) and the single-core rate of the
reference's per-sample loop.

    python tools/schmitt_trigger_rates.py [--out profiles/schmitt_trigger_rates.txt] [--quick [K] [--dense] [--method M]]

Rows: float and int16 at 2^24 and 2^27 samples, the three methods, on a sparse stream (a sine at fs/1000, two edges per 1000 samples) and on the dense one
(alternating +-2 against a band of +-1: every sample is an edge, and the call writes 24 B per sample).  The call reads its input twice (the summary and the
apply pass), so the bound column is 2 sizeof(T) B per sample over the ~6.3 TB/s MI355X_MICROARCH.md gives as achievable.  Each rate is back-to-back calls at
settled clocks (tools/_timing.py).  The CPU rows, for scale, time processOne (SchmittTrigger.hpp:103-222; NO and LINEAR, float, the sparse stream) written
out in C++, g++ -O2, one core.  --quick [K]: the float, LINEAR, sparse row at 2^K (default 2^27) only, nothing written (for a rocprofv3 run); with --dense, the dense row; with --method M, method M."""
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
METHODS = ("NO_INTERPOLATION", "BASIC_LINEAR_INTERPOLATION", "LINEAR_INTERPOLATION")

CPU_LOOP = r"""
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>
int main() {
    const int n = 1 << 24;
    std::vector<float> x(n + 32, 0.f);
    for (int i = 0; i < n; ++i) x[i + 32] = 2.f * std::sin(6.2831853e-3f * i);
    const float upper = 1.f, lower = -1.f, offset = 0.f;
    for (int method = 0; method < 3; method += 2) {
        bool last = false; long acc = 0, edges = 0; double chk = 0;
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < n; ++i) {
            const float* h = &x[i + 32]; const float yc = h[0], yp = h[-1];
            if (method == 0) {
                if (!last && yc >= upper) { last = true; ++edges; } else if (last && yc <= lower) { last = false; ++edges; }
                continue;
            }
            const bool was = acc > 0;
            if (!was && !last && yp <= lower && yc > lower) acc = 1;
            if (!was && last && yp >= upper && yc < upper) acc = 1;
            if (was) ++acc;
            if (acc > 0) {
                if ((!last && yc >= upper) || (last && yc <= lower)) {
                    const long ns = std::min(std::max(acc, 2L), 32L); const float nv = (float)ns;
                    const float sumX2 = (nv * (nv - 1.f) * (2.f * nv - 1.f)) / 6.f, meanX = 0.5f * (nv - 1.f);
                    float sumY = 0.f, sumXY = 0.f;
                    for (long k = 0; k < ns; ++k) { const float xi = (float)((ns - 1) - k), yi = h[-k]; sumY += yi; sumXY += xi * yi; }
                    const float meanY = sumY / nv, slope = (sumXY - nv * meanX * meanY) / (sumX2 - nv * meanX * meanX), icpt = meanY - slope * meanX;
                    chk += (offset - icpt) / slope - (float)(ns - 1);
                    last = !last; acc = 0; ++edges;
                } else if ((!last && yc < lower) || (last && yc > upper)) acc = 0;
            }
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%d %.6e %ld %.3f\n", method, n / sec, edges, chk);
    }
}
"""


def cpu_rates():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "st.cpp"), os.path.join(d, "st")
        open(src, "w").write(CPU_LOOP)
        subprocess.check_call(["g++", "-O2", "-std=c++20", src, "-o", exe])
        return {int(line.split()[0]): float(line.split()[1]) for line in subprocess.check_output([exe], text=True).splitlines()}


def stream(n, dtype, dense):
    scale = 1000.0 if dtype == torch.int16 else 1.0
    if dense:
        x = torch.where(torch.arange(n, device="cuda") % 2 == 0, 2.0 * scale, -2.0 * scale)
    else:
        x = 2.0 * scale * torch.sin(torch.arange(n, device="cuda", dtype=torch.float64) * (2 * np.pi / 1000.0))
    return x.to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schmitt_trigger_rates.txt"))
    ap.add_argument("--quick", nargs="?", type=int, const=27, default=None, metavar="K")
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--method", choices=METHODS, default="LINEAR_INTERPOLATION")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.quick:
        rows = [(1 << a.quick, torch.float32, a.method, a.dense)]
    else:
        rows = [(n, dt, m, dense) for dt in (torch.float32, torch.int16) for n in (1 << 24, 1 << 27) for dense in (False, True) for m in METHODS]
    lines = [f"# SchmittTrigger rates, MI355X ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}), input and edge list resident in device memory (tools/schmitt_trigger_rates.py)",
             "# type | samples | stream | method | edges per call | Gsamples/s | ms per call | of 6.3 TB/s at 2 sizeof(T) B per sample (the input read twice)"]
    st = torch.cuda.current_stream().cuda_stream
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    for n, dt, m, dense in rows:
        x = stream(n, dt, dense)
        scale = 1000.0 if dt == torch.int16 else 1.0
        blk = G.SchmittTrigger(0.0, scale, m, dt)
        cap = n if dense else n // 100
        buf = torch.empty((cap, capi.SCHMITT_EDGE_BYTES // 4), dtype=torch.int32, device="cuda")

        def call():
            rc = capi.lib().gr4hip_schmitt_process(blk._h, x.data_ptr(), n, buf.data_ptr(), cap, cnt.data_ptr(), st)
            assert rc == 0, (rc, capi.lib().gr4hip_last_error().decode())
        sec = steady(call)
        edges = int(cnt.item())
        rate = n / sec
        name = "float" if dt == torch.float32 else "int16"
        lines.append(f"{name} | 2^{n.bit_length() - 1} | {'dense' if dense else 'sparse'} | {m} | {edges} | {rate / 1e9:.1f} | {sec * 1e3:.3f} | "
                     f"{rate * 2 * x.element_size() / ACHIEVABLE:.3f}")
        del x, buf, blk
        torch.cuda.empty_cache()
    if not a.quick:
        for method, r in sorted(cpu_rates().items()):
            lines.append(f"processOne in C++, float, sparse, one CPU core (g++ -O2) | 2^24 | sparse | {METHODS[method]} | - | {r / 1e9:.3f} | - | -")
    text = "\n".join(lines) + "\n"
    if not a.quick:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
