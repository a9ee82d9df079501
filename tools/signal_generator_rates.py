"""SignalGenerator output rates on one MI355X (gr4hip_siggen_process; the output resident in device memory) and the single-core rate of the host mirror's
per-sample loop (gr::basic::SignalGenerator<T>::generateSample, gr4/blocks.hpp).

    python tools/signal_generator_rates.py [--out profiles/signal_generator_rates.txt] [--quick TYPE [--dtype D] [--log2 K]]

Rows: float, double, complex<float> and int16, every signal type, at 2^24 and 2^27 samples per call.  The yardstick of a row is the handle's own Const type at the
same sample type and size: pure stores with the same launch shape, so `of Const` is what the arithmetic, the jump-ahead and the extra launches cost.  Each rate is
back-to-back calls at settled clocks (tools/_timing.py); the stream simply continues from call to call.  The CPU rows, the figure before this block existed on the
device, time the host mirror's loop (g++ -O2, one core, 2^22 samples).  --quick TYPE: one row, nothing written (for a rocprofv3 run)."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402
from gnuradio4_amd import capi  # noqa: E402

DTYPES = {"float": torch.float32, "double": torch.float64, "complex<float>": torch.complex64, "int16": torch.int16}
CPU_TYPES = {"float": "float", "double": "double", "complex<float>": "std::complex<float>", "int16": "std::int16_t"}

CPU_LOOP = r"""
#include <chrono>
#include <cstdio>
#include <gr4/blocks.hpp>
template <typename T>
void run(const char* name) {
    const char* types[] = {"Const", "Sin", "Cos", "Square", "Saw", "Triangle", "FastSin", "FastCos", "UniformNoise", "TriangularNoise", "GaussianNoise"};
    const std::size_t n = std::size_t(1) << 22;
    std::vector<T> out(n);
    for (const char* t : types) {
        gr::basic::SignalGenerator<T> g;
        g.applySettings({{"signal_type", std::string(t)}, {"frequency", 37.5}, {"sample_rate", 1000.0}, {"phase", 0.3}, {"amplitude", 1.5}, {"offset", 0.25}, {"seed", std::int64_t(12345)}});
        const auto t0 = std::chrono::steady_clock::now();
        for (std::size_t i = 0; i < n; ++i) out[i] = g.generateSample();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%s|%s|%.6e|%g\n", name, t, double(n) / sec, double(std::abs(out[n / 2])));
    }
}
int main() {
    run<float>("float"); run<double>("double"); run<std::complex<float>>("complex<float>"); run<std::int16_t>("int16");
}
"""


def cpu_rates():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sg.cpp"), os.path.join(d, "sg")
        open(src, "w").write(CPU_LOOP)
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-I" + os.path.join(ROOT, "gnuradio4_amd", "host", "include"), src, "-o", exe,
                               "-L" + os.path.join(ROOT, "gnuradio4_amd"), "-lgr4hip", "-Wl,-rpath," + os.path.join(ROOT, "gnuradio4_amd"), "-Wl,-rpath,/opt/rocm/lib"])
        out = {}
        for line in subprocess.check_output([exe], text=True).splitlines():
            name, t, rate, _ = line.split("|")
            out[(name, t)] = float(rate)
        return out


def rate(name, t, n):
    gen = G.SignalGenerator(t, DTYPES[name], sample_rate=1000.0, frequency=37.5, amplitude=1.5, offset=0.25, phase=0.3, seed=12345)
    out = torch.empty(n, dtype=DTYPES[name], device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        rc = capi.lib().gr4hip_siggen_process(gen._h, out.data_ptr(), n, st)
        assert rc == 0, (rc, capi.lib().gr4hip_last_error().decode())
    sec = steady(call)
    del out, gen
    torch.cuda.empty_cache()
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signal_generator_rates.txt"))
    ap.add_argument("--quick", default=None, metavar="TYPE")
    ap.add_argument("--dtype", default="float", choices=list(DTYPES))
    ap.add_argument("--log2", type=int, default=27)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.quick:
        sec = rate(a.dtype, a.quick, 1 << a.log2)
        print(f"{a.dtype} | 2^{a.log2} | {a.quick} | {(1 << a.log2) / sec / 1e9:.1f} Gsamples/s | {sec * 1e3:.3f} ms per call")
        return
    lines = [f"# SignalGenerator rates, MI355X ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}), output resident in device memory (tools/signal_generator_rates.py)",
             "# type | samples | signal | Gsamples/s | ms per call | of Const (same type and size) | output GB/s"]
    for name in DTYPES:
        for k in (24, 27):
            n = 1 << k
            const = rate(name, "Const", n)
            for t in capi.SIGGEN_TYPES:
                sec = const if t == "Const" else rate(name, t, n)
                lines.append(f"{name} | 2^{k} | {t} | {n / sec / 1e9:.1f} | {sec * 1e3:.3f} | {const / sec:.3f} | {n * torch.empty(0, dtype=DTYPES[name]).element_size() / sec / 1e9:.0f}")
    for (name, t), r in cpu_rates().items():
        lines.append(f"host mirror generateSample(), one CPU core (g++ -O2), {name} | 2^22 | {t} | {r / 1e9:.4f} | - | - | -")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
