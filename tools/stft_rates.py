"""Overlapped FFT frame rates on one MI355X (gr4hip_stft_mag2 / gr4hip_stft_mag2_integrate; input and outputs resident in device memory; OVERLAPPED_FFT.md).

    python tools/stft_rates.py [--out profiles/stft_rates.txt] [--log2 26] [--rounds 3]

|X|^2 of 2^26 complex input samples per call, Hann window, at (N, S) in {(1024, 512), (1024, 256), (8192, 4096), (8192, 2048), (1024, 2048)}:
  (a) the means a caller has without the feature: the frames materialised in device memory (as_strided(...).contiguous(), what x.unfold(0, N, S).contiguous()
      does) followed by gr4hip_fft_mag2 on them;
  (b) the gather path (GR4HIP_STFT_GATHER): frame_gather into a bounded scratch, the FFT block's kernels behind it;
  (c) the native path: the hop front end in front of fft_fast_kernel's passes;
  (d) gr4hip_fft_mag2 on the same input at S = N on the block kernels (GR4HIP_FFT_NO_PIPELINE): with the shape's output-write bound, the ceiling.
Welch at A = 1024 frames per spectrum: gr4hip_stft_mag2_integrate against (c) followed by gr4hip_specint_process.
Rates are input samples per second and frames' values (k N) per second; the bound is (8 n_read + 4 k N) bytes at 6.3 TB/s, n_read the input
samples that lie in a frame.  Each figure is back-to-back calls at
settled clocks (tools/_timing.py); every configuration is measured `rounds` times, alternated round by round, and min / median / max are recorded.  Before
anything is timed the three forms' values are compared at the timed size."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402

SHAPES = [(1024, 512), (1024, 256), (8192, 4096), (8192, 2048), (1024, 2048)]
HBM = 6.3e12  # achievable bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_rates.txt"))
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--integrate", type=int, default=1024)
    ap.add_argument("--native-switch", type=int, default=2, help="value of GR4HIP_STFT_GATHER that forces the hop kernels")
    ap.add_argument("--seam-only", action="store_true", help="only the sweep over call sizes")
    a = ap.parse_args()
    n = 1 << a.log2
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn(n, 2, device="cuda", generator=g) * 0.70710678)
    nmax = max(((n - N) // S + 1) * N for N, S in SHAPES)
    out = torch.empty(nmax, dtype=torch.float32, device="cuda")

    def switched(name, fn):
        def run():
            G.capi.developer_switch(name, 1)
            try:
                return fn()
            finally:
                G.capi.developer_switch(name, 0)
        return run

    for N, S in ([] if a.seam_only else SHAPES):
        k = (n - N) // S + 1
        fft, st = G.FFT(N, "Hann"), G.STFT(N, S, "Hann")

        def materialised():
            return fft.mag2(x.as_strided((k, N), (S, 1)).contiguous(), out=out)

        def hop():
            st.reset()
            return st.mag2(x, out=out)

        cases = [("(a) materialised frames + FFT.mag2", materialised), ("(b) gather path", switched("GR4HIP_STFT_GATHER", hop)), ("(c) native path (hop front end)", hop)]
        # the values first: (b) and (c) bit for bit; (a) too where it runs the block kernels (at 8192 points and >= 256 frames it takes the frame pipeline: to rounding)
        ref = hop().clone().reshape(-1)
        same_b = bool(torch.equal(switched("GR4HIP_STFT_GATHER", hop)().reshape(-1), ref))
        ma = materialised().reshape(-1)[:k * N]
        same_a = bool(torch.equal(ma, ref))
        err_a = float(((ma - ref).abs().max() / ref.abs().max()).item())
        say(f"N {N:5d} S {S:5d} k {k:7d}: gather == native {same_b}; materialised == native {same_a} (max |diff| / max {err_a:.1e})")
        assert same_b
        del ref, ma
        sec = {name: [] for name, _ in cases}
        for _ in range(a.rounds):  # alternated: a drift of the machine reaches every configuration alike
            for name, fn in cases:
                sec[name].append(steady(fn))
        n_read = min(n, k * min(N, S))  # a skipping stride never reads the samples between two frames
        bound = (8 * n_read + 4 * k * N) / HBM
        base = statistics.median(sec[cases[0][0]])
        for name, _ in cases:
            s = sorted(sec[name])
            med = statistics.median(s)
            say(f"N {N:5d} S {S:5d} {name:<38} {n / s[-1] / 1e9:7.2f} / {n / med / 1e9:7.2f} / {n / s[0] / 1e9:7.2f} G input samples/s (min / median / max of {a.rounds})"
                f"   {k * N / med / 1e9:7.1f} G values/s   {base / med:5.2f} x (a)   {bound / med:5.3f} of the bound")
        say(f"N {N:5d} S {S:5d} bound: {8 * n_read + 4 * k * N} bytes at 6.3 TB/s = {bound * 1e3:.3f} ms = {n / bound / 1e9:.1f} G input samples/s")

        # Welch
        A = a.integrate
        if k >= 2 * A and S < N:
            si = G.SpectrumIntegrator(N, A)
            wout = torch.empty((k // A) * N, dtype=torch.float32, device="cuda")

            def fused():
                st.reset()
                si.reset()
                return st.power_integrated(x, si, out=wout)

            def two_calls():
                st.reset()
                si.reset()
                return si.process_bulk(st.mag2(x, out=out), out=wout)

            want = two_calls().clone()
            say(f"N {N:5d} S {S:5d} Welch A {A}: integrate == mag2 + specint {bool(torch.equal(fused(), want))}")
            wcases = [("Welch: (c) + SpectrumIntegrator.process_bulk", two_calls), ("Welch: STFT.power_integrated (pieces)", fused)]
            wsec = {name: [] for name, _ in wcases}
            for _ in range(a.rounds):
                for name, fn in wcases:
                    wsec[name].append(steady(fn))
            wbase = statistics.median(wsec[wcases[0][0]])
            for name, _ in wcases:
                s = sorted(wsec[name])
                med = statistics.median(s)
                say(f"N {N:5d} S {S:5d} {name:<46} {n / s[-1] / 1e9:7.2f} / {n / med / 1e9:7.2f} / {n / s[0] / 1e9:7.2f} G input samples/s   {wbase / med:5.2f} x the two calls")
            si.close()
        fft.close()
        st.close()

    # the seam: streams cut into calls of 2^14 .. 2^22 samples -- every call but the first begins with frames that start in the history.  The hop kernels forced
    # (GR4HIP_STFT_GATHER = 2: a staging launch and a second hop launch per call), the gather path forced (= 1: the history is one more source of the gather
    # kernel), and the default, which sends a call with a seam and few values to the gather path (stft.hip, stft_seam_gather_values)
    def switched_to(value, fn):
        def run():
            G.capi.developer_switch("GR4HIP_STFT_GATHER", value)
            try:
                return fn()
            finally:
                G.capi.developer_switch("GR4HIP_STFT_GATHER", 0)
        return run

    for N, S in ((256, 64), (1024, 512), (2048, 1024), (4096, 2048), (8192, 4096)):
        st = G.STFT(N, S, "Hann")
        for lg in (14, 16, 18, 20, 22):
            call = 1 << lg
            total = min(n, max(1 << 22, call * 8))

            def stream():
                st.reset()
                for p in range(0, total, call):
                    st.mag2(x[p:p + call], out=out)

            scases = [("hop kernels, staging span", switched_to(a.native_switch, stream)), ("gather path", switched_to(1, stream)), ("default", stream)]
            ssec = {name: [] for name, _ in scases}
            for _ in range(a.rounds):
                for name, fn in scases:
                    ssec[name].append(steady(fn))
            for name, _ in scases:
                s = sorted(ssec[name])
                med = statistics.median(s)
                say(f"N {N:5d} S {S:5d} 2^{lg}-sample calls, {name:<26} {total / s[-1] / 1e9:7.2f} / {total / med / 1e9:7.2f} / {total / s[0] / 1e9:7.2f} G input samples/s   {med / (total // call) * 1e6:7.1f} us per call")
        st.close()

    # (d) the FFT block at S = N on the block kernels: what a hop costs nothing over
    for N in ([] if a.seam_only else sorted({N for N, _ in SHAPES})):
        fft = G.FFT(N, "Hann")
        s = sorted(steady(switched("GR4HIP_FFT_NO_PIPELINE", lambda: fft.mag2(x, out=out))) for _ in range(a.rounds))
        med = statistics.median(s)
        say(f"N {N:5d} S = N (d) FFT.mag2, block kernels            {n / s[-1] / 1e9:7.2f} / {n / med / 1e9:7.2f} / {n / s[0] / 1e9:7.2f} G input samples/s = G values/s"
            f"   {12 * n / HBM / med:5.3f} of its bound (12 bytes per sample)")
        fft.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/stft_rates.py on %s (%s): 2^%d complex samples per call, Hann, |X|^2, back-to-back calls at settled clocks, configurations alternated round by round\n"
                 % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, a.log2))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
