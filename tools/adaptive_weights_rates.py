"""Adaptive-weights rates on one MI355X (gr4hip_mvdr_process; matrices, steering vectors and outputs resident in device memory).

    python tools/adaptive_weights_rates.py [--out profiles/adaptive_weights_rates.txt] [--rounds 5]

(matrix, bin) pairs solved per second at N = 1024 for (S, B) = (2, 1), (4, 4), (8, 4), (16, 16), (32, 32), with enough matrices per call to fill the chip many
times over (2^17 bins per call up to S = 8, 2^15 above: a CU holds 32 bins at S <= 8 and 8 at S = 32).  Per shape, measured in the same run and alternated
round by round:
  (d) gr4hip_mvdr_process with the power output;
  (t) what a user could do before, on the device: the packed triangles completed to Hermitian complex128 matrices, the loading added, torch.linalg.solve, the
      normalisation and the rounding to complex64 [Q, B, S, N] -- completion included.
Each figure is back-to-back calls at settled clocks (tools/_timing.py); every configuration is measured `rounds` times, min / median / max are recorded.  The
float64 flop count of one (matrix, bin) is that of the definition: a complex multiply-subtract is 8 flop, sum_j j (S - j) of them in the factorisation and
B S (S - 1) in the two solves, plus one flop per division, square root and |y|^2 term; the rate is set against the 78.6 TFLOP/s FP64 vector peak of the part."""
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

FP64_PEAK = 78.6e12


def flops(S, B):
    msub = sum(j * (S - j) for j in range(S)) + B * S * (S - 1)
    other = S + S * (S - 1) + B * (4 * S + 4 * S + 2 * S + 1)  # sqrt, the column's divisions; per beam: the solves' divisions, |y|^2, u / d, 1 / d
    return 8 * msub + other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_weights_rates.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", type=str, default="2x1,4x4,8x4,16x16,32x32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the rates are measured on the GPU or not at all"
    N, loading = 1024, 1e-3
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    g = torch.Generator(device="cuda").manual_seed(1)
    for S, B in shapes:
        Q = (1 << 17 if S <= 8 else 1 << 15) // N
        P, frames = S * (S + 1) // 2, 2 * S
        # Q well-conditioned matrices: the correlator's own output for 2 S frames of unit noise per matrix
        x = torch.view_as_complex(torch.randn(S, Q * frames, N, 2, device="cuda", generator=g) * 0.70710678)
        vis = G.CrossSpectrum(S, N, frames, mean=True).process_bulk(x)
        del x
        steer = torch.polar(torch.ones(B, S, N, device="cuda"), 6.2831853 * torch.rand(B, S, N, device="cuda", generator=g))
        blk = G.AdaptiveWeights(S, B, N, loading)
        blk.set_steering(steer)
        w = torch.empty(Q * B * S * N, dtype=torch.complex64, device="cuda")
        ii, jj = torch.tril_indices(S, S, device="cuda")
        a128 = steer.to(torch.complex128).permute(2, 1, 0).contiguous()  # [N, S, B]

        def device():
            blk.process_bulk(vis, out=w, power=True)

        def today():
            low = torch.zeros(Q, N, S, S, dtype=torch.complex128, device="cuda")
            low[:, :, ii, jj] = vis.permute(0, 2, 1).to(torch.complex128)
            R = low + torch.tril(low, -1).mH
            lam = loading * torch.diagonal(R, dim1=-2, dim2=-1).real.sum(-1) / S
            R = R + lam[..., None, None] * torch.eye(S, dtype=torch.complex128, device="cuda")
            u = torch.linalg.solve(R, a128[None].expand(Q, N, S, B))
            d = (a128.conj()[None] * u).sum(-2, keepdim=True).real
            return (u / d).conj().permute(0, 3, 2, 1).to(torch.complex64).contiguous(), (1.0 / d).to(torch.float32)

        Wt, _ = today()
        device()
        torch.cuda.synchronize()
        worst = float((Wt - w.view(Q, B, S, N)).abs().max())
        failed = blk.stats()[1]
        del Wt
        cases = [("(d) gr4hip_mvdr_process", device, dict()), ("(t) torch.linalg.solve", today, dict(warm_s=0.02, time_s=0.05, min_reps=2))]
        sec = {name: [] for name, _, _ in cases}
        for _ in range(a.rounds):  # alternated: a drift of the machine reaches every configuration alike
            for name, fn, kw in cases:
                sec[name].append(steady(fn, **kw))
        rate = {name: sorted(Q * N / s / 1e6 for s in v) for name, v in sec.items()}
        fl = flops(S, B)
        for name, _, _ in cases:
            r = rate[name]
            med = statistics.median(r)
            tail = ""
            if name.startswith("(d)"):
                t = statistics.median(rate["(t) torch.linalg.solve"])
                tail = f"   {med * 1e6 * fl / 1e12:6.3f} TFLOP/s = {med * 1e6 * fl / FP64_PEAK:6.4f} of the FP64 vector peak ({fl} flop per bin)   {med / t:6.1f} x torch   max |W - torch| {worst:.2e}, {failed} bins failed"
            say(f"S {S:2d} B {B:2d} Q {Q:3d} {name:<26} {r[0]:9.3f} / {med:9.3f} / {r[-1]:9.3f} M bins/s (min / median / max of {a.rounds}){tail}")
        blk.close()
        del vis, w, steer, a128

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("# tools/adaptive_weights_rates.py on %s: (matrix, bin) pairs per second, N = %d, loading %g, back-to-back calls at settled clocks, configurations alternated round by round\n"
                 % (torch.cuda.get_device_name(0), N, loading))
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
