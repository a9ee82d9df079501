"""PowerFactor / SystemUnbalance rates on one MI355X (gr4hip_powerfactor_process / gr4hip_unbalance_process; rows resident in device memory).

    python tools/power_quality_rates.py [--out profiles/power_quality_rates.txt] [--log2 27] [--chain-log2 24]

Rows at 2^27 items per row, float, three phases: Gsamples/s (samples per row) and TB/s moved (bytes read + bytes written) for both kernels with every output and with
single outputs, the same with rows n + 1 apart (rows then disagree in alignment: the ones off the common 16-byte grid move element by element), the run-time
phase count (five phases), and PowerMetrics(decimate 1) followed by the power factor on its resident output rows against PowerMetrics alone.  The yardstick, measured
in the same run, is a one-op gr4hip_ewise_process float program: the library's existing streaming kernel.  Each rate is back-to-back calls at settled clocks
(tools/_timing.py).  FIRST MEASUREMENTS: no threshold decides anything."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gnuradio4_amd as G  # noqa: E402
from _timing import steady  # noqa: E402
from gnuradio4_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_quality_rates.txt"))
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--chain-log2", type=int, default=24)
    a = ap.parse_args()
    n = 1 << a.log2
    L = capi.lib()
    rows = []

    def row(name, fn, items, nbytes):
        sec = steady(fn)
        rows.append((name, items / sec / 1e9, nbytes / sec / 1e12))
        print(f"{name:<78} {rows[-1][1]:9.2f} Gsamples/s {rows[-1][2]:7.3f} TB/s", flush=True)

    def call(rc):
        assert rc == capi.OK, L.gr4hip_last_error()

    xf = torch.randn(n, device="cuda")
    yf = torch.empty_like(xf)
    ew = G.Merged(torch.float32, [("Multiply", 1.0001)])
    row("yardstick: one-op ewise program, float", lambda: ew.process_bulk(xf, out=yf), n, 8 * n)
    del xf, yf

    def rows_of(count, stride, scale=1.0, offset=0.0):
        return (torch.rand(count * stride + 8, device="cuda") * scale + offset)

    st = 0  # the default stream: the one torch's events are recorded on
    for stride, what in ((n, ""), (n + 1, ", rows n + 1 apart")):
        S = rows_of(3, stride, 100.0, 1.0)
        P = S * (torch.rand_like(S) * 2.2 - 1.1)  # |P| > S on a tenth of the samples: the clamp
        f, ph = torch.empty(3 * stride + 8, device="cuda"), torch.empty(3 * stride + 8, device="cuda")
        pp, sp, fp, hp = (t.data_ptr() for t in (P, S, f, ph))
        row("PowerFactor<float, 3>" + what, lambda: call(L.gr4hip_powerfactor_process(capi.F32, 3, pp, sp, stride, fp, hp, stride, n, st)), n, 48 * n)
        row("PowerFactor<float, 3>, power_factor only (no acos)" + what, lambda: call(L.gr4hip_powerfactor_process(capi.F32, 3, pp, sp, stride, fp, None, stride, n, st)), n, 36 * n)
        del f, ph
        U, I = rows_of(3, stride, 23.0, 218.5), rows_of(3, stride, 2.0, 9.0)
        o = [torch.empty(n + 8, device="cuda") for _ in range(3)]
        up, ip, op = U.data_ptr(), I.data_ptr(), [t.data_ptr() for t in o]
        row("SystemUnbalance<float, 3>" + what, lambda: call(L.gr4hip_unbalance_process(capi.F32, 3, up, ip, pp, stride, op[0], op[1], op[2], n, st)), n, 48 * n)
        row("SystemUnbalance<float, 3>, voltage unbalance only" + what, lambda: call(L.gr4hip_unbalance_process(capi.F32, 3, up, ip, pp, stride, None, op[1], None, n, st)), n, 16 * n)
        del P, S, U, I, o
    m = n // 2  # five phases: the run-time loop reads U and I twice (the second pass from the cache where it fits)
    U, I, P = rows_of(5, m, 23.0, 218.5), rows_of(5, m, 2.0, 9.0), rows_of(5, m, 2000.0, 0.0)
    o = [torch.empty(m, device="cuda") for _ in range(3)]
    up, ip, pp, op = U.data_ptr(), I.data_ptr(), P.data_ptr(), [t.data_ptr() for t in o]
    row("SystemUnbalance<float, 5> (run-time phase count), 2^%d items" % (a.log2 - 1), lambda: call(L.gr4hip_unbalance_process(capi.F32, 5, up, ip, pp, m, op[0], op[1], op[2], m, st)), m,
        (15 + 3) * 4 * m)
    del U, I, P, o

    nc = 1 << min(a.chain_log2, a.log2)  # PowerMetrics is a five-launch float64 scan: the chain row is about what the power factor adds behind it
    u, i = torch.randn(3, nc, device="cuda") * 325.0, torch.randn(3, nc, device="cuda") * 14.0
    pm, pf = G.PowerMetrics(n_phases=3, decimate=1), G.PowerFactor(3)
    row("PowerMetrics<float, 3>(decimate 1) alone, 2^%d items" % (nc.bit_length() - 1), lambda: pm.process_bulk(u, i), nc, 3 * 7 * 4 * nc)

    def chain():
        Pm, _, Sm, _, _ = pm.process_bulk(u, i)
        pf.process(Pm, Sm)
    row("PowerMetrics<float, 3>(decimate 1) -> PowerFactor on the resident rows, 2^%d items" % (nc.bit_length() - 1), chain, nc, 3 * 11 * 4 * nc)

    with open(a.out, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}; 2^{a.log2} items per row and call unless the row says otherwise; FIRST MEASUREMENTS, no threshold decides anything\n")
        fh.write(f"# yardstick bytes/s: {rows[0][2]:.3f} TB/s (one-op gr4hip_ewise_process float program, same run); PowerMetrics rows count its inputs and outputs only\n")
        for name, gs, tb in rows:
            fh.write(f"{name:<78} {gs:9.2f} Gsamples/s {tb:7.3f} TB/s  ({100 * tb / rows[0][2]:5.1f} % of the yardstick's bytes/s)\n")


if __name__ == "__main__":
    main()
