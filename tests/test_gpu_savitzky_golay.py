"""The Savitzky-Golay blocks on the device against the numpy oracle (tests/savitzky_golay_oracle.py).

Zero-phase kernel (csrc/savitzky_golay.hip), per output, with S = sum |c| and M = max |x| of the row:
  float32   |out - oracle| <= 2^-22 S^2 M: an intermediate t may round to the neighbouring float (one ulp <= 2^-23 S M, carried through the second pass: x S), and
            the output is rounded once more (another 2^-23 S^2 M at most)
  float64   2 (W + 1) 2^-53 S^2 M: two float64 sums of W products each, in a different order from the oracle's
Rows sit row_stride = N + 5 apart and start off the 16-byte alignment; every element of the output buffer outside the rows must keep its value.
Streaming block (the design on the FIR handles), per output: (W + 1) eps_T sum_k |c_k x_k|.  Chunked runs are held to the same bar, not to bit equality: the FIR
dispatcher may take another kernel for another span.  The largest errors are printed (pytest -s) and quoted in SAVITZKY_GOLAY.md."""
import os
import subprocess

import numpy as np
import pytest
import torch

import savitzky_golay_oracle as SG

pytestmark = pytest.mark.gpu

TORCH = {np.float32: torch.float32, np.float64: torch.float64}
ZP_SETTINGS = [(1, 0, 0), (2, 1, 0), (4, 2, 1), (5, 2, 0), (11, 4, 0), (11, 4, 2), (64, 3, 1), (255, 4, 0)]
SENTINEL = 12345.0


def _tile():
    import gnuradio4_amd as G
    return G.SavitzkyGolayDataSetFilter.tile()


def _rows(dtype, N, seed):
    """three rows of seeded Gaussian noise on a ramp (a boundary error moves the ends by O(ramp))"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((3, N)) + np.linspace(-2.0, 5.0, N)[None, :] * np.array([[1.0], [-0.5], [3.0]])).astype(dtype)


def _strided(dtype, rows, offset):
    """a device buffer full of SENTINEL with the rows at `offset` elements, N + 5 apart; returns (buffer, the [batch, N] view)"""
    batch, N = rows.shape
    stride = N + 5
    buf = torch.full((offset + batch * stride + 8,), SENTINEL, dtype=TORCH[dtype], device="cuda")
    view = buf[offset:offset + (batch - 1) * stride + N].as_strided((batch, N), (stride, 1))
    view.copy_(torch.from_numpy(rows).cuda())
    return buf, view


@pytest.mark.parametrize("policy", ["Reflect", "Replicate"])
@pytest.mark.parametrize("W,p,d", ZP_SETTINGS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_phase_against_the_oracle(dtype, W, p, d, policy):
    import gnuradio4_amd as G
    TILE = _tile()
    blk = G.SavitzkyGolayDataSetFilter(TORCH[dtype], W, p, d, policy)
    c, info = blk.coefficients()
    cw, oi = SG.design(dtype, W, p, d)
    assert info.rank == oi["rank"] and np.max(np.abs(c.astype(np.float64) - cw.astype(np.float64))) <= 1e-9 * np.max(np.abs(cw))
    S = float(np.abs(c.astype(np.float64)).sum())
    worst = 0.0
    for N in sorted({1, 2, W - 1, W, W + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17} - {0}):
        rows = _rows(dtype, N, 1000 * W + N)
        want = np.stack([SG.zero_phase(c, r, policy)[0] for r in rows]).astype(np.float64)  # the oracle once per row, shared by both batch sizes
        M = np.max(np.abs(rows.astype(np.float64)), axis=1, keepdims=True)
        bar = (2.0 ** -22 if dtype == np.float32 else 2 * (W + 1) * 2.0 ** -53) * S * S * M
        for batch, off_in, off_out in ((1, 1, 3), (3, 3, 1)):
            _, x = _strided(dtype, rows[:batch], off_in)
            ybuf, y = _strided(dtype, np.zeros_like(rows[:batch]), off_out)
            got = blk.process(x, out=y)
            assert got.data_ptr() == y.data_ptr()
            err = np.abs(got.cpu().numpy().astype(np.float64) - want[:batch])
            worst = max(worst, float(np.max(err / bar[:batch])))
            assert np.all(err <= bar[:batch]), (N, batch, float(np.max(err / bar[:batch])))
            outside = torch.ones_like(ybuf, dtype=torch.bool)
            for r in range(batch):
                outside[off_out + r * (N + 5):off_out + r * (N + 5) + N] = False
            assert bool(torch.all(ybuf[outside] == SENTINEL)), (N, batch)  # beyond N in each row, between the rows, in front of the first
    print(f"{np.dtype(dtype).name} W {W} p {p} d {d} {policy}: largest error {worst:.3g} of the bar")
    if W > 1:  # n == 0: a no-op
        e = torch.zeros(0, dtype=TORCH[dtype], device="cuda")
        assert blk.process(e).numel() == 0


def test_zero_phase_set_params_contiguous_rows_and_refusals():
    import gnuradio4_amd as G
    TILE = _tile()
    blk = G.SavitzkyGolayDataSetFilter(torch.float32, 5, 2, 0, "Reflect")
    rows = _rows(np.float32, TILE + 300, 7)
    x = torch.from_numpy(rows).cuda()
    for settings in (dict(window_size=31, poly_order=6), dict(deriv_order=1, boundary_policy="Replicate"), dict(window_size=4, poly_order=9, deriv_order=9)):
        blk.set_params(**settings)
        c, _ = blk.coefficients()
        cw, _ = SG.design(np.float32, blk.window_size, blk.poly_order, blk.deriv_order)
        assert np.max(np.abs(c - cw)) <= np.spacing(np.max(np.abs(cw)))
        S = float(np.abs(c.astype(np.float64)).sum())
        got = blk.process(x).cpu().numpy().astype(np.float64)  # a contiguous [3, N] tensor: row_stride == N
        for r in range(3):
            want, _ = SG.zero_phase(c, rows[r], blk.boundary_policy)
            assert np.max(np.abs(got[r] - want.astype(np.float64))) <= 2.0 ** -22 * S * S * float(np.max(np.abs(rows[r])))
        one = blk.process(x[1])  # a 1-D tensor is one row
        assert np.array_equal(one.cpu().numpy().astype(np.float64), got[1])
    with pytest.raises(G.capi.Gr4HipError, match="overlap"):
        blk.process(x, out=x)
    with pytest.raises(G.capi.Gr4HipError):
        blk.process(x.double())


@pytest.mark.parametrize("alignment", ["Centred", "Causal"])
@pytest.mark.parametrize("W", [1, 5, 11, 32, 33, 128])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_streaming_against_the_oracle(dtype, W, alignment):
    import gnuradio4_amd as G
    n = 5000
    rng = np.random.default_rng(W)
    x = (rng.standard_normal(n) + 0.5 * np.sin(np.arange(n) * 0.01)).astype(dtype)
    xd = torch.from_numpy(x).cuda()
    eps = float(np.finfo(dtype).eps)
    worst = 0.0
    blk = G.SavitzkyGolayFilter(TORCH[dtype], 9, 2, 0, 1.0, "Centred")
    for d, rate in ((0, 1.0), (1, 1.0), (0, 1000.0), (1, 1000.0)):
        delta = float(dtype(1) / dtype(np.float32(rate)))
        cw, oi = SG.design(dtype, W, min(4, W - 1), d, delta, alignment)
        # a set_params issued mid-stream clears the history: a FIR handle whose history was kept would carry the samples before it into the first W - 1 outputs
        blk.process_bulk(xd[:777] * 100)
        blk.set_params(window_size=W, poly_order=4, deriv_order=d, sample_rate=rate, alignment=alignment)
        assert np.max(np.abs(blk.coeffs.astype(np.float64) - cw.astype(np.float64))) <= (np.spacing(np.max(np.abs(cw))) if dtype == np.float32 else 1e-9 * np.max(np.abs(cw)))
        assert blk.info.rank == oi["rank"]
        # the filter is evaluated with the block's own coefficients (held to the oracle's design just above): at p = W - 1 the design is an interpolation, its
        # off-centre coefficients are rounding noise of 1e-17, and the per-output bar below is about the sums, not about which noise the design left there
        want, mag = SG.streaming(blk.coeffs, x)
        bar = (W + 1) * eps * mag + 1e-300

        def check(got, what):
            nonlocal worst
            err = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64))
            worst = max(worst, float(np.max(err / bar)))
            assert np.all(err <= bar), (d, rate, what, float(np.max(err / bar)))

        check(blk.process_bulk(xd), "after set_params")
        blk.reset()
        check(blk.process_bulk(xd), "after reset")
        fresh = G.SavitzkyGolayFilter(TORCH[dtype], W, 4, d, rate, alignment)
        check(fresh.process_bulk(xd), "fresh")
        fresh.close()
        out = torch.empty_like(xd)
        for chunk in sorted({1, 7, W - 1, W, 1000} - {0}):
            blk.process_bulk(xd[:13] * 100)
            blk.reset()
            for a in range(0, n, chunk):
                blk.process_bulk(xd[a:a + chunk], out=out[a:a + chunk])
            check(out, f"chunks of {chunk}")
    blk.close()
    print(f"{np.dtype(dtype).name} W {W} {alignment}: largest streaming error {worst:.3g} of the bar")


def test_graphs_on_the_device(tmp_path):
    """source -> SavitzkyGolayFilter (gpu:hip:0, through hip::plan) -> sink and FFT -> SavitzkyGolayDataSetFilter (gpu:hip:0) -> sink as a fresh child process, against
    the oracle and against the CPU bodies of the same blocks in the same graphs"""
    import test_savitzky_golay_host as H
    subprocess.check_call(["bash", os.path.join(H.ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    x = H._stream()
    x.tofile(tmp_path / "x.f32")
    x.astype(np.float64).tofile(tmp_path / "x.f64")
    out = {}
    for domain, tag in (("gpu:hip:0", "device"), ("host", "host")):
        r = subprocess.run([H.BIN, H.PLUGIN, domain, str(tmp_path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"all checks passed (compute_domain {domain})" in r.stdout
        if tag == "device":
            assert "stream_f32: 5000 samples, 1 planned runs" in r.stdout and "stream_f64: 5000 samples, 1 planned runs" in r.stdout
        out[tag] = H.check_graph_outputs(tmp_path, tag)  # each against the oracle, under the T-precision bars
    for name in out["host"]:  # and against each other: both are within the bar of the oracle, so within twice the bar of each other; here a plain scale check
        a, b = out["device"][name].astype(np.float64), out["host"][name].astype(np.float64)
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-3 * max(np.max(np.abs(b)), 1e-30), name
