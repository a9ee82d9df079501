"""SvdDenoiser on the device (csrc/svd_denoiser.hip) against the numpy oracle in tests/svd_denoiser_oracle.py, on the oracle's SETTLED windows.

Bars, per output, relative to the peak |x| of the output's window:
  float32 / complex64:    1e-5, the project's float32 parity bar (the float64 internals leave it about two orders of margin: one float32 rounding is 6e-8);
  float64 / complex128:   1e-10 = eps64 * W * sweeps / relative gap ~ 2e-16 * 64 * 10 / 1e-3, the gap being what the settled rule's condition (b) guarantees.
A window is settled when the reference's rank rule is not on one of its knife edges (svd_denoiser_oracle.settled); tests/test_svd_denoiser_oracle.py asserts that
at most 5 % of the windows of every case used here are not.  Every case includes the stream's start (zero pre-fill, rank-deficient windows).

Chunking, reset and concurrency are compared bit for bit: every window is computed by the same instructions on the same values whatever the call boundaries."""
import numpy as np
import pytest
import torch

import svd_denoiser_oracle as SV

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f64": torch.float64, "c32": torch.complex64, "c64": torch.complex128}
BAR = {"f32": 1e-5, "c32": 1e-5, "f64": 1e-10, "c64": 1e-10}


def _blk(dtype, **settings):
    import gnuradio4_amd as G
    return G.SvdDenoiser(TORCH[dtype], **settings)


def _run(blk, x, cuts=(), empty=False):
    """x through the device block, cut into calls at `cuts` (with an empty call between the calls if `empty`)"""
    xd = torch.from_numpy(np.array(x)).cuda()
    marks = [0, *cuts, len(x)]
    parts = []
    for a, b in zip(marks[:-1], marks[1:]):
        parts.append(blk.process_bulk(xd[a:b]))
        if empty:
            assert blk.process_bulk(xd[:0]).numel() == 0
    return torch.cat(parts).cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize % 8 else np.uint64)


def _errors(got, r):
    """per output, relative to the peak of its window (an all-zero window: the absolute value)"""
    peak = r.peak()
    with np.errstate(all="ignore"):
        return np.abs(got.astype(np.complex128) - r.y.astype(np.complex128)) / np.where(peak > 0, peak, 1.0)


@pytest.mark.parametrize("name,dtype", [(n, d) for n, c in SV.CASES.items() for d in c[2]])
def test_parity_on_settled_windows(name, dtype):
    x, r = SV.case(name, dtype)
    blk = _blk(dtype, **SV.CASES[name][3])
    got = _run(blk, x)
    m = r.mask()
    assert m.mean() >= 0.95
    err = _errors(got, r)
    windows, bad = blk.stats()
    print(f"{name} {dtype}: max error on settled windows {err[m].max():.3g} (bar {BAR[dtype]:g}), on all {np.nanmax(err):.3g}; {windows} windows, "
          f"{r.unsettled()} unsettled, {blk.sweeps() / windows:.2f} sweeps per window")
    assert windows == len(r.windows) and bad == 0
    assert np.all(np.isfinite(got))
    assert err[m].max() <= BAR[dtype], (name, dtype, float(err[m].max()), int(np.argmax(np.where(m, err, 0))))


def _cuts(n, hop, seed):
    rng = np.random.default_rng(seed)
    yield [1]
    if hop > 2:
        yield [hop - 1]
    yield [hop]
    yield [hop + 1]
    for step in (7, 13, 101):
        yield list(range(step, n, step))
    for _ in range(2):
        yield sorted(set(int(c) for c in rng.integers(1, n, size=9)))


@pytest.mark.parametrize("name,dtype", [("A", "f32"), ("C", "f32"), ("C", "f64"), ("H", "f32"), ("D", "c32")])
def test_chunking_changes_no_bit(name, dtype):
    x, r = SV.case(name, dtype)
    x = x[:500]
    settings = SV.CASES[name][3]
    whole = _run(_blk(dtype, **settings), x)
    for k, cuts in enumerate(_cuts(len(x), r.geom["hop"], 5)):
        got = _run(_blk(dtype, **settings), x, cuts, empty=k % 2 == 0)
        assert np.array_equal(_bits(got), _bits(whole)), (cuts, np.flatnonzero(_bits(got) != _bits(whole))[:5])


def test_reset_returns_to_the_zero_prefill():
    x, r = SV.case("A", "f32")
    settings = SV.CASES["A"][3]
    blk = _blk("f32", **settings)
    first = _run(blk, x[:300])
    _run(blk, x[300:437])  # leaves the handle in the middle of a hop
    blk.reset()
    again = _run(blk, x[:300])
    assert np.array_equal(_bits(first), _bits(again))


def test_set_params_resets_and_follows_the_new_geometry():
    x, r = SV.case("C", "f32")
    blk = _blk("f32", **SV.CASES["A"][3])
    _run(blk, SV.case("A", "f32")[0][:211])
    blk.set_params(max_rank=SV.SIZE_MAX, energy_fraction=1.0, **SV.CASES["C"][3])  # W 64 -> 32, L 32 -> 8, hop 16 -> 3
    got = _run(blk, x, cuts=[100])
    fresh = _run(_blk("f32", **SV.CASES["C"][3]), x)
    assert np.array_equal(_bits(got), _bits(fresh))
    m = r.mask()
    assert _errors(got, r)[m].max() <= BAR["f32"]
    with pytest.raises(Exception):
        blk.set_params(hop_fraction=1.5)  # a rejected update leaves the handle's settings as they were
    blk.reset()
    assert np.array_equal(_bits(_run(blk, x[:50])), _bits(fresh[:50]))


def test_group_edges():
    import gnuradio4_amd as G
    g = G.SvdDenoiser.windows_per_group()
    assert g >= 1
    x, r = SV.case("A", "f32")
    hop = r.geom["hop"]
    m = r.mask()
    for nw in sorted({1, g - 1, g, g + 1}):
        n = (nw - 1) * hop + 1 if nw else 0  # the shortest stream with nw windows
        blk = _blk("f32", **SV.CASES["A"][3])
        got = _run(blk, x[:n])
        assert got.shape == (n,) and blk.stats() == (nw, 0)
        if n:
            err = np.abs(got.astype(np.float64) - r.y[:n]) / np.maximum(r.peak()[:n], 1e-300)
            assert err[m[:n]].max(initial=0.0) <= BAR["f32"]


@pytest.mark.parametrize("dtype", ["f32", "f64", "c32", "c64"])
def test_all_zero_input_gives_zeros(dtype):
    blk = _blk(dtype)
    got = _run(blk, np.zeros(200, dtype=SV.NUMPY_OF[dtype]))
    assert not np.any(got) and not np.any(np.isnan(got))
    assert blk.stats() == (13, 0)


def test_constant_input_stays_finite_and_near_its_value():
    for dtype in ("f32", "f64"):
        blk = _blk(dtype)
        got = _run(blk, np.full(400, 5.0, dtype=SV.NUMPY_OF[dtype]))
        assert np.all(np.isfinite(got)) and blk.stats()[1] == 0
        assert np.max(np.abs(got[64:] - 5.0)) <= 0.1


@pytest.mark.parametrize("dtype,value", [("f32", np.nan), ("f64", np.inf), ("c32", complex(0.0, np.nan))])
def test_one_bad_sample_poisons_exactly_the_hops_whose_window_holds_it(dtype, value):
    name = "D" if dtype[0] == "c" else "A"
    settings = SV.CASES[name][3]
    x = np.array(SV.case_input(name, 700)).astype(SV.NUMPY_OF[dtype])
    x[301] = value
    r = SV.run(x, dtype, **settings)
    want_nan = np.isnan(r.y)
    W, hop = r.geom["W"], r.geom["hop"]
    n_bad = sum(1 for w in r.windows if w["start"] - (W - 1) <= 301 <= w["start"])
    assert want_nan.sum() == n_bad * hop and 0 < n_bad < len(r.windows)
    blk = _blk(dtype, **settings)
    got = _run(blk, x, cuts=[333])
    assert np.array_equal(np.isnan(got), want_nan)
    ok = r.mask() & ~want_nan
    assert _errors(got, r)[ok].max() <= BAR[dtype]
    assert blk.stats() == (len(r.windows), n_bad)


def test_stats_counts_the_windows_of_every_call():
    blk = _blk("f32")  # hop 16
    xd = torch.zeros(100, dtype=torch.float32, device="cuda")
    assert blk.stats() == (0, 0)
    blk.process_bulk(xd[:1])
    assert blk.stats() == (1, 0)
    blk.process_bulk(xd[:15])
    assert blk.stats() == (1, 0)
    blk.process_bulk(xd[:33])  # samples 16 ... 48: windows at 16, 32 and 48
    assert blk.stats() == (4, 0)


def test_overlapping_buffers_are_rejected():
    from gnuradio4_amd import capi
    blk = _blk("f32")
    buf = torch.zeros(300, dtype=torch.float32, device="cuda")
    with pytest.raises(capi.Gr4HipError) as e:
        blk.process_bulk(buf[:200], out=buf[100:])
    assert e.value.status == capi.INVALID_ARGUMENT
    with pytest.raises(capi.Gr4HipError):
        blk.process_bulk(buf[:200], out=buf[:200])
    assert blk.stats() == (0, 0)


def test_two_handles_on_two_streams_agree_with_themselves():
    xa, ra = SV.case("A", "f32")
    xc, rc = SV.case("D", "c32")
    one_a = _run(_blk("f32", **SV.CASES["A"][3]), xa, cuts=[500])
    one_c = _run(_blk("c32", **SV.CASES["D"][3]), xc, cuts=[300])
    ba, bc = _blk("f32", **SV.CASES["A"][3]), _blk("c32", **SV.CASES["D"][3])
    da, dc = torch.from_numpy(np.array(xa)).cuda(), torch.from_numpy(np.array(xc)).cuda()
    sa, sc = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs_a, outs_c = [], []
    for (a0, a1), (c0, c1) in zip(((0, 500), (500, len(xa))), ((0, 300), (300, len(xc)))):
        with torch.cuda.stream(sa):
            outs_a.append(ba.process_bulk(da[a0:a1]))
        with torch.cuda.stream(sc):
            outs_c.append(bc.process_bulk(dc[c0:c1]))
    sa.synchronize()
    sc.synchronize()
    assert np.array_equal(_bits(torch.cat(outs_a).cpu().numpy()), _bits(one_a))
    assert np.array_equal(_bits(torch.cat(outs_c).cpu().numpy()), _bits(one_c))
    assert _errors(one_a, ra)[ra.mask()].max() <= BAR["f32"] and _errors(one_c, rc)[rc.mask()].max() <= BAR["c32"]
