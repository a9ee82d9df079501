"""SchmittTrigger on the device (csrc/schmitt_trigger.hip) against the plain-Python restatement in tests/schmitt_trigger_oracle.py.

Every comparison is EXACT: the count, `sample`, the kind, `edge_idx`, `n_fit`, the flags and the bits of `edge_offset`.  That is derived, not measured: the
automaton is comparisons of the same values against the same thresholds, and a fit is the same correctly rounded float (double for float64) operations in the
same order on both sides (the kernel file is compiled without contraction).  A last-bit difference means a contracted or reordered operation in the kernel.

The random streams are a sine plus noise with a band four noise sigmas wide; the tests assert on the ORACLE's output first that none of its fits is degenerate,
so the flag cannot excuse a mismatch.  The degenerate path is tested by its constructed input only."""
import functools

import numpy as np
import pytest
import torch

import schmitt_trigger_oracle as ST

pytestmark = pytest.mark.gpu

NO, BASIC, LINEAR = ST.NO_INTERPOLATION, ST.BASIC_LINEAR_INTERPOLATION, ST.LINEAR_INTERPOLATION
METHODS = [NO, BASIC, LINEAR]
R, F = ST.RISING, ST.FALLING
FIELDS = ("sample", "kind", "edge_idx", "edge_offset", "n_fit", "flags")
TORCH = {np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


@functools.lru_cache(maxsize=None)
def S():
    import gnuradio4_amd as G
    return G.SchmittTrigger.segment()


@functools.lru_cache(maxsize=None)
def walk_tile():
    """segments per workgroup of the carry walk (gr4hip_schmitt_walk_tile)"""
    import gnuradio4_amd as G
    return G.SchmittTrigger.walk_tile()


def _blk(offset, threshold, method, dtype=np.float32):
    import gnuradio4_amd as G
    return G.SchmittTrigger(offset, threshold, method, TORCH[np.dtype(dtype)])


def _np(e):
    return {"count": e.count, **{k: getattr(e, k).cpu().numpy() for k in FIELDS}}


def _join(parts, starts):
    out = {"count": sum(p["count"] for p in parts)}
    for k in FIELDS:
        out[k] = np.concatenate([p[k] + s if k == "sample" else p[k] for p, s in zip(parts, starts)])
    return out


def _run(blk, x, cuts=()):
    """x through blk (the device block or the oracle), cut into calls at `cuts`; the edges re-based to the stream"""
    dev = not isinstance(blk, ST.SchmittTrigger)
    xd = torch.from_numpy(np.array(x)).cuda() if dev else x
    marks = [0, *cuts, len(x)]
    parts = [_np(blk.process_bulk(xd[a:b])) if dev else blk.process(xd[a:b]) for a, b in zip(marks[:-1], marks[1:])]
    return _join(parts, marks[:-1])


def _assert_equal(got, want, upto=None):
    assert got["count"] == want["count"], (got["count"], want["count"])
    for k in FIELDS:
        a, b = got[k][:upto], want[k][:upto]
        if k == "edge_offset":
            a, b = a.view(np.int32), b.view(np.int32)
        bad = np.flatnonzero(a != b) if a.shape == b.shape else None
        assert bad is not None and bad.size == 0, (k, a.shape, b.shape, None if bad is None else [(int(j), got[k][j], want[k][j], want["sample"][j]) for j in bad[:5]])


def _parity(x, offset, threshold, method, cuts=(), clean=True):
    dtype = x.dtype
    want = _run(ST.SchmittTrigger(offset, threshold, method, dtype), x, cuts)
    if clean:
        assert np.all(want["flags"] == 0), "the generator must give the oracle no degenerate fit"
    got = _run(_blk(offset, threshold, method, dtype), x, cuts)
    _assert_equal(got, want)
    return want


@functools.lru_cache(maxsize=None)
def _noisy(n, seed=7, dtype=np.float32, scale=1.0):
    """a sine of period 37.3 samples plus noise of sigma 0.05; the tests' band is 0.1 +- 0.2: four sigmas wide"""
    rng = np.random.default_rng(seed)
    x = (scale * (np.sin(2 * np.pi * np.arange(n) / 37.3) + 0.05 * rng.standard_normal(n))).astype(dtype)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ constructed streams: band -1 ... 1, resting at -2 or 2
def _wobble(k):
    return 0.03 * np.sin(0.9 * np.arange(k))


def _rise(x, entry, hit):
    """low -> high: the zone is entered at `entry` (-2 -> inside the band), the samples up to `hit` climb inside the band, x[hit] = 2 is the edge"""
    k = hit - entry
    x[entry:hit] = np.linspace(-0.6, 0.6, k, endpoint=False) + _wobble(k)
    x[hit:] = 2.0


def _fall(x, entry, hit):
    k = hit - entry
    x[entry:hit] = np.linspace(0.6, -0.6, k, endpoint=False) + _wobble(k)
    x[hit:] = -2.0


def _resting(n, dtype=np.float32):
    return np.full(n, -2.0, dtype)


def _scaled(x, dtype):
    """the constructed streams for the other sample types: the integer ones in thousandths (band -1000 ... 1000)"""
    return (x.astype(np.float64) * 1000.0).astype(dtype) if np.dtype(dtype).kind == "i" else x.astype(dtype)


def _band(dtype):
    return (0, 1000) if np.dtype(dtype).kind == "i" else (0.0, 1.0)


# ------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("method", METHODS)
def test_lengths(method):
    s = S()
    for n in (0, 1, 31, 32, 33, s - 1, s, s + 1, 3 * s + 17):
        want = _parity(_noisy(3 * s + 17)[:n], 0.1, 0.2, method)
        assert want["count"] > 500 or n < 3 * s


# ------------------------------------------------------------------------------------------------ zones across boundaries
def _zone_stream(entry, hit, n):
    x = _resting(n)
    _rise(x, entry, hit)
    _fall(x, hit + 40, hit + 47)
    return x


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", ["next_segment", "two_segments_later", "lane_run", "first_sample_of_segment"])
def test_zone_across_a_boundary(method, case):
    s = S()
    entry, hit = {"next_segment": (s - 3, s + 2),               # entered in the last lane-run of a segment, threshold reached in the first run of the next
                  "two_segments_later": (s - 3, 2 * s + 5),     # the zone spans a whole segment: accumulated clamps at 32
                  "lane_run": (16 * 5 - 2, 16 * 5 + 3),         # across a lane-run boundary inside a segment
                  "first_sample_of_segment": (s - 5, s)}[case]  # the edge on a segment's first sample: the fit window lies in the halo
    want = _parity(_zone_stream(entry, hit, 2 * s + 200), 0.0, 1.0, method)
    assert list(want["sample"]) == [hit, hit + 47] and list(want["kind"]) == [R, F]
    if method == LINEAR:
        assert list(want["n_fit"]) == [min(hit - entry + 1, 32), 8]


@pytest.mark.parametrize("method", METHODS)
def test_zone_entered_and_abandoned_across_a_boundary(method):
    s = S()
    x = _resting(2 * s + 50)
    x[s - 2:s + 3] = [-0.5, -0.2, 0.1, 0.3, 0.2]  # entered at s - 2, left again below the band at s + 3: no edge
    _rise(x, 2 * s - 1, 2 * s + 1)
    want = _parity(x, 0.0, 1.0, method)
    assert list(want["sample"]) == [2 * s + 1]
    if method == LINEAR:
        assert list(want["n_fit"]) == [3]  # accumulated from the second entry, not from the abandoned zone


@pytest.mark.parametrize("method", METHODS)
def test_edge_on_the_first_samples_of_a_call(method):
    """the fit window lies in the handle's history: the zone is entered five samples in front of a cut, the edge is the next call's first (second) sample"""
    s = S()
    for hit_in_call in (0, 1):
        cut = s + 77
        x = _zone_stream(cut - 5 + hit_in_call, cut + hit_in_call, 2 * s)
        want = _parity(x, 0.0, 1.0, method, cuts=(cut,))
        assert list(want["sample"])[:1] == [cut + hit_in_call]
        if method == LINEAR:
            assert want["n_fit"][0] == 6


# ------------------------------------------------------------------------------------------------ split calls
@pytest.mark.parametrize("method", METHODS)
def test_one_call_and_five_uneven_calls(method):
    s = S()
    x = _noisy(3 * s + 17)
    cuts = (20, s + 5, s + 16, 2 * s + 100)  # calls of 20, s - 15, 11, s + 84 and s - 83 samples: two shorter than the history
    whole = _run(_blk(0.1, 0.2, method), x)
    split = _run(_blk(0.1, 0.2, method), x, cuts)
    _assert_equal(split, whole)
    _assert_equal(whole, _parity(x, 0.1, 0.2, method, cuts))


# ------------------------------------------------------------------------------------------------ dense and empty outputs
def test_dense_output_and_capacity():
    from gnuradio4_amd import capi
    n = 2 * S() + 10
    x = np.where(np.arange(n) % 2 == 0, 2.0, -2.0).astype(np.float32)
    want = ST.SchmittTrigger(0.0, 1.0, NO, np.float32).process(x)
    assert want["count"] == n  # every sample is an edge
    xd = torch.from_numpy(np.array(x)).cuda()
    _assert_equal(_np(_blk(0.0, 1.0, NO).process_bulk(xd)), want)
    half = _blk(0.0, 1.0, NO).process_bulk(xd, capacity=n // 2)
    assert half.count == n and half.sample.numel() == n // 2
    _assert_equal(_np(half), want, upto=n // 2)
    # the guard words behind `capacity`, through the C entry on a buffer of this test's own
    guard = 0x5A5A5A5A
    buf = torch.full((n, capi.SCHMITT_EDGE_BYTES // 4), guard, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    blk = _blk(0.0, 1.0, NO)
    capi.check(capi.lib().gr4hip_schmitt_process(blk._h, xd.data_ptr(), n, buf.data_ptr(), n // 2, cnt.data_ptr(), torch.cuda.current_stream().cuda_stream), "process")
    assert int(cnt.item()) == n
    b = buf.cpu().numpy()
    assert np.all(b[n // 2:] == guard)
    assert np.array_equal(b[:n // 2, 0:2].copy().view(np.int64).ravel(), want["sample"][:n // 2]) and np.array_equal(b[:n // 2, 4], want["kind"][:n // 2])
    # the state advanced over the whole call: one more sample of the same sign as the last is no edge, the other sign is
    assert blk.process_bulk(xd[n - 1:n]).count == 0 and blk.process_bulk(xd[n - 2:n - 1]).count == 1


@pytest.mark.parametrize("method", METHODS)
def test_no_edges_at_all(method):
    x = (0.5 * _noisy(S() + 100)).astype(np.float32)  # never reaches 0.1 + 0.9
    want = _parity(x, 0.1, 0.9, method)
    assert want["count"] == 0


# ------------------------------------------------------------------------------------------------ a call longer than one tile of the carry walk
@functools.lru_cache(maxsize=None)
def _long_stream():
    s, tile = S(), walk_tile()
    n = (2 * tile + 1) * s + 5  # three workgroups of the walk: the second has one map per lane in front of its tile, the third two to compose
    x = _resting(n)
    plants = [(pos, pos + 9, pos + 50, pos + 70) for pos in range(9, n - 100, 37 * s + 11)]  # sparse edges, a rise and a fall per 37 segments: the ranks cross the tile edge
    for edge in (tile * s, 2 * tile * s):                                                    # and a zone open across each tile edge itself
        plants.append((edge - 4, edge + 3, edge + 2000, edge + 2005))
    for r0, r1, f0, f1 in sorted(plants):
        _rise(x, r0, r1)
        _fall(x, f0, f1)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("method", METHODS)
def test_a_call_longer_than_one_walk_tile(method):
    s, tile = S(), walk_tile()
    want = _parity(_long_stream(), 0.0, 1.0, method)
    assert want["count"] > 20 and np.any(want["sample"] < tile * s) and np.any(want["sample"] >= 2 * tile * s) and tile * s + 3 in want["sample"] and 2 * tile * s + 3 in want["sample"]


# ------------------------------------------------------------------------------------------------ reset, set_params
@pytest.mark.parametrize("method", METHODS)
def test_reset_and_set_params_mid_stream(method):
    s = S()
    x = _noisy(2 * s + 300)
    a, b = s + 13, s + 140
    dev, ora = _blk(0.1, 0.2, method), ST.SchmittTrigger(0.1, 0.2, method, np.float32)
    xd = torch.from_numpy(np.array(x)).cuda()
    for k, (lo, hi) in enumerate(((0, a), (a, b), (b, len(x)))):
        if k == 1:
            dev.reset()
            ora.reset()
        if k == 2:
            dev.set_params(offset=-0.2, threshold=0.4)  # resets the detector as settingsChanged does
            ora.set_params(-0.2, 0.4)
        want = ora.process(x[lo:hi])
        assert np.all(want["flags"] == 0) and want["count"] > 3
        _assert_equal(_np(dev.process_bulk(xd[lo:hi])), want)


# ------------------------------------------------------------------------------------------------ NaN, the degenerate fit
def test_nan_samples_hold_the_state():
    s = S()
    x = _noisy(s + 200).copy()
    x[::5] = np.nan
    x[s - 3:s + 9] = np.nan  # across the segment boundary
    want = _parity(x, 0.1, 0.2, NO)
    assert want["count"] > 50
    y = np.array([0.0, np.nan, 2.0, np.nan, np.nan, -2.0, np.nan], np.float32)
    assert list(_parity(y, 0.0, 1.0, NO)["sample"]) == [2, 5]


def test_zero_slope_fit_is_flagged_and_the_state_flips():
    want = _parity(ST.ZERO_SLOPE, 0.0, 1.0, LINEAR, clean=False)
    assert list(want["sample"]) == [4, 6] and list(want["kind"]) == [R, F] and list(want["flags"]) == [ST.DEGENERATE, 0]
    assert list(want["edge_idx"][:1]) == [0] and want["edge_offset"][0] == 0.0 and want["n_fit"][0] == 4
    # the same fit with its window in the halo of the next segment
    s = S()
    x = _resting(s + 10)
    x[s - 4:s + 3] = ST.ZERO_SLOPE
    want = _parity(x, 0.0, 1.0, LINEAR, clean=False)
    assert list(want["sample"]) == [s, s + 2] and list(want["flags"]) == [ST.DEGENERATE, 0]


# ------------------------------------------------------------------------------------------------ the other sample types
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float64])
def test_other_sample_types_across_a_boundary(method, dtype):
    s = S()
    offset, threshold = _band(dtype)
    x = _scaled(_zone_stream(s - 3, s + 2, s + 300), dtype)
    want = _parity(x, offset, threshold, method)
    assert list(want["sample"]) == [s + 2, s + 49] and list(want["kind"]) == [R, F]
    scale = 1000.0 if np.dtype(dtype).kind == "i" else 1.0
    y = _noisy(s + 517, 11, np.dtype(dtype).type, scale)
    want = _parity(y, 0.1 * scale, 0.2 * scale, method, cuts=(s - 9,))
    assert want["count"] > 100
    if method == LINEAR and np.dtype(dtype).kind == "i":
        assert np.all(want["edge_offset"] == 0.0)  # the integer truncation (:198)


def test_int16_range_is_checked_at_create():
    from gnuradio4_amd import capi
    for offset, threshold in ((32000, 1000), (-32000, 1000), (0.5, 1), (40000, 0)):
        with pytest.raises(capi.Gr4HipError) as e:
            _blk(offset, threshold, NO, np.int16)
        assert e.value.status == capi.INVALID_ARGUMENT
    blk = _blk(32000, 767, NO, np.int16)
    with pytest.raises(capi.Gr4HipError):
        blk.set_params(offset=32001)
    with pytest.raises(capi.Gr4HipError) as e:
        _blk(0.0, 1.0, ST.POLYNOMIAL_INTERPOLATION)
    assert e.value.status == capi.UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the longest call
def test_a_call_beyond_the_longest_is_refused_before_any_device_work():
    """GR4HIP_SCHMITT_MAX_SAMPLES (2^32): one more is GR4HIP_INVALID_ARGUMENT; nothing is read or written (the buffers here hold 8 samples and one edge), and the
    handle's state is untouched: the next call gives the edges of a fresh detector"""
    from gnuradio4_amd import capi
    blk = _blk(0.0, 1.0, NO)
    x = torch.tensor([0, 2, -2, 2, 0, 0, -2, 2], dtype=torch.float32, device="cuda")
    buf = torch.full((6,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = capi.lib().gr4hip_schmitt_process(blk._h, x.data_ptr(), (1 << 32) + 1, buf.data_ptr(), 1, cnt.data_ptr(), st)
    assert rc == capi.INVALID_ARGUMENT and "GR4HIP_SCHMITT_MAX_SAMPLES" in capi.lib().gr4hip_last_error().decode()
    torch.cuda.synchronize()
    assert int(cnt.item()) == -7 and bool(torch.all(buf == 0x5A5A5A5A))
    import oracle_lib
    hdr = open(oracle_lib.ROOT + "/include/gr4hip.h").read()
    assert "#define GR4HIP_SCHMITT_MAX_SAMPLES 4294967296ULL" in hdr
    _assert_equal(_np(blk.process_bulk(x)), ST.SchmittTrigger(0.0, 1.0, NO, np.float32).process(x.cpu().numpy()))
