"""gr4hip_fir_batched_process's dispatch (csrc/fir_batched.hip): which of its three kernel paths serves a call, what its guard marks per channel and segment, and whether
row strides, carried histories and channels stay apart.  Every call asserts the path that served it, read from the library's test hook
gr4hip_internal_fir_batched_last_paths (bit 1: two-term f16, bit 2: three-term bf16, bit 3: f32 MFMA; bit 0: a second evaluation on the FP64 matrix pipe was enqueued
behind it), and the marks of the last call come from gr4hip_internal_fir_batched_last_flags ([nch][ceil(n / 4096)] bytes; 1: sample spread, 2: non-finite sample,
3: rejected by the guard).  Every result is compared per channel with the float64 oracle under the parity contract's bar (include/gr4hip.h): 1e-5, or under a rejected
tone the error of the reference's own float32 sum where that is larger, factor one.  Every call's input and output are views into larger allocations: the output
allocation outside the rows' [0, n) must keep its sentinel bit for bit, the input allocation must stay as it was."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
X2, F16, BF16, F32 = 0, 1, 2, 3  # bits of the path record
SEG = 4096                       # outputs per guard segment (fir_f16.hip kHfSeg; the tail's judge takes the same)
SENT = 0x4B1D5EED                # the output allocations' sentinel (as float32: 10313453.0)


def _rel(got, truth):
    """THE parity metric (include/gr4hip.h, "PARITY CONTRACT"): max_k |got_k - truth_k| / max(|truth_k|, rms(truth))"""
    got = np.asarray(got).astype(np.float64).ravel()
    truth = np.asarray(truth).ravel()
    rms = np.sqrt(np.mean(np.abs(truth) ** 2))
    return float(np.max(np.abs(got - truth) / np.maximum(np.abs(truth), rms if rms > 0 else 1.0)))


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


@pytest.fixture
def devsw(G):
    """developer switches of the library, restored when the test ends"""
    used = set()

    def set_(name, value=1):
        used.add(name)
        G.capi.developer_switch(name, value)
    yield set_
    for name in used:
        G.capi.developer_switch(name, 0)


def _paths(G, f):
    """the bits of the last call's path record, as a sorted tuple"""
    fn = G.capi.lib().gr4hip_internal_fir_batched_last_paths  # (test hook, not in include/gr4hip.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint)]
    m = C.c_uint(0xFFFFFFFF)
    assert fn(f._h, C.byref(m)) == 0
    return tuple(k for k in range(32) if m.value >> k & 1)


def _flags(G, f):
    """the last call's marks [nch][nsegs] (nsegs = 0: the call made none)"""
    fn = G.capi.lib().gr4hip_internal_fir_batched_last_flags  # (test hook, not in include/gr4hip.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]
    nch, nsegs = C.c_size_t(0), C.c_size_t(0)
    assert fn(f._h, None, 0, C.byref(nch), C.byref(nsegs), None) in (0, G.capi.INVALID_ARGUMENT)  # (the sizes first)
    buf = np.full(max(nch.value * nsegs.value, 1), 0xEE, np.uint8)
    assert fn(f._h, buf.ctypes.data, buf.size, C.byref(nch), C.byref(nsegs), None) == 0
    return buf[:nch.value * nsegs.value].reshape(nch.value, nsegs.value).copy()


def _up4(n):
    return (n + 3) // 4 * 4


def _call(G, f, x, want, in_pad=0, out_pad=0, xoff=0, fill=0.0, contiguous=False):
    """one gr4hip_fir_batched_process call on x [nch][n] -> (y, flags).  The rows of the input lie _up4(n) + in_pad floats apart (contiguous: n), the first of them `xoff`
    floats past a 16-byte boundary, everything between and around them holds `fill`; the output rows lie _up4(n) + out_pad apart in an allocation of sentinels.
    Asserts the path record, the sentinels and that the input allocation is unchanged."""
    nch, n = x.shape
    istr, ostr = (n if contiguous else _up4(n) + in_pad), _up4(n) + out_pad
    xbuf = torch.full((nch * istr + 8,), fill, dtype=torch.float32, device="cuda")
    xin = xbuf[xoff:xoff + nch * istr].view(nch, istr)[:, :n]
    xin.copy_(torch.from_numpy(np.ascontiguousarray(x, np.float32)))
    before = xbuf.view(torch.int32).clone()
    obuf = torch.full((nch * ostr + 8,), SENT, dtype=torch.int32, device="cuda")
    out = obuf[:nch * ostr].view(torch.float32).view(nch, ostr)[:, :n]
    assert (xin.data_ptr() % 16 == 0) == (xoff % 4 == 0) and out.data_ptr() % 16 == 0
    if nch > 1:
        assert xin.stride(0) == istr and out.stride(0) == ostr
    y = f.process_bulk(xin, out)
    assert y.data_ptr() == out.data_ptr() and y.shape == (nch, n)
    got = _paths(G, f)
    fl = _flags(G, f)
    torch.cuda.synchronize()
    assert got == tuple(sorted(want)), (got, want, n, istr, xoff)
    ob = obuf.cpu().numpy()
    rows = ob[:nch * ostr].reshape(nch, ostr)
    assert (rows[:, n:] == SENT).all() and (ob[nch * ostr:] == SENT).all(), "a store outside the rows' [0, n)"
    assert torch.equal(xbuf.view(torch.int32), before), "the input allocation was written"
    return rows[:, :n].view(np.float32).copy(), fl


def _lowpass(nch, ntaps, fc0=0.2, dfc=0.0):
    return np.stack([O.design_taps_hamming_lowpass(ntaps, fc0 + dfc * c) for c in range(nch)])


def _noise(nch, n, seed):
    return np.stack([O.signal_f32(seed + c, n, tone_frel=0.03) for c in range(nch)])


def _tone(n, seed, amp):
    """weak noise under a strong tone at 0.31 cycles / sample, which every low-pass here rejects"""
    rng = np.random.default_rng(seed)
    return (0.05 * rng.standard_normal(n) + amp * np.cos(2 * np.pi * 0.31 * np.arange(n))).astype(np.float32)


def _truth(b, x):
    return [O.fir(b[c], x[c])[0] for c in range(len(b))]


def _ref32_err(b, x, truth):
    """per channel the error of the REFERENCE's own float32 sum, in the reference's order (oracle gr4o_fir_f32), against the float64 evaluation"""
    return [_rel(O.fir(b[c], x[c], acc64=False)[0], truth[c]) for c in range(len(b))]


class _Stream:
    """one handle fed the consecutive spans of x [nch][total]; each call chooses its own alignment and row strides (fresh allocations)"""

    def __init__(self, G, f, x):
        self.G, self.f, self.x, self.pos, self.ys, self.flags = G, f, x, 0, [], []

    def __call__(self, n, want, **kw):
        y, fl = _call(self.G, self.f, self.x[:, self.pos:self.pos + n], want, **kw)
        self.ys.append(y)
        self.flags.append(fl)
        self.pos += n

    def y(self):
        return np.concatenate(self.ys, axis=1)


# ------------------------------------------------------------------ a. routing table: one case per row of the dispatcher's conditions
# the f16 kernel judges itself; the bf16 kernel is judged by the dispatcher's tail (fir_judge_kernel per channel and segment); both are followed by fir_exact_kernel on the
# marks.  The f32 MFMA kernel stands alone (section e)
_F16 = (F16, X2)
_BF16 = (BF16, X2)
_F32 = (F32,)
# (id, ntaps, switch, NaN tap in channel 1, calls): calls are (n, kwargs of _call, paths expected); at least two per case, the second from a carried history
_ROUTES = [(f"f16_{k}taps_KS{max(3, (k + 46) // 32)}", k, None, False, [(40_000, {}, _F16), (33_001, {}, _F16)]) for k in (33, 81, 82, 129, 160, 200, 230, 256)] + [
    ("bf16_200taps_no_f16x2", 200, "GR4HIP_FIR_NO_F16X2", False, [(40_000, {}, _BF16), (33_001, {}, _BF16)]),
    ("bf16_256taps_no_f16x2", 256, "GR4HIP_FIR_NO_F16X2", False, [(40_000, {}, _BF16), (33_001, {}, _BF16)]),
    ("bf16_64taps_no_f16x2", 64, "GR4HIP_FIR_NO_F16X2", False, [(40_000, {}, _BF16), (33_001, {}, _BF16)]),
    ("f32_200taps_no_bf16x3", 200, "GR4HIP_FIR_NO_BF16X3", False, [(40_000, {}, _F32), (33_001, {}, _F32)]),
    ("threshold_32767_f32_32768_f16", 200, None, False, [(32_767, {}, _F32), (32_768, {}, _F16), (32_764, {"contiguous": True}, _F32), (32_768, {"contiguous": True}, _F16)]),
    ("one_sample_into_a_ninth_segment_f16", 200, None, False, [(8 * SEG + 1, {}, _F16), (8 * SEG + 1, {}, _F16)]),
    ("f32_32taps_long_span", 32, None, False, [(40_000, {}, _F32), (33_001, {}, _F32)]),
    ("f32_1tap_long_span", 1, None, False, [(40_000, {}, _F32), (33_001, {}, _F32)]),
    ("f32_input_one_float_past_16_bytes", 200, None, False, [(40_000, {"xoff": 1}, _F32), (40_000, {}, _F16), (33_001, {"xoff": 1}, _F32)]),
    ("f32_row_stride_not_a_multiple_of_4", 200, None, False, [(40_001, {"contiguous": True}, _F32), (40_001, {"contiguous": True}, _F32)]),
    ("bf16_nan_tap_in_one_channel", 200, None, True, [(40_000, {}, _BF16), (33_001, {}, _BF16)]),
]


def test_routing_table_reaches_every_path():
    seen = set()
    for case in _ROUTES:
        for call in case[-1]:
            seen.update(call[2])
    assert {X2, F16, BF16, F32} <= seen
    assert {max(3, (r[1] + 46) // 32) for r in _ROUTES if r[0].startswith("f16_")} == set(range(3, 10))  # every window width of fir_f16_make_afrag


@pytest.mark.parametrize("cid,ntaps,switch,nan_tap,calls", _ROUTES, ids=[r[0] for r in _ROUTES])
def test_batched_routing_table(G, devsw, cid, ntaps, switch, nan_tap, calls):
    nch = 3
    b = _lowpass(nch, ntaps, 0.1, 0.05) if ntaps > 1 else np.array([[0.5], [-2.0], [1.25]], np.float32)
    if nan_tap:
        b[1, ntaps // 3] = np.nan
    x = _noise(nch, sum(c[0] for c in calls), 1000 + ntaps)
    f = G.FirBatched(b)
    if switch:
        devsw(switch)
    s = _Stream(G, f, x)
    for n, kw, want in calls:
        s(n, want, **kw)
    y, truth = s.y(), _truth(b, x)
    for c in range(nch):
        if nan_tap and c == 1:  # the reference's sum holds the NaN tap in every output
            assert np.isnan(truth[c]).all() and np.isnan(y[c]).all()
            continue
        e = _rel(y[c], truth[c])
        assert e <= TOL, (cid, c, e)


# ------------------------------------------------------------------ b. hand-offs between the paths on one handle; channel counts; refusals
@pytest.mark.parametrize("nch", [1, 3, 64])
def test_batched_handoffs(G, devsw, nch):
    """f16 -> f32 (short) -> bf16 (switch) -> f32 (misaligned) -> f16 -> f16, cut at positions that are no multiples of 4096 or of 16: the concatenation of every channel
    is the oracle's stream; then reset() and the head of the stream again"""
    ntaps = 200
    b = _lowpass(nch, ntaps, 0.05, 0.3 / nch)
    cuts = [40_003, 9_001, 35_007, 33_333, 40_005, 32_771]
    x = _noise(nch, sum(cuts), 2000 + nch)
    f = G.FirBatched(b)
    s = _Stream(G, f, x)
    s(cuts[0], _F16)
    s(cuts[1], _F32, in_pad=4)
    devsw("GR4HIP_FIR_NO_F16X2")
    s(cuts[2], _BF16, out_pad=8)
    devsw("GR4HIP_FIR_NO_F16X2", 0)
    s(cuts[3], _F32, xoff=1)
    s(cuts[4], _F16, in_pad=SEG + 8, out_pad=4)
    s(cuts[5], _F16)
    y, truth = s.y(), _truth(b, x)
    errs = [_rel(y[c], truth[c]) for c in range(nch)]
    assert max(errs) <= TOL, errs
    f.reset()
    s2 = _Stream(G, f, x)
    s2(cuts[0], _F16)
    s2(cuts[1], _F32)
    y2 = s2.y()
    errs = [_rel(y2[c], truth[c][:y2.shape[1]]) for c in range(nch)]
    assert max(errs) <= TOL, errs


def test_batched_1024_channels(G):
    """grid.y = 1024 and fir_exact_launch's gx = max(1, 4 n_cu / nch) at its small end: 1024 channels x 33 taps x 32768 samples on the f16 path, then a short span on the
    f32 path from the carried histories; three of the channels carry a rejected tone, so the second evaluation has marks to serve"""
    nch, ntaps, n0, n1 = 1024, 33, 32_768, 4_100
    b = _lowpass(nch, ntaps, 0.05, 0.15 / nch)
    rng = np.random.default_rng(77)
    x = rng.standard_normal((nch, n0 + n1)).astype(np.float32)
    tones = (5, 517, 1023)
    for c in tones:
        x[c] = _tone(n0 + n1, 300 + c, 30.0)
    f = G.FirBatched(b)
    s = _Stream(G, f, x)
    s(n0, _F16)
    fl = s.flags[0]
    s(n1, _F32)
    y, truth = s.y(), _truth(b, x)
    ref32 = {c: _rel(O.fir(b[c], x[c], acc64=False)[0], truth[c]) for c in tones}
    errs = np.array([_rel(y[c], truth[c]) for c in range(nch)])
    bars = np.array([max(TOL, ref32.get(c, 0.0)) for c in range(nch)])
    assert (errs <= bars).all(), [(c, errs[c], bars[c]) for c in np.nonzero(errs > bars)[0][:8]]
    assert fl.shape == (nch, n0 // SEG)
    plain = np.ones(nch, bool)
    plain[list(tones)] = False
    assert not fl[plain].any() and all((fl[c, 1:] == 3).all() for c in tones), "marks in the wrong rows"


def test_batched_create_refuses_what_the_device_path_cannot_take(G):
    for shape in ((2, 257), (65536, 1)):
        with pytest.raises(G.capi.Gr4HipError) as e:
            G.FirBatched(np.ones(shape, np.float32))
        assert e.value.status == G.capi.UNSUPPORTED
    G.FirBatched(np.ones((2, 256), np.float32))


# ------------------------------------------------------------------ c. row strides
@pytest.mark.parametrize("pad", [4, SEG + 8])
@pytest.mark.parametrize("path", ["f16", "bf16", "f32"])
def test_batched_row_strides(G, devsw, path, pad):
    """in_stride > n and out_stride > n on each path, two calls with the history carried; the gaps between the input rows hold 0, 1e30 and NaN in turn: nothing of a
    channel's result, path or marks may change (a buffer resource or a history read that crosses a row end would), and every run meets the bar.  Channel 1 carries a
    rejected tone, so the second evaluation reads strided rows as well."""
    nch, ntaps = 3, 200
    n = (36_868, 33_004) if path != "f32" else (9_004, 5_000)
    want = {"f16": _F16, "bf16": _BF16, "f32": _F32}[path]
    b = _lowpass(nch, ntaps)
    x = _noise(nch, sum(n), 3000)
    x[1] = _tone(sum(n), 3001, 30.0)
    truth = _truth(b, x)
    ref32 = _ref32_err(b, x, truth)
    if path == "bf16":
        devsw("GR4HIP_FIR_NO_F16X2")
    runs = []
    for fill in (0.0, 1e30, float("nan")):
        f = G.FirBatched(b)
        s = _Stream(G, f, x)
        for k in n:
            s(k, want, in_pad=pad, out_pad=pad, fill=fill)
        runs.append((s.y(), s.flags))
    y0, fl0 = runs[0]
    for c in range(nch):
        e = _rel(y0[c], truth[c])
        assert e <= max(TOL, ref32[c]), (path, pad, c, e, ref32[c])
    for y, fl in runs[1:]:
        assert np.array_equal(y.view(np.uint32), y0.view(np.uint32)), "the gap between the rows was read"
        assert all(np.array_equal(a, b_) for a, b_ in zip(fl, fl0))
    if path == "f32":
        assert all(fl.shape == (nch, 0) for fl in fl0)  # (no marks: that kernel is not judged)
    else:
        assert all((fl[1, 1:k // SEG] == 3).all() and not fl[0].any() and not fl[2].any() for fl, k in zip(fl0, n)), fl0


# ------------------------------------------------------------------ d. the guard, per channel
N_GUARD = 40 * SEG + 37
P_NAN, P_INF, P_OUT = 10_000, 40 * SEG + 20, 70_000                 # bad samples: NaN, Inf (in the last, partial segment), a 1e30 outlier
RUN = (5 * SEG + 1_000, 27 * SEG + 2_000)                           # the switching channel's rejected run: 22 segments, starting and ending in mid segment
TONE1000, NOISE, NANINF, BIG, ZERO, SWITCH, TONE30, OUTLIER, SMALL = range(9)


def _mixture(seed):
    """nine channels, one of each kind, in no particular order"""
    n = N_GUARD
    x = _noise(9, n, seed)
    x[TONE1000] = _tone(n, seed + 20, 1000.0)
    x[TONE30] = _tone(n, seed + 21, 30.0)
    x[NANINF, P_NAN] = np.nan
    x[NANINF, P_INF] = np.inf
    x[BIG] *= np.float32(1e20)
    x[SMALL] *= np.float32(1e-20)
    x[ZERO] = 0
    x[SWITCH, RUN[0]:RUN[1]] = _tone(RUN[1] - RUN[0], seed + 22, 30.0)
    x[OUTLIER, P_OUT] = 1e30
    return x


def _segments_staging(p, ntaps):
    """the segments of the f16 kernel whose staged window [4096 s - Hb, 4096 s + 4096) holds sample p (Hb = 32 KS - 16, KS as fir_f16_make_afrag chooses it)"""
    hb = 32 * max(3, (ntaps + 46) // 32) - 16
    return [s for s in range(-(-N_GUARD // SEG)) if s * SEG - hb <= p < (s + 1) * SEG]


@pytest.mark.parametrize("replicas", [1, 35], ids=["9ch", "315ch"])
@pytest.mark.parametrize("ntaps", [200, 64])
def test_batched_guard_per_channel(G, ntaps, replicas):
    """the f16 path's guard on a mixture of channels.  With 35 replicas of the mixture (315 channels) a workgroup runs 12 .. 25 consecutive segments of its channel, so the
    streak -- two rejections in a row, then the first evaluation is skipped but for every eighth segment -- works across the switching channel's run and past its end; with
    9 channels a workgroup has one segment.  Replicas are compared bit for bit with the first one, the first with the oracle."""
    n, nsegs = N_GUARD, -(-N_GUARD // SEG)
    b = _lowpass(9, ntaps, 0.2, 0.005)
    x = _mixture(4000 + ntaps)
    truth = _truth(b, x)
    r32 = [O.fir(b[c], x[c], acc64=False)[0] for c in range(9)]
    f = G.FirBatched(np.tile(b, (replicas, 1)))
    yall, flall = _call(G, f, np.tile(x, (replicas, 1)), _F16)
    for r in range(1, replicas):
        assert np.array_equal(yall[9 * r:9 * r + 9].view(np.uint32), yall[:9].view(np.uint32)) and np.array_equal(flall[9 * r:9 * r + 9], flall[:9]), r
    y, fl = yall[:9], flall[:9]
    assert fl.shape == (9, nsegs)
    # parity: every channel over its whole length, the bar the reference's own float32 error where that is above 1e-5
    bad = ~np.isfinite(r32[NANINF])
    want_bad = np.zeros(n, bool)
    want_bad[P_NAN:P_NAN + ntaps] = True
    want_bad[P_INF:] = True
    assert np.array_equal(bad, want_bad) and bad.sum() == ntaps + (n - P_INF) <= 512  # (the Inf's window is cut by the end of the span)
    for c in range(9):
        sl = ~bad if c == NANINF else slice(None)
        ref = _rel(r32[c][sl], truth[c][sl])
        e = _rel(y[c][sl], truth[c][sl])
        print(f"guard ntaps={ntaps} x{replicas} ch{c}: err {e:.3g} ref32 {ref:.3g} ratio {e / ref if ref else 0:.3g}")
        assert e <= max(TOL, ref), (c, e, ref)
    assert np.array_equal(~np.isfinite(y[NANINF]), bad), "non-finite outputs are not the reference's"
    assert not y[ZERO].any()
    clear = np.ones(n, bool)
    clear[P_OUT:P_OUT + ntaps] = False
    e, ref = _rel(y[OUTLIER][clear], truth[OUTLIER][clear]), _rel(r32[OUTLIER][clear], truth[OUTLIER][clear])
    assert e <= max(TOL, ref), ("outlier channel away from the outlier", e, ref)
    # marks
    for c in (TONE1000, TONE30):
        assert (fl[c, 1:nsegs - 1] == 3).all(), (c, fl[c])
    assert (fl[BIG] == 3).all() and (fl[SMALL] == 3).all(), (fl[BIG], fl[SMALL])  # powers outside float32's range: handed to the second evaluation unjudged
    assert not fl[NOISE].any() and not fl[ZERO].any(), (fl[NOISE], fl[ZERO])
    want = np.zeros(nsegs, np.uint8)
    want[_segments_staging(P_NAN, ntaps) + _segments_staging(P_INF, ntaps)] = 2
    assert np.array_equal(fl[NANINF], want), fl[NANINF]
    want = np.zeros(nsegs, np.uint8)
    want[_segments_staging(P_OUT, ntaps)] = 1
    assert np.array_equal(fl[OUTLIER], want), fl[OUTLIER]
    first_in, last_in = -(-RUN[0] // SEG), RUN[1] // SEG - 1  # segments wholly inside the run (their staged history may reach in front of it: one more)
    assert (fl[SWITCH, first_in + 1:last_in + 1] == 3).all(), fl[SWITCH]
    assert not fl[SWITCH, :RUN[0] // SEG].any() and not fl[SWITCH, RUN[1] // SEG + 9:].any(), fl[SWITCH]  # (a probe every eighth segment ends the streak behind the run)


def test_batched_channels_are_independent(G):
    """the neighbours of a rejected, a non-finite and a 1e+20 channel are bit-identical, marks included, to the same channels in a batch where those three carry
    ordinary noise: nothing leaks through shared LDS statistics or a neighbour's row of marks"""
    ntaps = 200
    b = _lowpass(9, ntaps, 0.2, 0.005)
    x = _mixture(4200)
    x2 = x.copy()
    swapped = (TONE1000, NANINF, BIG)
    for c in swapped:
        x2[c] = O.signal_f32(4300 + c, N_GUARD, tone_frel=0.03)
    ya, fa = _call(G, G.FirBatched(b), x, _F16)
    yb, fb = _call(G, G.FirBatched(b), x2, _F16)
    keep = [c for c in range(9) if c not in swapped]
    assert np.array_equal(ya[keep].view(np.uint32), yb[keep].view(np.uint32)) and np.array_equal(fa[keep], fb[keep])
    assert not fb[list(swapped)].any() and fa[list(swapped)].any(axis=1).all()


def test_batched_per_channel_tap_scales(G):
    """taps at 1e-6, 1 and 1e+3 and an all-zero row in one handle: the table's block exponent is per channel; zero taps give exactly zero"""
    ntaps, n = 200, 36_868
    b = _lowpass(4, ntaps, 0.15, 0.02) * np.array([1e-6, 1.0, 1e3, 0.0], np.float32)[:, None]
    x = _noise(4, 2 * n, 4400)
    f = G.FirBatched(b)
    s = _Stream(G, f, x)
    s(n, _F16)
    s(n, _F16)
    y, truth = s.y(), _truth(b, x)
    errs = [_rel(y[c], truth[c]) for c in range(3)]
    assert max(errs) <= TOL and not y[3].any(), errs


# ------------------------------------------------------------------ e. the contract where the kernel does not judge itself
_UNJUDGED = [
    ("f32_short_span_200", 200, None, (9_000, 9_000), {}, _F32),
    ("f32_short_span_64", 64, None, (9_000, 9_000), {}, _F32),
    ("f32_24_taps", 24, None, (40_004, 33_000), {}, _F32),
    ("f32_32_taps", 32, None, (40_004, 33_000), {}, _F32),
    ("f32_misaligned_200", 200, None, (40_003, 33_000), {"xoff": 1}, _F32),
    ("f32_misaligned_64", 64, None, (40_003, 33_000), {"xoff": 1}, _F32),
    ("f32_n_40001_200", 200, None, (40_001, 40_001), {"contiguous": True}, _F32),
    ("bf16_200", 200, "GR4HIP_FIR_NO_F16X2", (40_004, 33_000), {}, _BF16),
    ("bf16_64", 64, "GR4HIP_FIR_NO_F16X2", (40_004, 33_000), {}, _BF16),
]


@pytest.mark.parametrize("cid,ntaps,switch,spans,kw,want", _UNJUDGED, ids=[u[0] for u in _UNJUDGED])
def test_batched_contract_on_the_unjudged_paths(G, devsw, cid, ntaps, switch, spans, kw, want):
    """a tone 50 / 80 dB above what the filter passes where the dispatcher takes the f32 MFMA or the bf16 kernel, neither of which judges itself.  The bar is the
    contract's: max(1e-5, the reference's float32 error), factor one.  Measured on an MI355X as the kernels stood, worst err / ref32_err over the tone channels:
      f32 MFMA  0.49 .. 0.53 in every case (9 000-sample spans of 200 / 64 taps, 24 and 32 taps on a long span, the misaligned input with 200 / 64 taps, n = 40 001):
                float32 products summed four at a time beat the reference's sequential sum by a factor of two -- that kernel is left alone and marks nothing;
      bf16      0.62 with 200 taps, 1.48 (amplitude 30) and 1.52 (amplitude 1000) with 64 taps (4.3e-5 and 5.4e-5 against 2.9e-5 and 3.5e-5): over the bar -- the dispatcher
                now judges that kernel's output per channel and segment (fir_judge_kernel) and evaluates the marked segments again (fir_exact_kernel); bit 0 of the path
                record reports it, and the rejected channels' marks are asserted below."""
    b = _lowpass(3, ntaps)
    n = sum(spans)
    x = np.stack([_tone(n, 5000 + ntaps, 30.0), O.signal_f32(5001 + ntaps, n, tone_frel=0.03), _tone(n, 5002 + ntaps, 1000.0)])
    truth = _truth(b, x)
    ref32 = _ref32_err(b, x, truth)
    if switch:
        devsw(switch)
    f = G.FirBatched(b)
    s = _Stream(G, f, x)
    for k in spans:
        s(k, want, **kw)
    y = s.y()
    errs = [_rel(y[c], truth[c]) for c in range(3)]
    for c in range(3):
        print(f"unjudged {cid} ch{c}: err {errs[c]:.3g} ref32 {ref32[c]:.3g} ratio {errs[c] / ref32[c]:.3g}")
    assert all(e <= max(TOL, r) for e, r in zip(errs, ref32)), (cid, errs, ref32)
    if BF16 in want:
        assert all((fl[0, 1:k // SEG] == 3).all() and (fl[2, 1:k // SEG] == 3).all() and not fl[1].any() for fl, k in zip(s.flags, spans)), s.flags
    else:
        assert all(fl.shape == (3, 0) for fl in s.flags)
