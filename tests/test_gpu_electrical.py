"""PowerFactor and SystemUnbalance on the device (csrc/electrical.hip, include/gr4hip.h "Power factor and system unbalance") against tests/electrical_oracle.py:
power_factor and the three unbalance outputs bit for bit (NaN equal to NaN), the phase within its bound (POWER_QUALITY.md)."""
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import electrical_oracle as EO
import oracle_lib as O
import power_metrics_oracle as PM

pytestmark = pytest.mark.gpu

TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
TNAME = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
# the phase against the oracle (acos in float64 on the sample-type argument, rounded once), in units in the last place of the sample type.
#   float:  the device computes the same thing with its own float64 acos: 0.5 for each of the two roundings, a derived bound.
#   double: the device library's acos, measured on the inputs of this file on an MI355X; the bound is twice that (CONVERTERS.md: glibc, behind the oracle, is
#           itself up to 1 ulp from the true value, and the inputs are a finite sample).
PHASE_MEASURED_ULP_F64 = 1.0
PHASE_BOUND_ULP = {"f32": 1.0, "f64": 2.0 * PHASE_MEASURED_ULP_F64}


@functools.lru_cache(maxsize=None)
def tile():
    import gnuradio4_amd as G
    return G.PowerFactor.tile()


def _sizes():
    t = tile()
    return [0, 1, 5, t - 1, t + 3, 2 * t + 1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits_dev(a, b):
    """bit for bit on the device, two NaNs equal"""
    return a.shape == b.shape and bool(torch.all((_bits(a) == _bits(b)) | (torch.isnan(a) & torch.isnan(b))))


def _special_columns(dtype, rows, count, rng):
    """[rows, count] columns of the special-value grid: the whole grid where it fits, otherwise every-phase-+inf, every-phase-NaN and random grid points"""
    if 14 ** rows <= count:
        return EO.grid(dtype, rows)
    sp = EO.specials(dtype)
    cols = sp[rng.integers(0, sp.size, (rows, count))]
    if count > 0:
        cols[:, 0] = np.inf
    if count > 1:
        cols[:, 1] = np.nan
    return cols


def _splice(x, cols, at):
    """cols written into x from column max(at, 0) on, as far as they fit"""
    at = max(at, 0)
    k = max(min(cols.shape[1], x.shape[1] - at), 0)
    x[:, at:at + k] = cols[:, :k]


@functools.lru_cache(maxsize=None)
def _pf_inputs(dtype, n_phases, n):
    """(P, S), each [n_phases, n]: seeded magnitudes over 1e-30 ... 1e30 with the 14 x 14 grid of special (P, S) pairs at the head, across the body / tail seam up to
    the last element and across the first tile edge, and the phase inputs (linspace(-1, 1), the neighbours of +-1, +-0, subnormals, clamped cases) behind the head"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1000 * n_phases + n % 997 + dtype.itemsize)
    P, S = EO.wide_random(rng, (n_phases, n), dtype, signed=True), EO.wide_random(rng, (n_phases, n), dtype)
    g = EO.grid(dtype, 2)
    p, s = EO.phase_inputs(dtype)
    for r in range(n_phases):
        o = rng.permutation(g.shape[1])
        for at in (tile() - 98, 200 + 40 * r, n - g.shape[1], 0):  # (the later splices win where they overlap: the head and the end are always whole)
            if at == 200 + 40 * r:
                k = max(min(p.size, n - at), 0)
                P[r, at:at + k], S[r, at:at + k] = p[:k], s[:k]
            else:
                _splice(P[r:r + 1], g[0:1, o], at)
                _splice(S[r:r + 1], g[1:2, o], at)
    for a in (P, S):
        a.setflags(write=False)
    return P, S


@functools.lru_cache(maxsize=None)
def _ub_inputs(dtype, n_phases, n):
    """(U, I, P), each [n_phases, n]: the same plan with columns of the 14^n_phases grid (every phase +inf and every phase NaN among them)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(2000 * n_phases + n % 997 + dtype.itemsize)
    out = []
    for signed in (False, False, True):
        x = EO.wide_random(rng, (n_phases, n), dtype, signed=signed)
        near = (230.0 * rng.uniform(0.95, 1.05, (n_phases, n))).astype(dtype)  # realistic phases on every other sample: unbalances of a few percent
        x[:, 1::2] = near[:, 1::2]
        cols = _special_columns(dtype, n_phases, 14 ** n_phases if n_phases <= 3 else 400, rng)
        cols = cols[:, rng.permutation(cols.shape[1])]
        for k, at in enumerate((tile() - 98, n - 196)):  # across the first tile edge, and across the body / tail seam up to the last element
            _splice(x, cols[:, 196 * (k + 1):196 * (k + 2)], at)
        cols[:, :2] = np.array([np.inf, np.nan], dtype)[None, :]  # every phase +inf, every phase NaN
        _splice(x, cols[:, :min(cols.shape[1], max(n - 400, min(n, 196)))], 0)  # the head last: it is always whole (the whole grid where n leaves room for it)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


def _check_phase(got, want, what):
    t = TNAME[want.dtype]
    d = float(EO.ulp_distance(got, want).max()) if want.size else 0.0
    print(f"{what}: phase {d} ulp from the oracle (bound {PHASE_BOUND_ULP[t]})")
    assert d <= PHASE_BOUND_ULP[t], (what, d)
    return d


def _check_exact(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    u = f"u{want.itemsize}"
    assert EO.same_bits(got, want), (what, np.nonzero((got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want)))[-1][:8])


@pytest.mark.parametrize("n_phases", [1, 3, 5])
@pytest.mark.parametrize("dtype", EO.FLOATS)
def test_power_factor_parity(dtype, n_phases):
    import gnuradio4_amd as G
    blk = G.PowerFactor(n_phases, TORCH[np.dtype(dtype)])
    worst = 0.0
    for n in _sizes():
        P, S = _pf_inputs(dtype, n_phases, n)
        pf, ph = blk.process(_dev(P), _dev(S))
        torch.cuda.synchronize()
        assert pf.shape == ph.shape == (n_phases, n)
        want_pf, want_ph = EO.power_factor(P, S)
        _check_exact(pf.cpu().numpy(), want_pf, f"power_factor<{TNAME[np.dtype(dtype)]}, {n_phases}> n={n}")
        worst = max(worst, _check_phase(ph.cpu().numpy(), want_ph, f"PowerFactor<{TNAME[np.dtype(dtype)]}, {n_phases}> n={n}"))
    if n_phases == 1:  # a 1-D tensor is one phase
        P, S = _pf_inputs(dtype, 1, tile() + 3)
        pf1, _ = blk.process(_dev(P[0]), _dev(S[0]))
        _check_exact(pf1.cpu().numpy(), EO.power_factor(P, S)[0], "1-D")
    print(f"PowerFactor<{TNAME[np.dtype(dtype)]}, {n_phases}>: largest phase distance {worst} ulp")


@pytest.mark.parametrize("n_phases", [2, 3, 5])
@pytest.mark.parametrize("dtype", EO.FLOATS)
def test_system_unbalance_parity(dtype, n_phases):
    """2 and 3 phases are compile-time kernels, 5 the run-time loop; every-phase-+inf (voltage 0, current NaN) is among the inputs of every size but 0"""
    import gnuradio4_amd as G
    blk = G.SystemUnbalance(n_phases, TORCH[np.dtype(dtype)])
    for n in _sizes():
        U, I, P = _ub_inputs(dtype, n_phases, n)
        outs = blk.process(_dev(U), _dev(I), _dev(P))
        torch.cuda.synchronize()
        want = EO.system_unbalance(U, I, P)
        for name, o, w in zip(("P_total", "U_unbalance", "I_unbalance"), outs, want):
            assert o.shape == (n,)
            _check_exact(o.cpu().numpy(), w, f"{name}<{TNAME[np.dtype(dtype)]}, {n_phases}> n={n}")
        if n:
            k = int(np.nonzero(np.all(np.isposinf(U), axis=0) & np.all(np.isposinf(I), axis=0))[0][0])
            assert want[1][k] == 0 and np.isnan(want[2][k])


# ---- alignment: every pointer 0 / 1 / 3 elements off a 16-byte boundary, rows n, n + 1 and n + 3 apart (rows disagree), sentinels around every row
OFFSETS = (0, 1, 3)
N_ALIGN = 517  # a head, a body of more than one wave and a tail whatever the offsets
SENTINEL = 12345.678


class _Rows:
    """n_rows rows of n elements `stride` apart, `off` elements behind a 16-byte boundary, inside a buffer of sentinels"""

    def __init__(self, dtype, n_rows, n, stride, off, data=None):
        self.n_rows, self.n, self.stride, self.off = n_rows, n, stride, off
        self.buf = torch.full((off + n_rows * stride + 8,), SENTINEL, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        if data is not None:
            self.rows()[:] = data
        self.ptr = self.buf.data_ptr() + off * self.buf.element_size()

    def rows(self, buf=None):
        buf = self.buf if buf is None else buf
        return buf[self.off:self.off + self.n_rows * self.stride].view(self.n_rows, self.stride)[:, :self.n]

    def holds(self, want):
        """the rows equal `want` bit for bit and every other element is still the sentinel"""
        exp = torch.full_like(self.buf, SENTINEL)
        self.rows(exp)[:] = want
        return _same_bits_dev(self.buf, exp)


@pytest.mark.parametrize("dtype", EO.FLOATS)
def test_power_factor_alignment_strides_and_sentinels(dtype):
    from gnuradio4_amd import capi
    L = capi.lib()
    td, did, n, R = TORCH[np.dtype(dtype)], (capi.F32 if dtype == np.float32 else capi.F64), N_ALIGN, 3
    P, S = _pf_inputs(dtype, R, n)
    want_pf, want_ph = EO.power_factor(P, S)
    dP, dS, w_pf = _dev(P), _dev(S), _dev(want_pf)
    worst, cases = 0.0, 0
    for stride in (n, n + 1, n + 3):
        for oP, oS, of, oa in itertools.product(OFFSETS, repeat=4):
            rP, rS = _Rows(td, R, n, stride, oP, dP), _Rows(td, R, n, stride, oS, dS)
            rf, ra = _Rows(td, R, n, stride, of), _Rows(td, R, n, stride, oa)
            st = torch.cuda.current_stream().cuda_stream
            assert L.gr4hip_powerfactor_process(did, R, rP.ptr, rS.ptr, stride, rf.ptr, ra.ptr, stride, n, st) == capi.OK
            assert rf.holds(w_pf), (stride, oP, oS, of, oa)
            got = ra.rows().clone()
            ra.rows()[:] = 0
            assert ra.holds(torch.zeros_like(got)), (stride, oP, oS, of, oa)  # nothing outside the phase rows was written
            assert rP.holds(dP) and rS.holds(dS)
            if (oP, oS, of) == (0, 1, 3) or cases % 27 == 0:  # the phase values of a sample of the cases on the host (the rest were written by the same code)
                worst = max(worst, float(EO.ulp_distance(got.cpu().numpy(), want_ph).max()))
            cases += 1
    assert cases == 3 * 81 and worst <= PHASE_BOUND_ULP[TNAME[np.dtype(dtype)]], worst
    # different strides on the two sides, and a call per offset of a single phase
    rP, rS, rf, ra = _Rows(td, R, n, n + 3, 1, dP), _Rows(td, R, n, n + 3, 1, dS), _Rows(td, R, n, n + 1, 3), _Rows(td, R, n, n + 1, 0)
    assert L.gr4hip_powerfactor_process(did, R, rP.ptr, rS.ptr, n + 3, rf.ptr, ra.ptr, n + 1, n, None) == capi.OK
    torch.cuda.synchronize()
    assert rf.holds(w_pf)


@pytest.mark.parametrize("n_phases", [3, 5])
@pytest.mark.parametrize("dtype", EO.FLOATS)
def test_system_unbalance_alignment_strides_and_sentinels(dtype, n_phases):
    """three phases: all 3^6 offset combinations of the six pointers; five phases (the run-time loop): the inputs together against every output combination"""
    from gnuradio4_amd import capi
    L = capi.lib()
    td, did, n, R = TORCH[np.dtype(dtype)], (capi.F32 if dtype == np.float32 else capi.F64), N_ALIGN, n_phases
    U, I, P = _ub_inputs(dtype, R, n)
    want = [_dev(w)[None] for w in EO.system_unbalance(U, I, P)]
    dU, dI, dP = _dev(U), _dev(I), _dev(P)
    combos = list(itertools.product(OFFSETS, repeat=6)) if R == 3 else [(a, b, c, d, e, f) for a, b, c in ((0, 0, 0), (1, 1, 1), (3, 3, 3), (0, 1, 3)) for d, e, f in itertools.product(OFFSETS, repeat=3)]
    st = torch.cuda.current_stream().cuda_stream
    for stride in (n, n + 1, n + 3):
        ins = {(k, o): _Rows(td, R, n, stride, o, d) for k, d in enumerate((dU, dI, dP)) for o in OFFSETS}  # inputs are only read: one buffer per offset
        for oU, oI, oP, ot, ou, oi in combos:
            outs = [_Rows(td, 1, n, n, o) for o in (ot, ou, oi)]
            assert L.gr4hip_unbalance_process(did, R, ins[0, oU].ptr, ins[1, oI].ptr, ins[2, oP].ptr, stride, outs[0].ptr, outs[1].ptr, outs[2].ptr, n, st) == capi.OK
            for o, w in zip(outs, want):
                assert o.holds(w), (stride, oU, oI, oP, ot, ou, oi)
        for (k, o), r in ins.items():
            assert r.holds((dU, dI, dP)[k])


@pytest.mark.parametrize("dtype", EO.FLOATS)
def test_null_outputs(dtype):
    """each output alone and all but one: an unconnected port is a NULL pointer, and the others are unchanged bit for bit"""
    import gnuradio4_amd as G
    td, n = TORCH[np.dtype(dtype)], tile() + 3
    P, S = _pf_inputs(dtype, 3, n)
    pf = G.PowerFactor(3, td)
    names = ("power_factor", "phase")
    full = pf.process(_dev(P), _dev(S))
    for keep in (("power_factor",), ("phase",)):
        part = pf.process(_dev(P), _dev(S), outputs=keep)
        for k, a, b in zip(names, part, full):
            assert (a is None) == (k not in keep) and (a is None or _same_bits_dev(a, b)), (keep, k)
    assert pf.process(_dev(P), _dev(S), outputs=()) == (None, None)
    for R in (3, 5):
        U, I, Pw = _ub_inputs(dtype, R, n)
        ub = G.SystemUnbalance(R, td)
        names = ("P_total", "U_unbalance", "I_unbalance")
        full = ub.process(_dev(U), _dev(I), _dev(Pw))
        for keep in [(k,) for k in names] + [tuple(k for k in names if k != drop) for drop in names] + [()]:
            part = ub.process(_dev(U), _dev(I), _dev(Pw), outputs=keep)
            for k, a, b in zip(names, part, full):
                assert (a is None) == (k not in keep) and (a is None or _same_bits_dev(a, b)), (R, keep, k)
    torch.cuda.synchronize()


def _chain(pm, pf, ub, u, i, cuts=()):
    """PowerMetrics -> PowerFactor + SystemUnbalance on device tensors only; the stream cut into calls at `cuts` (input samples).  Returns the metrics' rows and the
    five results, concatenated over the calls"""
    edges = [0, *cuts, u.shape[1]]
    rows, res = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        P, Q, S, U, I = pm.process_bulk(u[:, a:b], i[:, a:b])
        rows.append((P, S, U, I))
        res.append((*pf.process(P, S), *ub.process(U, I, P)))
    return [torch.cat([r[k] for r in rows], dim=1) for k in range(4)], [torch.cat([r[k] for r in res], dim=-1) for k in range(5)]


def _check_chain(rows, res, what):
    P, S, U, I = (r.cpu().numpy() for r in rows)
    want = (*EO.power_factor(P, S), *EO.system_unbalance(U, I, P))
    for k, (name, got, w) in enumerate(zip(("power_factor", "phase", "P_total", "U_unbalance", "I_unbalance"), res, want)):
        if name == "phase":
            _check_phase(got.cpu().numpy(), w, what)
        else:
            _check_exact(got.cpu().numpy(), w, f"{what} {name}")


def test_chaining_behind_power_metrics():
    """G.PowerMetrics (three phases, decimate 7) feeds both blocks with its output tensors, no host copy: the results are the oracle's on the downloaded metrics"""
    import gnuradio4_amd as G
    D, n_out = 7, tile() + 3
    u, i = PM.qa_signals(D * n_out, 10000.0, 3, 42)
    du, di = _dev(u), _dev(i)
    pf, ub = G.PowerFactor(3), G.SystemUnbalance(3)
    rows, res = _chain(G.PowerMetrics(n_phases=3, decimate=D), pf, ub, du, di)
    torch.cuda.synchronize()
    assert rows[0].shape == (3, n_out) and res[0].shape == (3, n_out) and res[2].shape == (n_out,)
    _check_chain(rows, res, "one call")
    print(f"power factor {float(res[0][:, -1].mean())}, voltage unbalance {float(res[3][-1])} %, current unbalance {float(res[4][-1])} %")
    # column ranges of the metrics' rows (strided views: rows n_out apart, read in place) give the same bits as the whole rows
    cuts = [0, 5, tile() // 2 + 1, n_out]
    parts = [(*pf.process(rows[0][:, a:b], rows[1][:, a:b]), *ub.process(rows[2][:, a:b], rows[3][:, a:b], rows[0][:, a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    assert rows[0][:, 5:9].stride(0) == n_out
    for k in range(5):
        assert _same_bits_dev(torch.cat([p[k] for p in parts], dim=-1), res[k]), k
    # the same stream in three calls: again the oracle's values on the metrics of that run, and the same bits when it is run again
    three = [_chain(G.PowerMetrics(n_phases=3, decimate=D), pf, ub, du, di, cuts=(D * 5, D * (tile() // 2 + 1))) for _ in range(2)]
    torch.cuda.synchronize()
    _check_chain(*three[0], "three calls")
    for a, b in zip(three[0][0] + three[0][1], three[1][0] + three[1][1]):
        assert _same_bits_dev(a, b)


def test_two_streams_at_once():
    import gnuradio4_amd as G
    n = 2 * tile() + 1
    P, S = _pf_inputs(np.float32, 3, n)
    U, I, Pw = _ub_inputs(np.float64, 3, n)
    pf, ub = G.PowerFactor(3), G.SystemUnbalance(3, torch.float64)
    args_pf, args_ub = (_dev(P), _dev(S)), (_dev(U), _dev(I), _dev(Pw))
    one = (*pf.process(*args_pf), *ub.process(*args_ub))
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    both = []
    for _ in range(4):
        with torch.cuda.stream(sa):
            a = pf.process(*args_pf)
        with torch.cuda.stream(sb):
            b = ub.process(*args_ub)
        both.append((*a, *b))
    sa.synchronize()
    sb.synchronize()
    for r in both:
        for x, y in zip(r, one):
            assert _same_bits_dev(x, y)


def test_bad_calls_are_refused_with_nothing_written():
    import gnuradio4_amd as G
    from gnuradio4_amd import capi
    L = capi.lib()
    n = 300
    x = torch.ones(3, n, device="cuda")
    out = [torch.full((3, n), SENTINEL, device="cuda") for _ in range(3)]
    keep = [o.clone() for o in out]
    p = [t.data_ptr() for t in out]
    INV = capi.INVALID_ARGUMENT
    assert L.gr4hip_powerfactor_process(capi.C32, 3, x.data_ptr(), x.data_ptr(), n, p[0], p[1], n, n, None) == INV
    assert L.gr4hip_powerfactor_process(capi.F32, 17, x.data_ptr(), x.data_ptr(), n, p[0], p[1], n, n, None) == INV
    assert L.gr4hip_powerfactor_process(capi.F32, 3, x.data_ptr(), None, n, p[0], p[1], n, n, None) == INV
    assert L.gr4hip_powerfactor_process(capi.F32, 3, x.data_ptr(), x.data_ptr(), n - 1, p[0], p[1], n, n, None) == INV
    assert L.gr4hip_powerfactor_process(capi.F32, 3, x.data_ptr(), x.data_ptr(), n, p[0], p[1], n - 1, n, None) == INV
    assert L.gr4hip_powerfactor_process(capi.F32, 3, p[0] + 4 * (3 * n - 1), x.data_ptr(), n, p[0], p[1], n, n, None) == INV  # P's first element is the output's last
    assert L.gr4hip_powerfactor_process(capi.F32, 3, x.data_ptr(), x.data_ptr(), n, p[0] + 2, p[1], n, n, None) == INV
    assert L.gr4hip_unbalance_process(capi.I32, 3, x.data_ptr(), x.data_ptr(), x.data_ptr(), n, p[0], p[1], p[2], n, None) == INV
    assert L.gr4hip_unbalance_process(capi.F32, 1, x.data_ptr(), x.data_ptr(), x.data_ptr(), n, p[0], p[1], p[2], n, None) == INV
    assert L.gr4hip_unbalance_process(capi.F32, 3, x.data_ptr(), x.data_ptr(), None, n, p[0], p[1], p[2], n, None) == INV
    assert L.gr4hip_unbalance_process(capi.F32, 3, x.data_ptr(), x.data_ptr(), x.data_ptr(), n - 1, p[0], p[1], p[2], n, None) == INV
    assert L.gr4hip_unbalance_process(capi.F32, 3, x.data_ptr(), x.data_ptr(), x.data_ptr(), n, p[0], x.data_ptr() + 4 * (3 * n - 1), p[2], n, None) == INV
    with pytest.raises(capi.Gr4HipError):
        G.PowerFactor(3).process(x, x.double())
    with pytest.raises(capi.Gr4HipError):
        G.PowerFactor(3).process(x, x[:2])
    with pytest.raises(capi.Gr4HipError):
        G.SystemUnbalance(3).process(x, x, x.cpu())
    with pytest.raises(capi.Gr4HipError):
        G.SystemUnbalance(2).process(x, x, x)
    torch.cuda.synchronize()
    for o, k in zip(out, keep):
        assert _same_bits_dev(o, k)
    assert L.gr4hip_powerfactor_process(capi.F32, 3, x.data_ptr(), x.data_ptr(), n, p[0], p[1], n, n, None) == capi.OK  # the library goes on working
    torch.cuda.synchronize()
    assert bool(torch.all(out[0] == 1)) and bool(torch.all(out[1] == 0))


def test_host_graphs_on_the_device(tmp_path):
    """gnuradio4_amd/host/tests/test_host_electrical.cpp as a fresh child process on gpu:hip:0: the four graphs per type against the oracle, then PowerMetrics<float, 3>
    -> ThreePhasePowerFactorCalculator + ThreePhaseSystemUnbalanceCalculator built in C++ and the same graph from a GRC text through the plugin, both against the
    Python chain on the same input"""
    import gnuradio4_amd as G
    from test_electrical_host import check_graph_files, write_graph_files
    root = O.ROOT
    subprocess.check_call(["bash", os.path.join(root, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    prog = os.path.join(root, "build", "host", "test_host_electrical")
    plugin = os.path.join(root, "gnuradio4_amd", "libgr4hip_blocks.so")
    want = write_graph_files(tmp_path)
    D, n_out = 7, tile() + 3
    u, i = PM.qa_signals(D * n_out, 10000.0, 3, 42)
    u.tofile(tmp_path / "u.f32")
    i.tofile(tmp_path / "i.f32")
    r = subprocess.run([prog, plugin, "gpu:hip:0", str(tmp_path), repr(PHASE_BOUND_ULP["f32"]), repr(PHASE_BOUND_ULP["f64"])], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "all checks passed (compute_domain gpu:hip:0)" in r.stdout, r.stdout + r.stderr
    check_graph_files(tmp_path, want, PHASE_BOUND_ULP)
    _, res = _chain(G.PowerMetrics(n_phases=3, decimate=D), G.PowerFactor(3), G.SystemUnbalance(3), _dev(u), _dev(i))
    torch.cuda.synchronize()
    pf, ph, pt, uu, iu = (x.cpu().numpy() for x in res)
    for tag in ("chain", "grc"):
        def sink(name):
            return np.fromfile(tmp_path / f"{tag}_{name}.bin", np.float32)
        for k in range(3):
            _check_exact(sink(f"power_factor{k}"), pf[k], f"{tag} power_factor {k}")
            _check_exact(sink(f"phase{k}"), ph[k], f"{tag} phase {k}")
        _check_exact(sink("P_total"), pt, f"{tag} P_total")
        _check_exact(sink("U_unbalance"), uu, f"{tag} U_unbalance")
        _check_exact(sink("I_unbalance"), iu, f"{tag} I_unbalance")
