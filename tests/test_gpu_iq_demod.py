"""IQDemodulator on the device (csrc/iq_demod.hip) against the float64 restatement in tests/iq_demod_oracle.py.

Parity is asserted where the oracle's decisions have margin (MARGIN relative to eps; every asin argument of the frequency iteration away from +-1): 1e-6 relative for amplitude and frequency
and 1e-6 rad absolute for phase with float, 1e-9 with double.  Outputs the reference gives as 0 must be exactly 0."""
import numpy as np
import pytest
import torch

import iq_demod_oracle as IQ

pytestmark = pytest.mark.gpu

S = 8192  # samples per workgroup segment (csrc/iq_demod.hip)
N = 1 << 20


def _blk(p: IQ.Params):
    import gnuradio4_amd as G
    return G.IQDemodulator(dtype=torch.float32 if p.dtype == np.float32 else torch.float64, chunk=p.chunk, **p.kw())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(blk, ref, resp, cuts=()):
    """one stream through blk, cut into calls at the given sample indices (multiples of the chunk)"""
    r, x = _dev(ref), _dev(resp)
    edges = [0, *cuts, len(ref)]
    outs = [blk.process_bulk(r[a:b], x[a:b]) for a, b in zip(edges[:-1], edges[1:]) if b > a]
    torch.cuda.synchronize()
    return tuple(torch.cat([o[i] for o in outs]).cpu().numpy().astype(np.float64) for i in range(3))


def _parity(p, got, want, min_decided=0.9):
    amp, ph, fr, m = want
    ok = m["decided"]
    assert ok.mean() >= min_decided, ok.mean()
    tol = 1e-6 if p.dtype == np.float32 else 1e-9
    pht = tol * (180.0 / np.pi if p.phase_unit == 1 else 1.0)
    for g, w, name in ((got[0], amp, "amplitude"), (got[2], fr, "frequency")):
        assert g.shape == w.shape
        zero = ok & (w == 0)
        assert np.all(g[zero] == 0), name
        e = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
        e = np.where(ok & (w != 0), e, 0.0)
        assert e.max() <= tol, (name, float(e.max()), int(e.argmax()))
    e = np.where(ok, np.abs(got[1] - ph), 0.0)
    assert e.max() <= pht, ("phase", float(e.max()), int(e.argmax()))
    assert np.all(got[1][ok & (ph == 0)] == 0)


def _signals(n, freq=5e6, fs=62.5e6, dtype=np.float32, seed=42):
    return IQ.qa_signals(freq, fs, 0.8, 0.5, 0.1, 0.01, n, dtype, seed)


@pytest.mark.parametrize("C", [1, 7, 256, 1024, S - 1, S + 1, 3 * S + 5])
def test_parity_over_chunks(C):
    p = IQ.Params(chunk=C)
    n = (N // C) * C
    ref, resp = _signals(n)
    _parity(p, _run(_blk(p), ref, resp), IQ.truth(p, ref, resp))


@pytest.mark.parametrize("method", range(3))
@pytest.mark.parametrize("unit,invert", [(0, False), (1, False), (0, True), (1, True)])
def test_methods_degrees_invert(method, unit, invert):
    p = IQ.Params(sample_rate=1e6, f_high_pass=50.0, f_low_pass=20000.0, derivative_method=method, phase_unit=unit, invert_phase=invert, chunk=256)
    ref, resp = _signals(1 << 18, 50e3, 1e6)
    _parity(p, _run(_blk(p), ref, resp), IQ.truth(p, ref, resp))


@pytest.mark.parametrize("method", range(3))
def test_double(method):
    p = IQ.Params(np.float64, derivative_method=method, phase_unit=1, chunk=1024)
    ref, resp = _signals(N, dtype=np.float64)
    _parity(p, _run(_blk(p), ref, resp), IQ.truth(p, ref, resp))


def test_long_run_carries_cross_thousands_of_segments():
    """2^24 samples at the defaults (62.5 MHz, f_hp 100 Hz: a high-pass time constant of ~1e5 samples), 2048 segments"""
    p = IQ.Params(chunk=1024)
    ref, resp = _signals(1 << 24, 1.1e6)
    _parity(p, _run(_blk(p), ref, resp), IQ.truth(p, ref, resp))


@pytest.mark.parametrize("C,cuts", [(1, [S - 1, S + 2, 2 * S - 3, 2 * S + 1, 5 * S + 4]),
                                    (7, [7 * 1170, 7 * 1171, 7 * 2341, 7 * 2342]),
                                    (1024, [1024, 2048, 3072, 4096, 8 * 1024, 9 * 1024])])
def test_split_calls_meet_the_same_bound(C, cuts):
    p = IQ.Params(chunk=C)
    n = (N // 4 // C) * C
    ref, resp = _signals(n)
    want = IQ.truth(p, ref, resp)
    _parity(p, _run(_blk(p), ref, resp, cuts), want)


def test_same_calls_twice_are_bitwise_equal():
    p = IQ.Params(chunk=7, derivative_method=2)
    n = (N // 7) * 7
    ref, resp = _signals(n)
    cuts = [7 * 1000, 7 * 5000]
    a, b = _run(_blk(p), ref, resp, cuts), _run(_blk(p), ref, resp, cuts)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_reset_equals_a_fresh_handle():
    p = IQ.Params(chunk=256, derivative_method=1)
    ref, resp = _signals(1 << 18)
    blk = _blk(p)
    _run(blk, ref, resp)
    blk.reset()
    a = _run(blk, ref[:1 << 16], resp[:1 << 16])
    b = _run(_blk(p), ref[:1 << 16], resp[:1 << 16])
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_set_params_with_and_without_reinitialisation():
    p = IQ.Params(chunk=512)
    n = 1 << 18
    ref, resp = _signals(2 * n)
    # without: the filters carry on, the new phase settings apply to the next outputs
    blk = _blk(p)
    first = _run(blk, ref[:n], resp[:n])
    blk.set_params(phase_unit=1, invert_phase=True)
    second = _run(blk, ref[n:], resp[n:])
    states = IQ.lp_states(p, ref, resp)
    k = n // 512
    _parity(p, first, IQ.extract(p, states[:, :k]))
    p2 = p.replace(phase_unit=1, invert_phase=True)
    _parity(p2, second, IQ.extract(p2, states[:, k:]))
    # with: a filter key re-initialises, as a fresh handle with the new settings
    blk = _blk(p)
    _run(blk, ref[:n], resp[:n])
    blk.set_params(f_low_pass=5000.0)
    p3 = p.replace(f_low_pass=5000.0)
    got = _run(blk, ref[n:], resp[n:])
    fresh = _run(_blk(p3), ref[n:], resp[n:])
    assert all(np.array_equal(u, v) for u, v in zip(got, fresh))
    _parity(p3, got, IQ.truth(p3, ref[n:], resp[n:]))


@pytest.mark.parametrize("which,pos,val", [(0, 300_001, np.nan), (1, 123_457, np.inf), (0, 3 * S, -np.inf)])
def test_non_finite_input_poisons_until_reset(which, pos, val):
    p = IQ.Params(chunk=256)
    n = 1 << 19
    ref, resp = _signals(n)
    (ref if which == 0 else resp)[pos] = val
    want = IQ.truth(p, ref, resp)
    blk = _blk(p)
    got = _run(blk, ref, resp, [n // 2])
    _parity(p, got, want, 0.5)  # (a NaN state decides every threshold exactly)
    after = slice(pos // 256 + 1, None)
    assert np.all(want[0][after] == 0) and np.all(want[1][after] == 0)  # Px or Pr and I, Q are NaN from there on
    assert which == 1 or np.all(want[2][after] == 0)  # the frequency needs only the reference
    more = _run(blk, ref[:1 << 16], resp[:1 << 16])  # the state stays poisoned
    assert np.all(more[0] == 0) and np.all(more[1] == 0) and (which == 1 or np.all(more[2] == 0))
    blk.reset()
    clean = IQ.qa_signals(5e6, 62.5e6, 0.8, 0.5, 0.1, 0.01, 1 << 16, np.float32, 3)
    _parity(p, _run(blk, *clean), IQ.truth(p, *clean))


def test_zero_input_gives_exact_zero():
    for method in range(3):
        p = IQ.Params(chunk=7, derivative_method=method)
        z = np.zeros(7 * 20000, np.float32)
        assert all(np.all(v == 0) for v in _run(_blk(p), z, z))


def test_two_handles_on_two_streams():
    import gnuradio4_amd as G
    pa, pb = IQ.Params(chunk=1024), IQ.Params(chunk=7, derivative_method=2)
    na, nb = N, (N // 7) * 7
    ra, xa = _signals(na)
    rb, xb = _signals(nb, 2e6, seed=5)
    want_a, want_b = _run(_blk(pa), ra, xa, [na // 2]), _run(_blk(pb), rb, xb, [7 * 50000])
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ba, bb = _blk(pa), _blk(pb)
    dra, dxa, drb, dxb = _dev(ra), _dev(xa), _dev(rb), _dev(xb)
    torch.cuda.synchronize()
    oa, ob = [], []
    with torch.cuda.stream(sa):
        oa.append(ba.process_bulk(dra[:na // 2], dxa[:na // 2]))
    with torch.cuda.stream(sb):
        ob.append(bb.process_bulk(drb[:7 * 50000], dxb[:7 * 50000]))
    with torch.cuda.stream(sa):
        oa.append(ba.process_bulk(dra[na // 2:], dxa[na // 2:]))
    with torch.cuda.stream(sb):
        ob.append(bb.process_bulk(drb[7 * 50000:], dxb[7 * 50000:]))
    torch.cuda.synchronize()
    for outs, want in ((oa, want_a), (ob, want_b)):
        got = tuple(torch.cat([o[i] for o in outs]).cpu().numpy().astype(np.float64) for i in range(3))
        assert all(np.array_equal(u, v) for u, v in zip(got, want))
    assert isinstance(ba, G.IQDemodulator)


def test_reset_queued_between_calls_without_a_host_sync():
    p = IQ.Params(chunk=256)
    ref, resp = _signals(1 << 18)
    fresh = _run(_blk(p), ref[:1 << 16], resp[:1 << 16])
    st = torch.cuda.Stream()
    blk = _blk(p)
    r, x = _dev(ref), _dev(resp)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        blk.process_bulk(r, x)
        blk.reset()
        out = blk.process_bulk(r[:1 << 16], x[:1 << 16])
    st.synchronize()
    got = tuple(o.cpu().numpy().astype(np.float64) for o in out)
    assert all(np.array_equal(u, v) for u, v in zip(got, fresh))


def test_bad_calls_are_refused_before_device_work():
    from gnuradio4_amd import capi
    p = IQ.Params(chunk=1024)
    blk = _blk(p)
    ref, resp = _signals(1000)
    with pytest.raises(capi.Gr4HipError):
        blk.process_bulk(_dev(ref), _dev(resp))  # n_in % chunk != 0
    with pytest.raises(capi.Gr4HipError):
        blk.set_params(f_low_pass=4e7)  # f_lp >= fs / 2
