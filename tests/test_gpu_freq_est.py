"""FrequencyEstimatorTimeDomain / FrequencyEstimatorFrequencyDomain on the device (csrc/freq_est.hip) against the restatement in tests/freq_est_oracle.py.

Parity inputs have unambiguous decisions: each case asserts in the float64 oracle that the top two magnitudes of the search range differ by more than 1e-4
relative and that every threshold (|delta| vs 1, the denominator vs eps, z vs +-1, B vs eps, |4 y| vs eps) has margin.  The fallback paths get inputs of
their own where the decision is exact."""
import numpy as np
import pytest
import torch

import freq_est_oracle as FE

pytestmark = pytest.mark.gpu

TD, FD = 0, 1
N_LONG = 1 << 20


def _block(p: FE.Params, chunk=None):
    import gnuradio4_amd as G
    cls = G.FrequencyEstimatorTimeDomain if p.method == TD else G.FrequencyEstimatorFrequencyDomain
    return cls(chunk=p.chunk if chunk is None else chunk, **p.kw())


def _run(blk, x, cuts=()):
    """one stream through blk, cut into calls at the given sample indices (multiples of the chunk)"""
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    edges = [0, *cuts, len(x)]
    outs = [blk.process_bulk(xd[a:b]) for a, b in zip(edges[:-1], edges[1:]) if b > a]
    torch.cuda.synchronize()
    return torch.cat(outs).cpu().numpy().astype(np.float64) if outs else np.zeros(0)


def _truth(p, x, prev=None):
    return (FE.td_truth if p.method == TD else FE.fd_truth)(p, x, prev)


def _margins_ok(p, m):
    if p.method == TD:
        assert m["b_over_eps"] > 10 and m["z_to_edge"] > 1e-4 and m["y_over_eps"] > 1e-3, m
    else:
        assert m["top2"] > 1e-4 and m["delta_to_1"] > 1e-4 and m["den_over_eps"] > 1e-3, m


def _parity(p, got, x, prev=None):
    out, raw, valid, m = _truth(p, x, prev)
    _margins_ok(p, m)
    assert valid.any()
    err = FE.rel_err(got, out)
    assert got.shape == out.shape
    assert float(np.max(err)) <= 1e-5, (float(np.max(err)), int(np.argmax(err)))
    return out, valid


def _signal(n, f=50.3, fs=1000.0, seed=7, noise=0.01):
    return FE.tone(f, fs, n, noise=noise, seed=seed)


def _chunks(method):
    W = FE.geometry(FE.Params(method))[0]
    return [1, 7, 10, W, W + 3]


@pytest.mark.parametrize("method", [TD, FD])
@pytest.mark.parametrize("ci", range(5))
def test_parity_over_many_tiles(method, ci):
    C = _chunks(method)[ci]
    p = FE.Params(method, chunk=C)
    n = (N_LONG // C) * C
    x = _signal(n)
    got = _run(_block(p), x)
    _parity(p, got, x)


def test_parity_at_the_reference_qa_size():
    """the frequency-domain form per sample at N = 4096 (qa_FrequencyEstimator.cpp:136-166), many tiles"""
    p = FE.Params(FD, f_min=45.0, f_max=55.0, min_fft_size=4096, chunk=1)
    x = _signal(1 << 18, f=50.37)
    _parity(p, _run(_block(p), x), x)


@pytest.mark.parametrize("method", [TD, FD])
@pytest.mark.parametrize("C", [1, 10])
def test_split_calls_equal_one_call(method, C):
    p = FE.Params(method, chunk=C)
    W = FE.geometry(p)[0]
    n = 200000 // C * C
    x = _signal(n, seed=3)
    whole = _run(_block(p), x)
    r = lambda v: max(C, v // C * C)  # noqa: E731
    cuts = sorted({r(1), r(1) + r(W - 1), r(1) + r(W - 1) + r(W), 4 * r(1025) + C, 65536 // C * C + C, 100000 // C * C})
    split = _run(_block(p), x, cuts)
    assert np.max(FE.rel_err(split, whole)) <= 1e-6
    _parity(p, split, x)


@pytest.mark.parametrize("method", [TD, FD])
def test_settling_outputs_are_the_initial_estimate(method):
    p = FE.Params(method, f_expected=47.25, chunk=1)
    W = FE.geometry(p)[0]
    got = _run(_block(p), _signal(4 * W))
    assert np.all(got[:W - 1] == np.float32(47.25))
    assert np.all(np.abs(got[W:] - 50.3) < 1.0)


@pytest.mark.parametrize("method", [TD, FD])
def test_reset_and_set_params_mid_stream(method):
    p = FE.Params(method, f_expected=47.25, chunk=1)
    W = FE.geometry(p)[0]
    x = _signal(8 * W)
    blk = _block(p)
    a = _run(blk, x[:4 * W])
    last = a[-1]
    assert abs(last - 50.3) < 1.0 and last != np.float32(47.25)
    blk.set_params(f_max=p.f_max)  # settingsChanged: histories emptied, the last estimate kept
    b = _run(blk, x[4 * W:])
    assert np.all(b[:W - 1] == np.float32(last))
    _parity(p, b, x[4 * W:], prev=last)
    blk.reset()  # reset(): the last estimate is f_expected
    c = _run(blk, x[4 * W:])
    assert np.all(c[:W - 1] == np.float32(47.25))
    _parity(p, c, x[4 * W:])
    # a settings change that changes the geometry and the biquad takes effect on the next call
    q = FE.Params(method, f_min=35.0, f_expected=47.25, f_max=58.0, n_periods=3, min_fft_size=512, chunk=1)
    blk.set_params(**q.kw())
    d = _run(blk, x)
    Wq = FE.geometry(q)[0]
    assert Wq != W and np.all(d[:Wq - 1] == c[-1])
    _parity(q, d, x, prev=c[-1])


@pytest.mark.parametrize("method", [TD, FD])
def test_all_zero_input_keeps_the_previous_estimate(method):
    p = FE.Params(method, f_expected=51.5, chunk=1)
    got = _run(_block(p), np.zeros(1 << 16, np.float32), cuts=[1000, 30000])
    assert np.all(got == np.float32(51.5))


def test_frequency_domain_non_finite_window_repeats_the_previous_output():
    p = FE.Params(FD, chunk=1)
    N = FE.geometry(p)[0]
    x = _signal(1 << 16, seed=5)
    q0, q1 = 5000, 30000
    x[q0] = np.nan
    x[q1] = np.inf
    got = _run(_block(p), x, cuts=[q0 + 17, q1 + N - 1])
    _parity(p, got, x)
    for q in (q0, q1):
        assert np.all(got[q:q + N] == got[q - 1])  # exactly the N outputs whose window holds it
        assert got[q + N] != got[q - 1]
    assert np.all(np.isfinite(got))


def test_time_domain_nan_poisons_until_reset():
    p = FE.Params(TD, chunk=1)
    x = _signal(1 << 15, seed=9)
    q0 = 7000
    x[q0] = np.nan
    blk = _block(p)
    got = _run(blk, x, cuts=[q0 + 3])
    assert np.all(np.isfinite(got[:q0])) and np.all(np.isnan(got[q0:]))
    more = _run(blk, _signal(4096, seed=10))
    assert np.all(np.isnan(more))
    blk.reset()
    y = _signal(4096, seed=11)
    after = _run(blk, y)
    assert np.all(np.isfinite(after))
    _parity(p, after, y)


def test_search_range_edges():
    # f_min = 0: i_min clamps to 1
    p = FE.Params(FD, f_min=0.0, f_expected=20.0, f_max=60.0, chunk=3)
    assert FE.geometry(p)[1] == 1
    x = _signal(300000, f=31.7)
    _parity(p, _run(_block(p), x), x)
    # i_min == i_max: the reference's empty range gives k = i_max
    p = FE.Params(FD, sample_rate=1024.0, f_min=48.0, f_expected=50.0, f_max=48.0, chunk=5)
    N, a, b = FE.geometry(p)
    assert a == b == 12 and N == 256
    x = _signal(300000, f=48.4, fs=1024.0)
    got = _run(_block(p), x)
    _parity(p, got, x)
    assert abs(got[-1] - 48.4) < 0.5


def test_long_window_per_sample():
    """N = 2^16, C = 1: the truth at sampled positions the oracle shows to be valid"""
    p = FE.Params(FD, min_fft_size=1 << 16, chunk=1)
    N = FE.geometry(p)[0]
    assert N == 1 << 16
    x = _signal(N + 40000, f=50.3, seed=13)
    got = _run(_block(p), x, cuts=[N - 1, N + 20000])
    pos = np.linspace(N - 1, len(x) - 1, 48).astype(int)
    out, raw, valid, m = FE.fd_truth(p, x, only=pos)
    _margins_ok(p, m)
    assert valid[pos].all()
    assert np.all(got[:N - 1] == np.float32(p.f_expected))
    assert np.max(FE.rel_err(got[pos], raw[pos])) <= 1e-5


def test_two_handles_on_two_non_blocking_streams():
    import gnuradio4_amd as G
    pt, pf = FE.Params(TD, chunk=10), FE.Params(FD, chunk=1)
    xt, xf = _signal(500000, seed=21), _signal(500000, f=52.2, seed=22)
    want_t, want_f = _run(_block(pt), xt), _run(_block(pf), xf)
    bt, bf = _block(pt), _block(pf)
    st, sf = torch.cuda.Stream(), torch.cuda.Stream()
    dt, df = torch.from_numpy(xt).cuda(), torch.from_numpy(xf).cuda()
    torch.cuda.synchronize()
    outs_t, outs_f = [], []
    for k in range(5):
        a, b = k * 100000, (k + 1) * 100000
        with torch.cuda.stream(st):
            outs_t.append(bt.process_bulk(dt[a:b]))
        with torch.cuda.stream(sf):
            outs_f.append(bf.process_bulk(df[a:b]))
    torch.cuda.synchronize()
    got_t = torch.cat(outs_t).cpu().numpy().astype(np.float64)
    got_f = torch.cat(outs_f).cpu().numpy().astype(np.float64)
    assert np.max(FE.rel_err(got_t, want_t)) <= 1e-6 and np.max(FE.rel_err(got_f, want_f)) <= 1e-6
    assert isinstance(G.FrequencyEstimatorTimeDomain, type)


def test_decimating_forms_and_argument_checks():
    import gnuradio4_amd as G
    from gnuradio4_amd.capi import Gr4HipError
    t = G.FrequencyEstimatorTimeDomain(decimating=True, n_periods=3, f_min=45.0, f_max=55.0)
    f = G.FrequencyEstimatorFrequencyDomain(decimating=True, min_fft_size=4096, f_min=45.0, f_max=55.0)
    assert t.chunk == 10 and f.chunk == 4096
    x = torch.from_numpy(FE.qa_signal(50.3, 1000.0, 0.01, 40960)).cuda()
    assert abs(float(t.process_bulk(x[:1280])[-1]) - 50.3) < 0.03  # (the QA's lengths: its float phase accumulator drifts over longer signals)
    assert abs(float(f.process_bulk(x)[-1]) - 50.3) < 1.0
    with pytest.raises(Gr4HipError):
        t.process_bulk(x[:15])  # not a multiple of the chunk
    with pytest.raises(Gr4HipError):
        G.FrequencyEstimatorTimeDomain(f_max=600.0)
