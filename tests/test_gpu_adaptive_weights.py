"""The adaptive (MVDR / Capon) beamformer weights on the device (gr4hip_mvdr_*; csrc/adaptive_weights.hip) against their oracle
(tests/adaptive_weights_oracle.py).  Parity is against the long-double routine under the definition's bound
    per component |W - W_exact| <= 2^-24 |W_exact| + (8 + S) cond2(R') 2^-53 ||w||_2,   |P - P_exact| <= 2^-24 P + 2 (8 + S) cond2(R') 2^-53 P;
the device is not required to equal the ordered float64 routine bit for bit (it evaluates the sums as fma chains), each test prints how many components do.
Matrices are cross_spectrum_oracle.cross_ordered(streams(S, 64 n_spectra, N, 7 S + B), 64, mean=True), steering vectors of unit modulus.  Every output is
filled with a canary first, and what lies behind the written region is checked untouched.

Shapes (S, B, N, n_spectra): the smallest problem; N = 10 and 70 (no multiple of a bin tile, several tiles plus a ragged one); S = 9 with B = 17 and S = 17 (odd
sizes on both sides of 8 and 16); S = 32 with B = 32 (a tile of 8 bins, two passes of 16 beams) and with B = 1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import adaptive_weights_oracle as AO
import beamformer_oracle as BO
import cross_spectrum_oracle as XO
import oracle_lib as O

pytestmark = pytest.mark.gpu
CANARY = -77.25
A = 64
SHAPES = [(2, 1, 8, 1), (3, 5, 10, 2), (8, 4, 8, 1), (9, 17, 8, 1), (17, 3, 8, 2), (32, 32, 4, 1), (32, 1, 70, 3)]
HOST_BIN = os.path.join(O.ROOT, "build", "host", "test_host_adaptive_weights")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
INV = -101


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    assert G.capi.INVALID_ARGUMENT == INV
    return G


_cases = {}


def case(S, B, N, Q):
    """(V complex64 [Q, P, N], a complex64 [B, S, N]): computed once, shared, read-only"""
    key = (S, B, N, Q)
    if key not in _cases:
        V = XO.cross_ordered(XO.streams(S, A * Q, N, 7 * S + B), A, mean=True)
        a = AO.steering(B, S, N, 100 * S + B)
        for x in (V, a):
            x.setflags(write=False)
        _cases[key] = (V, a)
    return _cases[key]


_exact = {}


def exact(S, B, N, Q, loading):
    key = (S, B, N, Q, loading)
    if key not in _exact:
        V, a = case(S, B, N, Q)
        _exact[key] = AO.mvdr_exact(V, a, loading)[:2] + (AO.kappa(V, S, loading), AO.mvdr_ordered(V, a, loading)[0])
    return _exact[key]


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def run(G, blk, V, power=True):
    """weights (and power) of matrices V through the C-ABI into canary-filled tensors with one spare row each; (W [Q, B, S, N], P [Q, B, N] or None)"""
    S, B, N = blk.n_streams, blk.n_beams, blk.n_bins
    Q = V.shape[0]
    w = torch.full(((Q + 1) * B * S * N * 2,), CANARY, dtype=torch.float32, device="cuda")
    p = torch.full(((Q + 1) * B * N,), CANARY, dtype=torch.float32, device="cuda")
    v = dev(V)
    rc = G.capi.lib().gr4hip_mvdr_process(blk._h, v.data_ptr(), Q, w.data_ptr(), p.data_ptr() if power else None, stream())
    assert rc == 0, G.capi.lib().gr4hip_last_error()
    w, p = w.cpu().numpy(), p.cpu().numpy()
    assert np.all(w[Q * B * S * N * 2:] == CANARY) and np.all(p[Q * B * N if power else 0:] == CANARY)  # nothing behind the results, nothing at all without power
    return w[:Q * B * S * N * 2].view(np.complex64).reshape(Q, B, S, N), (p[:Q * B * N].reshape(Q, B, N) if power else None)


def make(G, a, loading=0.0):
    a = np.array(a)
    blk = G.AdaptiveWeights(a.shape[1], a.shape[0], a.shape[2], loading)
    blk.set_steering(a)
    return blk


@pytest.mark.parametrize("loading", [0.0, 1e-2])
@pytest.mark.parametrize("S,B,N,Q", SHAPES)
def test_parity_with_the_long_double_result_under_the_bound(G, S, B, N, Q, loading):
    V, a = case(S, B, N, Q)
    Wx, Px, kap, W64 = exact(S, B, N, Q, loading)
    blk = make(G, a, loading)
    W, P = run(G, blk, V)
    rw, rp = AO.ratios(W, P, Wx, Px, kap, S)
    same = float(np.mean(u32(W) == u32(W64)))
    print(f"S={S} B={B} N={N} Q={Q} loading={loading}: cond2 <= {kap.max():.3g}, worst error / bound: W {rw:.3f}, P {rp:.3f}; {100 * same:.2f} % of the components equal the ordered float64 routine's")
    assert rw <= 1.0 and rp <= 1.0
    resp = (W.astype(np.complex128) * np.asarray(a, np.complex128)[None]).sum(axis=2)
    assert np.max(np.abs(resp - 1)) <= 1e-6  # distortionless
    assert blk.stats() == (Q * N, 0)


@pytest.mark.parametrize("S,B,N", [(3, 5, 10), (32, 32, 4), (32, 1, 70)])
def test_the_result_does_not_depend_on_the_cut_or_on_the_power_output(G, S, B, N):
    V, a = case(S, B, N, 3)
    blk = make(G, a, 1e-2)
    W, P = run(G, blk, V)
    for q in range(3):
        Wq, Pq = run(G, blk, V[q:q + 1])
        assert np.array_equal(u32(Wq[0]), u32(W[q])) and np.array_equal(u32(Pq[0]), u32(P[q])), q
    W0, none = run(G, blk, V, power=False)  # d_power = NULL
    assert none is None and np.array_equal(u32(W0), u32(W))
    Wp, Pp = blk.process_bulk(dev(V), power=True)  # the Python block
    assert tuple(Wp.shape) == (3, B, S, N) and tuple(Pp.shape) == (3, B, N)
    assert np.array_equal(u32(Wp.cpu().numpy()), u32(W)) and np.array_equal(u32(Pp.cpu().numpy()), u32(P))
    assert np.array_equal(u32(blk.process_bulk(dev(V)).cpu().numpy()), u32(W))


def test_a_failed_bin_is_nan_in_exactly_its_place_and_counted(G):
    S, B, N = 4, 3, 6
    V, bad = AO.hand_made(S, N)
    a = AO.steering(B, S, N, 9)
    blk = make(G, a)
    W, P = run(G, blk, V)
    want = np.zeros((4, N), bool)
    for q, c in bad:
        want[q, c] = True
    hit_w, hit_p = np.broadcast_to(want[:, None, None, :], W.shape), np.broadcast_to(want[:, None, :], P.shape)
    assert np.array_equal(np.isnan(W.real) & np.isnan(W.imag), hit_w) and np.array_equal(np.isnan(P), hit_p)
    assert np.all(np.isfinite(W[~hit_w])) and np.all(np.isfinite(P[~hit_p]))
    clean = XO.cross_ordered(XO.streams(S, 4 * 16, N, 5), 16, mean=True)
    W0, P0 = run(G, make(G, a), clean)
    assert np.array_equal(u32(W[~hit_w]), u32(W0[~hit_w])) and np.array_equal(u32(P[~hit_p]), u32(P0[~hit_p]))  # the neighbours: the same bits as without the failures
    assert blk.stats() == (4 * N - 4, 4)
    run(G, blk, V[1:3])
    assert blk.stats() == (4 * N - 4 + 2 * N - 2, 6)  # since the block was made


def test_a_nan_in_a_steering_vector_reaches_only_its_beam_and_bin(G):
    S, B, N = 4, 3, 6
    V = XO.cross_ordered(XO.streams(S, 16, N, 5), 16, mean=True)
    a = np.array(AO.steering(B, S, N, 9))
    W0, P0 = run(G, make(G, a), V)
    a[1, 2, 3] = np.nan
    blk = make(G, a)
    W, P = run(G, blk, V)
    hit_w, hit_p = np.zeros(W.shape, bool), np.zeros(P.shape, bool)
    hit_w[:, 1, :, 3] = True
    hit_p[:, 1, 3] = True
    assert np.all(np.isnan(W[hit_w])) and np.all(np.isnan(P[hit_p]))
    assert np.array_equal(u32(W[~hit_w]), u32(W0[~hit_w])) and np.array_equal(u32(P[~hit_p]), u32(P0[~hit_p]))
    assert blk.stats() == (N, 0)  # not counted


def test_steering_and_loading_are_stream_ordered(G):
    """set_steering and set_loading between two calls, nothing waited for: the first call has the old values, the second the new ones"""
    S, B, N = 8, 4, 8
    V, a1 = case(S, B, N, 1)
    a2 = AO.steering(B, S, N, 4242)
    want1, _ = run(G, make(G, a1, 0.0), V)
    want2, _ = run(G, make(G, a2, 0.25), V)
    assert not np.array_equal(u32(want1), u32(want2))
    blk = make(G, a1, 0.0)
    v = dev(V)
    torch.cuda.synchronize()
    out1 = blk.process_bulk(v)
    blk.set_steering(dev(a2))  # a device tensor, taken as it is
    blk.set_loading(0.25)
    out2 = blk.process_bulk(v)
    torch.cuda.synchronize()
    assert np.array_equal(u32(out1.cpu().numpy()), u32(want1)) and np.array_equal(u32(out2.cpu().numpy()), u32(want2))
    short = np.ascontiguousarray(np.array(a1)[:, :, 0])  # the [B, S] form: the same vector in every bin
    blk.set_steering(short)
    want3, _ = run(G, make(G, np.repeat(short[:, :, None], N, axis=2), 0.25), V)
    assert np.array_equal(u32(blk.process_bulk(v).cpu().numpy()), u32(want3))


def test_the_weights_go_straight_into_the_beamformer(G):
    S, B, N, Q = 3, 5, 10, 2
    V, a = case(S, B, N, Q)
    W = make(G, a, 1e-2).process_bulk(dev(V))
    X = XO.streams(S, 7, N, 99)
    bf = G.Beamformer(S, B, N)
    for q in range(Q):
        bf.set_weights(W[q])  # a device tensor: row q of the call's output, as it lies
        Y = bf.process_bulk(dev(X)).cpu().numpy()
        assert np.array_equal(u32(Y), u32(BO.beams_ordered(W[q].cpu().numpy(), X))), q


def test_alignment_is_accepted_or_refused_as_the_header_says(G):
    S, B, N, Q = 3, 5, 10, 2
    V, a = case(S, B, N, Q)
    blk = make(G, a, 1e-2)
    want_w, want_p = run(G, blk, V)
    L = G.capi.lib()
    v = dev(V)
    nw, npow = Q * B * S * N * 2, Q * B * N
    w = torch.full((nw + 8,), CANARY, dtype=torch.float32, device="cuda")
    p = torch.full((npow + 8,), CANARY, dtype=torch.float32, device="cuda")
    assert w.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0
    # the weights at 4 bytes mod 8: refused, nothing written
    assert L.gr4hip_mvdr_process(blk._h, v.data_ptr(), Q, w.data_ptr() + 4, p.data_ptr(), stream()) == INV
    torch.cuda.synchronize()
    assert bool(torch.all(w == CANARY)) and bool(torch.all(p == CANARY))
    # the weights at 8 bytes mod 16 and the power at 4 bytes mod 8: accepted, the same bits
    assert L.gr4hip_mvdr_process(blk._h, v.data_ptr(), Q, w.data_ptr() + 8, p.data_ptr() + 4, stream()) == 0, L.gr4hip_last_error()
    wh, ph = w.cpu().numpy(), p.cpu().numpy()
    assert np.all(wh[:2] == CANARY) and np.all(wh[2 + nw:] == CANARY) and ph[0] == CANARY and np.all(ph[1 + npow:] == CANARY)
    assert np.array_equal(u32(wh[2:2 + nw]), u32(want_w).ravel()) and np.array_equal(u32(ph[1:1 + npow]), u32(want_p).ravel())
    # the matrices at 4 bytes mod 8: refused
    v2 = torch.zeros(v.numel() * 2 + 2, dtype=torch.float32, device="cuda")
    assert L.gr4hip_mvdr_process(blk._h, v2.data_ptr() + 4, Q, w.data_ptr(), None, stream()) == INV
    # an output over the matrices: refused
    assert L.gr4hip_mvdr_process(blk._h, v.data_ptr(), Q, v.data_ptr() + 8, None, stream()) == INV


def test_end_to_end_correlate_weights_beamform(G):
    """a half-wavelength line array of 8: a unit-power signal at broadside (a = 1), an interferer of amplitude 10 at a phase step of 0.3125 pi per element, unit
    noise.  CrossSpectrum(mean) -> AdaptiveWeights(loading 1e-3) -> Beamformer, nothing leaves the device.  The conventional beam's response to the
    interferer is 0.1875; numpy's float64 solve of this scenario gives at most 0.0102."""
    S, N, F = 8, 16, 256
    rng = np.random.default_rng(20261020)
    a_sig = np.ones(S, complex)
    a_int = np.exp(1j * np.pi * 0.3125 * np.arange(S))
    cn = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(2)
    X = (a_sig[:, None, None] * cn(F, N)[None] + 10.0 * a_int[:, None, None] * cn(F, N)[None] + cn(S, F, N)).astype(np.complex64)
    x = dev(X)
    vis = G.CrossSpectrum(S, N, F, mean=True).process_bulk(x)
    assert tuple(vis.shape) == (1, S * (S + 1) // 2, N)
    aw = G.AdaptiveWeights(S, 1, N, loading=1e-3)
    aw.set_steering(np.ones((1, S), np.complex64))
    W = aw.process_bulk(vis)
    bf = G.Beamformer(S, 1, N)
    bf.set_weights(W[0])
    Y = bf.process_bulk(x).cpu().numpy()
    Wh = W.cpu().numpy()[0, 0].astype(np.complex128)  # [S, N]
    r_int = np.abs((Wh * a_int[:, None]).sum(axis=0))
    r_sig = np.abs((Wh * a_sig[:, None]).sum(axis=0) - 1)
    print(f"response to the interferer <= {r_int.max():.4f} (conventional 0.1875), |response to the signal - 1| <= {r_sig.max():.2e}")
    assert aw.stats() == (N, 0)
    assert np.all(r_int <= 0.05)
    assert np.all(r_sig <= 1e-6)
    assert np.array_equal(u32(Y), u32(BO.beams_ordered(W.cpu().numpy()[0], X)))


@pytest.fixture(scope="module")
def device_run(tmp_path_factory):
    assert os.path.exists(HOST_BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_adaptive_weights.cpp and the plugin"
    prefix = str(tmp_path_factory.mktemp("mvdr") / "device")
    r = subprocess.run([HOST_BIN, "device", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r, prefix


@pytest.mark.parametrize("form", ["full", "short"])
@pytest.mark.parametrize("S,B,N,A_,loading", [(2, 1, 8, 64, 0.0), (3, 5, 16, 19, 1e-3), (9, 2, 8, 40, 1e-2)])
def test_the_host_block_on_the_device_is_the_c_abi(G, device_run, S, B, N, A_, loading, form):
    """CrossSpectrum (host) -> AdaptiveWeights on gpu:hip:0 -> sink: what the seam writes is what gr4hip_mvdr_process writes for the same matrices, bit for bit"""
    r, prefix = device_run
    assert r.returncode == 0 and "adaptive weights device: ok" in r.stdout and "FAIL" not in r.stdout
    assert "steering and loading again on the live handle (by settings in front of matrix 2 of 4): 128 weights" in r.stdout
    tag = f"{prefix}.S{S}.B{B}.N{N}.{form}"
    X = np.fromfile(tag + ".in", np.complex64).reshape(S, 2 * A_, N)
    a = np.fromfile(tag + ".a", np.complex64).reshape((B, S, N) if form == "full" else (B, S))
    got = np.fromfile(tag + ".out", np.complex64).reshape(2, B, S, N)
    if form == "short":
        a = np.ascontiguousarray(np.broadcast_to(a[:, :, None], (B, S, N)))
    V = XO.cross_ordered(X, A_, mean=True)
    want, _ = run(G, make(G, a, loading), V)
    assert np.array_equal(u32(got), u32(want))
