"""Host side of the adaptive beamformer weights (gr4hip_mvdr_*): symbols, every refusal that needs no device, the definition's lines in every place that states
them, and the C++ host mirror (gr::blocks::fft::AdaptiveWeights<float>: its CPU body in a host-domain graph CrossSpectrum -> AdaptiveWeights -> sink against the
oracle's long-double result under the bound, with per-bin steering vectors and with the [B, S] short form, the settings errors, the chunk sizes, gr:sample_rate,
the plugin registration).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_weights_oracle as AO
import cross_spectrum_oracle as XO
import oracle_lib as O

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_adaptive_weights")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
SYMBOLS = ["gr4hip_mvdr_create", "gr4hip_mvdr_set_steering", "gr4hip_mvdr_set_loading", "gr4hip_mvdr_process", "gr4hip_mvdr_stats", "gr4hip_mvdr_destroy"]
HOST_CASES = [(2, 1, 8, 64, 0.0), (3, 5, 16, 19, 1e-3), (9, 2, 8, 40, 1e-2)]  # (S, B, N, A, loading) of host/tests/test_host_adaptive_weights.cpp
MATRICES = 2


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    assert os.path.exists(BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_adaptive_weights.cpp and the plugin"
    prefix = str(tmp_path_factory.mktemp("mvdr") / "host")
    r = subprocess.run([BIN, "host", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r, prefix


def _create(L, S, B, N):
    h = C.c_void_p()
    return L.gr4hip_mvdr_create(C.byref(h), S, B, N), h


def test_symbols_exist_and_are_declared(L):
    from gnuradio4_amd import capi
    import gnuradio4_amd as G
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gr4hip.h")).read(), flags=re.S)
    raw = C.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in gr4hip.h"
        assert hasattr(raw, s) and s in capi.SIGNATURES
    for s in ("gr4hip_internal_mvdr_set_path", "gr4hip_internal_mvdr_last_path"):  # one kernel form ships: there are no path hooks
        assert not hasattr(raw, s) and s not in text and s not in capi.SIGNATURES
    assert hasattr(G, "AdaptiveWeights") and "AdaptiveWeights" in G.__all__
    for m in ("set_steering", "set_loading", "process_bulk", "stats", "steering_from_delays"):
        assert hasattr(G.AdaptiveWeights, m)
    assert L.gr4hip_abi_version() == 1


def test_the_definition_reads_the_same_everywhere():
    """the lines of the definition, in the header, the document, the oracle, the host block and the kernel file"""
    squash = lambda s: re.sub(r"[\s*/]+", "", s)
    lines = ["R_ij = V_ij (j < i),  R_ji = conj(V_ij),  R_ii = Re V_ii (the imaginary part is ignored)",
             "lambda = loading * (sum_i R_ii) / S ;   R'_ii = R_ii + lambda",
             "R' = L L^H   Cholesky, columns j ascending, every inner sum with k ascending:",
             "s_j  = R'_jj - sum_{k<j} |L_jk|^2 ;   L_jj = sqrt(s_j)",
             "L_ij = (R'_ij - sum_{k<j} L_ik conj(L_jk)) / L_jj            (i > j)",
             "per beam b:   L y = a_b  (forward, k ascending) ;   d = sum_k |y_k|^2",
             "L^H u = y  (backward) ;   w = u / d",
             "W[q][b][s][c] = conj(w_s)  rounded once to complex<float>"]
    for path in ("include/gr4hip.h", "ADAPTIVE_WEIGHTS.md", "tests/adaptive_weights_oracle.py", "gnuradio4_amd/host/include/gr4/blocks.hpp", "gnuradio4_amd/csrc/adaptive_weights.hip"):
        text = squash(open(os.path.join(ROOT, path)).read())
        for line in lines:
            assert squash(line) in text, (path, line)
    for path in ("include/gr4hip.h", "ADAPTIVE_WEIGHTS.md", "tests/adaptive_weights_oracle.py", "gnuradio4_amd/csrc/adaptive_weights.hip"):  # (the block has no power port)
        assert squash("P[q][b][c]    = (float)(1 / d)") in squash(open(os.path.join(ROOT, path)).read()), path


def test_create_refusals(L):
    from gnuradio4_amd import capi
    INV, UNS = capi.INVALID_ARGUMENT, capi.UNSUPPORTED
    assert L.gr4hip_mvdr_create(None, 2, 1, 64) == INV
    for args in ((0, 1, 64), (1, 1, 64), (2, 0, 64), (2, 1, 1), (2, 1, 0)):
        rc, h = _create(L, *args)
        assert rc == INV and not h.value, args
    # more than 32 streams or beams, more than 2^20 bins, B S n_bins above 2^24
    for args in ((33, 1, 64), (2, 33, 64), (2, 1, (1 << 20) + 1), (32, 32, (1 << 14) + 1), (17, 1, 1 << 20)):
        rc, h = _create(L, *args)
        assert rc == UNS and not h.value, args
    for args in ((32, 32, 1 << 14), (16, 1, 1 << 20), (2, 1, 2)):
        rc, h = _create(L, *args)
        assert rc == capi.OK and h.value, args
        L.gr4hip_mvdr_destroy(h)


def test_refusals_come_before_any_device_work(L):
    """every one of these returns its status with or without a device: the checks run on the host first, and a handle is host state until its first
    set_steering"""
    from gnuradio4_amd import capi
    INV = capi.INVALID_ARGUMENT
    S, B, N, Q = 3, 2, 64, 2
    P = S * (S + 1) // 2
    rc, h = _create(L, S, B, N)
    assert rc == capi.OK
    nv, nw, npow = Q * P * N * 2, Q * B * S * N * 2, Q * B * N
    buf = np.zeros(nv + nw + npow + 8, np.float32)  # (host memory: no call below gets as far as reading it)
    v = buf.ctypes.data + (-buf.ctypes.data) % 8
    w, p = v + nv * 4, v + (nv + nw) * 4
    proc = L.gr4hip_mvdr_process
    assert proc(None, v, Q, w, p, None) == INV
    assert proc(h, None, Q, w, p, None) == INV and proc(h, v, Q, None, p, None) == INV
    assert proc(h, v + 4, Q, w, p, None) == INV and proc(h, v, Q, w + 4, p, None) == INV  # complex buffers not aligned to 8 bytes
    assert proc(h, v, Q, w, p + 2, None) == INV  # the power output not aligned to 4
    assert proc(h, v, Q, v + 8, p, None) == INV and b"overlap" in L.gr4hip_last_error()  # the weights over the matrices
    assert proc(h, v, Q, w, v + nv * 4 - 4, None) == INV and b"overlap" in L.gr4hip_last_error()  # the power over the matrices' last value
    assert proc(h, v, Q, w, w + 8, None) == INV and b"overlap" in L.gr4hip_last_error()  # the power over the weights
    assert proc(h, v, Q, w, p, None) == INV and b"no steering" in L.gr4hip_last_error()  # process before any set_steering
    assert proc(h, v, Q, w, p + 4, None) == INV and b"no steering" in L.gr4hip_last_error()  # (a power output at 4 bytes mod 8 is fine as far as alignment goes)
    assert proc(h, v, Q, w, None, None) == INV and b"no steering" in L.gr4hip_last_error()
    assert L.gr4hip_mvdr_set_steering(None, v, None) == INV and L.gr4hip_mvdr_set_steering(h, None, None) == INV
    assert L.gr4hip_mvdr_set_steering(h, v + 4, None) == INV  # not aligned to 8 bytes
    for bad in (-1.0, -1e-300, float("inf"), float("-inf"), float("nan")):
        assert L.gr4hip_mvdr_set_loading(h, bad) == INV, bad
    assert L.gr4hip_mvdr_set_loading(None, 0.0) == INV
    for good in (0.0, 1e-3, 10.0):
        assert L.gr4hip_mvdr_set_loading(h, good) == capi.OK
    assert not buf.any()
    assert proc(h, v, 0, w, p, None) == capi.OK and proc(h, None, 0, None, None, None) == capi.OK  # no matrices: a no-op, with or without a device
    solved, failed = C.c_ulonglong(7), C.c_ulonglong(7)
    assert L.gr4hip_mvdr_stats(h, C.byref(solved), C.byref(failed)) == capi.OK and solved.value == 0 and failed.value == 0  # nothing has run
    assert L.gr4hip_mvdr_stats(None, C.byref(solved), C.byref(failed)) == INV
    assert L.gr4hip_mvdr_destroy(h) == capi.OK and L.gr4hip_mvdr_destroy(None) in (capi.OK, INV)


def test_python_block_refuses_on_the_host():
    import gnuradio4_amd as G
    from gnuradio4_amd import capi
    for args in ((1, 1, 8), (2, 0, 8), (2, 1, 1), (33, 1, 8)):
        with pytest.raises(capi.Gr4HipError):
            G.AdaptiveWeights(*args)
    with pytest.raises(capi.Gr4HipError):
        G.AdaptiveWeights(2, 1, 8, loading=-1.0)
    aw = G.AdaptiveWeights(3, 2, 8, loading=0.5)
    assert aw.loading == 0.5 and aw.n_baselines == 6
    with pytest.raises(capi.Gr4HipError):
        aw.set_loading(float("nan"))
    with pytest.raises(capi.Gr4HipError):
        aw.set_steering(np.ones((2, 4, 8), np.complex64))  # another shape
    assert aw.stats() == (0, 0)


def test_steering_from_delays_is_the_float64_formula_rounded_once():
    import gnuradio4_amd as G
    tau = np.array([[0.0, 1e-6, 2.5e-6], [0.0, -1e-6, -2.5e-6]])
    f = np.arange(8) * 125e3
    a = G.AdaptiveWeights.steering_from_delays(tau, f)
    want = np.exp(2j * np.pi * f[None, None, :] * tau[:, :, None]).astype(np.complex64)
    assert a.dtype == np.complex64 and a.shape == (2, 3, 8) and np.array_equal(a.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(a, np.conj(G.Beamformer.delay_weights(tau, f, normalise=False)))  # what the docstring says
    assert np.all(a[:, 0] == np.complex64(1))  # zero delay: 1 in every bin


def test_host_program_holds(host_run):
    """the settings errors, the chunk sizes, gr:sample_rate scaled by n_beams n_inputs / P, the reflected members, the C-ABI's refusals and the plugin
    registration are EXPECTs of the program"""
    r, _ = host_run
    assert r.returncode == 0 and "adaptive weights host: ok" in r.stdout and "FAIL" not in r.stdout
    assert "plugin: gr::blocks::fft::AdaptiveWeights<float32> available" in r.stdout


@pytest.mark.parametrize("form", ["full", "short"])
@pytest.mark.parametrize("S,B,N,A,loading", HOST_CASES)
def test_cpu_body_stays_within_the_bound_of_the_long_double_result(host_run, S, B, N, A, loading, form):
    _, prefix = host_run
    tag = f"{prefix}.S{S}.B{B}.N{N}.{form}"
    X = np.fromfile(tag + ".in", np.complex64).reshape(S, MATRICES * A, N)
    a = np.fromfile(tag + ".a", np.complex64).reshape((B, S, N) if form == "full" else (B, S))
    got = np.fromfile(tag + ".out", np.complex64).reshape(MATRICES, B, S, N)
    if form == "short":
        a = np.ascontiguousarray(np.broadcast_to(a[:, :, None], (B, S, N)))
    V = XO.cross_ordered(X, A, mean=True)  # (what CrossSpectrum's CPU body emits, bit for bit: tests/test_cross_spectrum_host.py)
    Wx, Px, failed = AO.mvdr_exact(V, a, loading)
    kap = AO.kappa(V, S, loading)
    assert not failed.any()
    rw, _ = AO.ratios(got, None, Wx, Px, kap, S)
    print(f"S={S} B={B} N={N} A={A} loading={loading} {form}: cond2 <= {kap.max():.3g}, worst error / bound: W {rw:.3f}")
    assert rw <= 1.0
