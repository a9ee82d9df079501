"""Savitzky-Golay on the host side, through the C ABI without a device: gr4hip_savgol_design / gr4hip_savgol_pinv_row against the numpy oracle and exact rational
least squares (kept rank, coefficients before and after the rounding to T, the `ambiguous` flag), the argument checks, the zero-phase handle's limits, the Python
blocks' names, and the host C++ program (gnuradio4_amd/host/tests/test_host_savitzky_golay.cpp): block defaults, settings by name, the plugin's four names and the
CPU bodies of both blocks in graphs, whose outputs are compared here with the oracle.

The bar on the float64 row of the truncated pseudo-inverse, relative to its largest entry (SAVITZKY_GOLAY.md "Design: measured"):
  E         the worst deviation of the ORACLE (numpy's LAPACK SVD) from the exact rational coefficients over the settings below where the rule drops nothing
  nothing dropped     library vs exact      <= max(8 E, 4 eps64)                          (8: Jacobi and LAPACK differ by small constants)
  something dropped   library vs oracle     <= max(8 E, 4 eps64) * sigma_0 / sigma_min_kept   (no exact answer exists: the two float64 designs against each other)
The T-rounded float coefficients may differ from the oracle's by one ulp of the largest coefficient."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import savitzky_golay_oracle as SG

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_savitzky_golay")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
F32, F64 = 8, 9

# (dtype, W, p, d, alignment): the issue's list
SETTINGS = [(np.float32, 11, 4, 0, "Centred"), (np.float32, 11, 4, 0, "Causal"), (np.float32, 25, 4, 2, "Centred"), (np.float32, 51, 4, 0, "Centred"),
            (np.float32, 101, 4, 0, "Centred"), (np.float32, 64, 3, 0, "Causal"), (np.float32, 21, 10, 0, "Centred"), (np.float32, 1, 0, 0, "Centred"),
            (np.float32, 2, 1, 0, "Centred"), (np.float32, 5, 10, 10, "Centred"), (np.float32, 31, 6, 0, "Centred"),
            (np.float64, 11, 4, 1, "Centred"), (np.float64, 31, 6, 0, "Centred"), (np.float64, 101, 6, 1, "Centred")]
EPS64 = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    return BIN


def _did(dtype):
    return F32 if dtype == np.float32 else F64


def _al(alignment):
    return 1 if alignment == "Causal" else 0


def _lib_row(L, dtype, W, p, d, alignment):
    from gnuradio4_amd import capi
    row, info = np.full(max(W, 1), np.nan), capi.SavgolInfo()
    assert L.gr4hip_savgol_pinv_row(_did(dtype), W, p, d, _al(alignment), row.ctypes.data, C.byref(info)) == 0, L.gr4hip_last_error()
    return row, info


def _lib_design(L, dtype, W, p, d, delta, alignment):
    from gnuradio4_amd import capi
    c, info = np.full(max(W, 1), np.nan, dtype), capi.SavgolInfo()
    assert L.gr4hip_savgol_design(_did(dtype), W, p, d, float(delta), _al(alignment), c.ctypes.data, C.byref(info)) == 0, L.gr4hip_last_error()
    return c, info


@pytest.fixture(scope="module")
def oracle_deviation():
    """E: the oracle's own worst deviation from exact least squares over the settings where nothing is dropped"""
    worst = 0.0
    for dtype, W, p, d, alignment in SETTINGS:
        row, info = SG.pinv_row(dtype, W, p, d, alignment)
        if info["rank"] == info["p"] + 1:
            exact = np.array([float(v) for v in SG.exact_row(W, p, d, alignment)])
            worst = max(worst, float(np.max(np.abs(row - exact)) / np.max(np.abs(exact))))
    return worst


def _coeff_tol(want, oracle_deviation):
    """T-rounded coefficients, library against oracle: one ulp of the largest for float; for double the two float64 rows differ by the design bar of this file"""
    big = np.max(np.abs(want))
    return float(np.spacing(big)) + (max(8 * oracle_deviation, 4 * EPS64) * float(big) if want.dtype == np.float64 else 0.0)


@pytest.mark.parametrize("dtype,W,p,d,alignment", SETTINGS)
def test_design_matches_the_oracle(L, oracle_deviation, dtype, W, p, d, alignment):
    row, info = _lib_row(L, dtype, W, p, d, alignment)
    want, oi = SG.pinv_row(dtype, W, p, d, alignment)
    assert (info.window_size, info.poly_order, info.deriv_order) == (oi["W"], oi["p"], oi["d"])
    assert info.rank == oi["rank"]
    assert abs(info.sigma_max - oi["sigma_max"]) <= 1e-12 * oi["sigma_max"] and abs(info.sigma_min_kept - oi["sigma_min_kept"]) <= 1e-9 * oi["sigma_max"]
    assert abs(info.threshold - oi["threshold"]) <= 1e-12 * oi["threshold"]
    assert bool(info.ambiguous) == oi["ambiguous"]
    bar = max(8 * oracle_deviation, 4 * EPS64)
    dropped = oi["rank"] < oi["p"] + 1
    if dropped:
        bar *= oi["sigma_max"] / oi["sigma_min_kept"]
        ref = want
    else:
        ref = np.array([float(v) for v in SG.exact_row(W, p, d, alignment)])
    dev = float(np.max(np.abs(row - ref)) / np.max(np.abs(ref)))
    print(f"{np.dtype(dtype).name} W {W} p {p} d {d} {alignment}: rank {info.rank}/{oi['p'] + 1}, cond {oi['sigma_max'] / oi['sigma_min_kept']:.3g}, "
          f"library vs {'oracle' if dropped else 'exact'} {dev:.3g} (bar {bar:.3g}, E {oracle_deviation:.3g}), ambiguous {info.ambiguous}")
    assert dev <= bar
    # after the rounding to T and the scale
    for delta in (1.0, 1e-3):
        c, _ = _lib_design(L, dtype, W, p, d, delta, alignment)
        cw, _ = SG.design(dtype, W, p, d, delta, alignment)
        big = np.max(np.abs(cw))
        if dtype == np.float32:
            assert np.max(np.abs(c.astype(np.float64) - cw.astype(np.float64))) <= float(np.spacing(big))  # one ulp of the largest coefficient
        else:
            assert np.max(np.abs(c - cw)) <= bar * big + float(np.spacing(big))


def test_ambiguous_is_reported_where_a_singular_value_sits_on_the_threshold(L):
    _, info = _lib_row(L, np.float32, 31, 6, 0, "Centred")
    s, thr = SG.pinv_row(np.float32, 31, 6, 0)[1]["sigma"], info.threshold
    assert info.ambiguous == 1 and np.min(np.abs(np.log2(s / thr))) < 0.1
    assert _lib_row(L, np.float32, 11, 4, 0, "Centred")[1].ambiguous == 0
    assert _lib_row(L, np.float64, 31, 6, 0, "Centred")[1].ambiguous == 0


def test_argument_checks(L, oracle_deviation):
    from gnuradio4_amd import capi
    c = np.zeros(16, np.float64)
    for bad in (0, 7, 10, 99, -1):
        assert L.gr4hip_savgol_design(bad, 11, 4, 0, 1.0, 0, c.ctypes.data, None) == capi.INVALID_ARGUMENT
        assert b"dtype" in L.gr4hip_last_error()
        assert L.gr4hip_savgol_pinv_row(bad, 11, 4, 0, 0, c.ctypes.data, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_savgol_design(F64, 11, 4, 0, 1.0, 2, c.ctypes.data, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_savgol_design(F64, 11, 4, 0, 1.0, 0, None, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_savgol_design(F64, 1 << 30, 1 << 30, 0, 1.0, 0, c.ctypes.data, None) == capi.UNSUPPORTED
    # delta <= 0 is clamped to eps_T, not refused (SavitzkyGolay.hpp:98)
    for dtype in (np.float32, np.float64):
        for delta in (0.0, -2.5):
            got, _ = _lib_design(L, dtype, 7, 2, 1, delta, "Centred")
            want, _ = SG.design(dtype, 7, 2, 1, delta, "Centred")
            assert np.all(np.isfinite(got)) and np.max(np.abs(got - want)) <= _coeff_tol(want, oracle_deviation)
    # window_size 0 is one coefficient, 1 (:95)
    got, info = _lib_design(L, np.float32, 0, 4, 2, 1.0, "Centred")
    assert got[0] == 1.0 and (info.window_size, info.poly_order, info.deriv_order, info.rank) == (1, 0, 0, 1)


def test_zero_phase_handle_limits(L, oracle_deviation):
    from gnuradio4_amd import capi
    assert capi.SAVGOL_ZP_MAX_WINDOW == 255 and "#define GR4HIP_SAVGOL_ZP_MAX_WINDOW 255\n" in open(os.path.join(ROOT, "include", "gr4hip.h")).read()
    assert int(L.gr4hip_savgol_zp_tile()) >= 2 * 255  # a row longer than a tile is longer than every window: the boundary map wraps once
    h = C.c_void_p()
    for dtype in (F32, F64):
        p = capi.SavgolZpParams(dtype, 256, 4, 0, capi.SAVGOL_REFLECT)
        assert L.gr4hip_savgol_zp_create(C.byref(h), C.byref(p)) == capi.UNSUPPORTED and not h.value
        assert b"window_size" in L.gr4hip_last_error()
        p = capi.SavgolZpParams(dtype, 255, 4, 0, capi.SAVGOL_REPLICATE)
        assert L.gr4hip_savgol_zp_create(C.byref(h), C.byref(p)) == 0 and h.value  # a handle owns no device memory: made without a device
        c = np.zeros(255, np.float32 if dtype == F32 else np.float64)
        info = capi.SavgolInfo()
        assert L.gr4hip_savgol_zp_coeffs(h, c.ctypes.data, C.byref(info)) == 0
        want, oi = SG.design(c.dtype.type, 255, 4, 0)
        assert info.rank == oi["rank"] and np.max(np.abs(c - want)) <= _coeff_tol(want, oracle_deviation)
        assert L.gr4hip_savgol_zp_process(h, None, None, 0, 1, 0, None) == 0  # n == 0: a no-op (:180)
        assert L.gr4hip_savgol_zp_process(h, 64, 64, 8, 1, 8, None) == capi.INVALID_ARGUMENT and b"overlap" in L.gr4hip_last_error()  # refused before any device work
        assert L.gr4hip_savgol_zp_process(h, 64, 64 + 4 * c.itemsize, 8, 1, 8, None) == capi.INVALID_ARGUMENT
        assert L.gr4hip_savgol_zp_process(h, 66, 4096, 8, 1, 8, None) == capi.INVALID_ARGUMENT and b"aligned" in L.gr4hip_last_error()
        assert L.gr4hip_savgol_zp_process(h, 64, 4096, 8, 2, 7, None) == capi.INVALID_ARGUMENT and b"row_stride" in L.gr4hip_last_error()
        q = capi.SavgolZpParams(dtype, 256, 4, 0, capi.SAVGOL_REFLECT)
        assert L.gr4hip_savgol_zp_set_params(h, C.byref(q)) == capi.UNSUPPORTED
        q = capi.SavgolZpParams(F64 if dtype == F32 else F32, 11, 4, 0, capi.SAVGOL_REFLECT)
        assert L.gr4hip_savgol_zp_set_params(h, C.byref(q)) == capi.INVALID_ARGUMENT
        q = capi.SavgolZpParams(dtype, 11, 4, 0, 7)
        assert L.gr4hip_savgol_zp_set_params(h, C.byref(q)) == capi.INVALID_ARGUMENT
        assert L.gr4hip_savgol_zp_coeffs(h, c.ctypes.data, C.byref(info)) == 0 and info.window_size == 255  # a refused update leaves the handle as it was
        q = capi.SavgolZpParams(dtype, 5, 10, 10, capi.SAVGOL_REFLECT)
        assert L.gr4hip_savgol_zp_set_params(h, C.byref(q)) == 0
        assert L.gr4hip_savgol_zp_coeffs(h, c.ctypes.data, C.byref(info)) == 0 and (info.window_size, info.poly_order, info.deriv_order) == (5, 4, 4)
        assert L.gr4hip_savgol_zp_destroy(h) == 0
        h = C.c_void_p()
    p = capi.SavgolZpParams(F32 + 2, 11, 4, 0, capi.SAVGOL_REFLECT)
    assert L.gr4hip_savgol_zp_create(C.byref(h), C.byref(p)) == capi.INVALID_ARGUMENT and not h.value


def test_python_names_and_design():
    import torch
    import gnuradio4_amd as G
    for name in ("SavitzkyGolayFilter", "SavitzkyGolayDataSetFilter", "design_savitzky_golay"):
        assert name in G.__all__ and hasattr(G, name)
    assert G.SavitzkyGolayFilter._names == ("window_size", "poly_order", "deriv_order", "sample_rate", "alignment")
    assert G.SavitzkyGolayDataSetFilter._names == ("window_size", "poly_order", "deriv_order", "boundary_policy")
    assert G.SavitzkyGolayDataSetFilter.tile() == int(G.capi.lib().gr4hip_savgol_zp_tile())
    c, info = G.design_savitzky_golay(torch.float32, 51, 4, 1, 1e-3, "Causal")
    want, oi = SG.design(np.float32, 51, 4, 1, 1e-3, "Causal")
    assert c.dtype == np.float32 and info.rank == oi["rank"] and np.max(np.abs(c - want)) <= np.spacing(np.max(np.abs(want)))
    c2, _ = G.design_savitzky_golay(torch.float32, 51, 4, 1, 1e-3, "Sideways")  # anything but "Causal" is Centred
    assert np.array_equal(c2, G.design_savitzky_golay(torch.float32, 51, 4, 1, 1e-3)[0]) and not np.array_equal(c2, c)
    with pytest.raises(G.capi.Gr4HipError):
        G.design_savitzky_golay(torch.complex64)
    f = G.SavitzkyGolayDataSetFilter(torch.float64, 21, 3, 1, "Replicate")  # host-only to make
    assert (f.window_size, f.poly_order, f.deriv_order, f.boundary_policy) == (21, 3, 1, "Replicate")
    with pytest.raises(G.capi.Gr4HipError):
        f.set_params(window_size=300)
    assert f.window_size == 21
    with pytest.raises(TypeError):
        f.set_params(alignment="Causal")
    with pytest.raises(G.capi.Gr4HipError):
        f.process(torch.zeros(8, dtype=torch.float64))  # a host tensor is refused, never filtered on the CPU
    f.close()


def test_device_blocks_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        return
    import gnuradio4_amd as G
    with pytest.raises(G.capi.Gr4HipError):
        G.SavitzkyGolayFilter(torch.float32)  # its FIR handle needs device memory: no silent CPU path


# ------------------------------------------------------------------------------------------------ the host C++ program
def _stream():
    rng = np.random.default_rng(5)
    return (rng.standard_normal(5000) + 1e-3 * np.arange(5000)).astype(np.float32)


def check_graph_outputs(tmp_path, tag):
    """the files of test_host_savitzky_golay against the oracle; the bars are those of a T-precision accumulation (the CPU bodies sum in T like the reference,
    the device sums in float64): (W + 1) eps_T sum |c_k x_k| per streaming output, 2 (W + 1) eps_T S^2 M for the two passes with S = sum |c|, M = max |x|.
    Returns the outputs by name."""
    x = _stream()
    out = {}
    for name, dtype, (W, p, d, rate, al) in (("stream_f32", np.float32, (11, 4, 1, 1000.0, "Causal")), ("stream_f64", np.float64, (33, 3, 0, 1.0, "Centred"))):
        xs = x.astype(dtype)
        c, _ = SG.design(dtype, W, p, d, float(dtype(1) / dtype(np.float32(rate))), al)
        want, mag = SG.streaming(c, xs)
        got = np.fromfile(tmp_path / f"{name}.{tag}.bin", dtype)
        assert got.size == xs.size
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= (W + 1) * float(np.finfo(dtype).eps) * mag + 1e-300), name
        out[name] = got
    # stream_set: {5, 2, 0} up to sample 2000, {11, 2, 0} with an empty history from there on
    c5, _ = SG.design(np.float32, 5, 2, 0)
    c11, _ = SG.design(np.float32, 11, 2, 0)
    got = np.fromfile(tmp_path / f"stream_set.{tag}.bin", np.float32)
    for sl, c in ((slice(0, 2000), c5), (slice(2000, 5000), c11)):
        want, mag = SG.streaming(c, x[sl])
        assert np.all(np.abs(got[sl].astype(np.float64) - want.astype(np.float64)) <= (len(c) + 1) * float(np.finfo(np.float32).eps) * mag + 1e-300), sl
    out["stream_set"] = got
    for name, dtype, (W, p, d, policy), nbins in (("dataset_f32", np.float32, (11, 4, 0, "Reflect"), 256), ("dataset_f64", np.float64, (8, 2, 1, "Replicate"), 128)):
        xin = np.fromfile(tmp_path / f"{name}.in.bin", dtype).reshape(3, 4 * nbins)  # three DataSets, each four signals of nbins values, filtered as ONE sequence
        got = np.fromfile(tmp_path / f"{name}.{tag}.bin", dtype).reshape(3, 4 * nbins)
        c, _ = SG.design(dtype, W, p, d)
        S = float(np.abs(c.astype(np.float64)).sum())
        for f in range(3):
            want, _ = SG.zero_phase(c, xin[f], policy)
            bar = 2 * (W + 1) * float(np.finfo(dtype).eps) * S * S * float(np.max(np.abs(xin[f])))
            assert np.max(np.abs(got[f].astype(np.float64) - want.astype(np.float64))) <= bar, (name, f)
        out[name] = got
    # dataset_gap: DataSets of 32, 0 and 32 values through {11, 4, 0, Reflect}; the empty one is passed through, the other two are under the same bar
    xin = np.fromfile(tmp_path / "dataset_gap.in.bin", np.float32).reshape(2, 32)
    got = np.fromfile(tmp_path / f"dataset_gap.{tag}.bin", np.float32).reshape(2, 32)
    c, _ = SG.design(np.float32, 11, 4, 0)
    S = float(np.abs(c.astype(np.float64)).sum())
    for f in range(2):
        want, _ = SG.zero_phase(c, xin[f], "Reflect")
        bar = 2 * (11 + 1) * float(np.finfo(np.float32).eps) * S * S * float(np.max(np.abs(xin[f])))
        assert np.max(np.abs(got[f].astype(np.float64) - want.astype(np.float64))) <= bar, ("dataset_gap", f)
    out["dataset_gap"] = got
    # dataset_retune: three DataSets of 32 values, {11, 4, 0, Reflect} for the first, window_size 7 by settings from the second on; the same bar per window
    xin = np.fromfile(tmp_path / "dataset_retune.in.bin", np.float32).reshape(3, 32)
    got = np.fromfile(tmp_path / f"dataset_retune.{tag}.bin", np.float32).reshape(3, 32)
    for f, W in enumerate((11, 7, 7)):
        c, _ = SG.design(np.float32, W, 4, 0)
        S = float(np.abs(c.astype(np.float64)).sum())
        want, _ = SG.zero_phase(c, xin[f], "Reflect")
        bar = 2 * (W + 1) * float(np.finfo(np.float32).eps) * S * S * float(np.max(np.abs(xin[f])))
        assert np.max(np.abs(got[f].astype(np.float64) - want.astype(np.float64))) <= bar, ("dataset_retune", f)
    out["dataset_retune"] = got
    return out


def test_blocks_defaults_settings_plugin_and_cpu_bodies(prog, tmp_path):
    x = _stream()
    x.tofile(tmp_path / "x.f32")
    x.astype(np.float64).tofile(tmp_path / "x.f64")
    r = subprocess.run([prog, PLUGIN, "host", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed (compute_domain host)" in r.stdout
    check_graph_outputs(tmp_path, "host")


def test_device_graph_fails_loudly_without_gpu(prog, tmp_path):
    import torch
    if torch.cuda.is_available():
        return  # (with a device the same command is tests/test_gpu_savitzky_golay.py::test_graphs_on_the_device)
    x = _stream()
    x.tofile(tmp_path / "x.f32")
    x.astype(np.float64).tofile(tmp_path / "x.f64")
    r = subprocess.run([prog, PLUGIN, "gpu:hip:0", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
