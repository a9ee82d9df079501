"""CPU-side checks of PowerFactor / SystemUnbalance: the refusals of gr4hip_powerfactor_process / gr4hip_unbalance_process (include/gr4hip.h "Power factor and
system unbalance") before any device work, the exported symbols, the shared arithmetic header under sanitizers, and the host mirror blocks in host-domain graphs
against the oracle."""
import os
import subprocess

import numpy as np
import pytest

import electrical_oracle as EO

TNAME = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
HOST_PHASE_BOUND_ULP = 2.0  # CONVERTERS.md's host bound: two libraries within 1 ulp of the true value differ by at most 2


@pytest.fixture(scope="module")
def capi():
    from gnuradio4_amd import capi
    capi.lib()
    return capi


def test_symbols_are_exported_and_declared(capi):
    L = capi.lib()
    for name in ("gr4hip_powerfactor_process", "gr4hip_unbalance_process", "gr4hip_electrical_tile"):
        assert name in capi.SIGNATURES and hasattr(L, name)
    tile = L.gr4hip_electrical_tile()
    assert tile == 256 * 8  # 256 lanes x two 16-byte vectors of float / four of double per row


# device pointers the refusals never dereference: 16-byte aligned, far apart
A, B, C_, D, E, F = (0x10000000 + k * 0x01000000 for k in range(6))


def test_powerfactor_refusals_come_before_any_device_work(capi):
    L = capi.lib()
    INV, OK = capi.INVALID_ARGUMENT, capi.OK

    def pf(dtype=capi.F32, np_=3, P=A, S=B, in_stride=100, f=C_, a=D, out_stride=100, n=100):
        return L.gr4hip_powerfactor_process(dtype, np_, P, S, in_stride, f, a, out_stride, n, None)
    for dtype in (-1, capi.I32, capi.C32, capi.C64, 12, 13, 99):
        assert pf(dtype=dtype) == INV, dtype
    assert b"dtype" in L.gr4hip_last_error()
    for np_ in (0, 17, 1000):
        assert pf(np_=np_) == INV
    assert pf(P=None) == INV and pf(S=None) == INV
    assert pf(in_stride=99) == INV and pf(out_stride=99) == INV
    assert pf(np_=1, in_stride=99) == INV  # (also with one phase, where no second row exists)
    for dtype, es in ((capi.F32, 4), (capi.F64, 8)):
        span = (2 * 100 + 100) * es
        for out in ("f", "a"):
            for inp in ("P", "S"):
                base = {"P": A, "S": B}[inp]
                assert pf(dtype=dtype, **{out: base}) == INV                      # the same memory
                assert pf(dtype=dtype, **{out: base + span - es}) == INV          # the output begins on the input's last element
                assert pf(dtype=dtype, **{out: base - span + es}) == INV          # the output ends on the input's first element
                assert b"overlaps" in L.gr4hip_last_error()
        assert pf(dtype=dtype, P=A + es // 2) == INV and pf(dtype=dtype, a=D + es // 2) == INV  # not aligned to the element
    # n == 0 is OK and touches nothing: not even the pointers are looked at; a bad dtype or phase count is still refused
    assert pf(n=0) == OK and pf(n=0, P=None, S=None, f=None, a=None, in_stride=0, out_stride=0) == OK
    assert pf(n=0, dtype=capi.C32) == INV and pf(n=0, np_=0) == INV


def test_unbalance_refusals_come_before_any_device_work(capi):
    L = capi.lib()
    INV, OK = capi.INVALID_ARGUMENT, capi.OK

    def ub(dtype=capi.F32, np_=3, U=A, I=B, P=C_, in_stride=100, t=D, u=E, i=F, n=100):
        return L.gr4hip_unbalance_process(dtype, np_, U, I, P, in_stride, t, u, i, n, None)
    for dtype in (-1, capi.I32, capi.C32, capi.C64, 12, 13, 99):
        assert ub(dtype=dtype) == INV, dtype
    for np_ in (0, 1, 17, 1000):  # at least two phases
        assert ub(np_=np_) == INV
    assert b"n_phases" in L.gr4hip_last_error()
    assert ub(U=None) == INV and ub(I=None) == INV and ub(P=None) == INV
    assert ub(in_stride=99) == INV
    for dtype, es in ((capi.F32, 4), (capi.F64, 8)):
        in_span, out_span = (2 * 100 + 100) * es, 100 * es
        for out in ("t", "u", "i"):
            for base in (A, B, C_):
                assert ub(dtype=dtype, **{out: base}) == INV
                assert ub(dtype=dtype, **{out: base + in_span - es}) == INV
                assert ub(dtype=dtype, **{out: base - out_span + es}) == INV
                assert b"overlaps" in L.gr4hip_last_error()
        assert ub(dtype=dtype, I=B + es // 2) == INV and ub(dtype=dtype, u=E + es // 2) == INV
    assert ub(n=0) == OK and ub(n=0, U=None, I=None, P=None, t=None, u=None, i=None, in_stride=0) == OK
    assert ub(n=0, dtype=capi.I32) == INV and ub(n=0, np_=1) == INV


def test_python_blocks_refuse_host_tensors_and_bad_shapes(capi):
    torch = pytest.importorskip("torch")
    import gnuradio4_amd as G
    for make in (lambda: G.PowerFactor(0), lambda: G.PowerFactor(17), lambda: G.SystemUnbalance(1), lambda: G.PowerFactor(3, torch.complex64),
                 lambda: G.SystemUnbalance(3, torch.int32)):
        with pytest.raises(capi.Gr4HipError) as e:
            make()
        assert e.value.status == capi.INVALID_ARGUMENT
    x = torch.zeros(3, 8)
    with pytest.raises(capi.Gr4HipError):
        G.PowerFactor(3).process(x, x)
    with pytest.raises(capi.Gr4HipError):
        G.SystemUnbalance(3).process(x, x, x)
    assert G.PowerFactor.tile() == G.SystemUnbalance.tile() == 2048


def test_header_is_defined_behaviour_under_sanitizers(tmp_path):
    """gr4/electrical_ops.hpp over the special-value grid in a stand-alone program built with -fsanitize=address,undefined (no recovery)"""
    from test_host_cpp import ROOT
    exe = tmp_path / "electrical_ops_selftest"
    host = os.path.join(ROOT, "gnuradio4_amd", "host")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(host, "include"),
                           os.path.join(host, "tests", "electrical_ops_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def write_graph_files(d, seed=5):
    """the inputs of test_host_electrical and the oracle's outputs for its four graphs per type (want_<graph>_<type>_<port>.bin); returns {name: array}"""
    rng = np.random.default_rng(seed)
    want = {}
    for dt in EO.FLOATS:
        t = TNAME[np.dtype(dt)]
        x = EO.graph_inputs(dt, rng)
        for k, v in x.items():
            v.tofile(d / f"{k}_{t}.bin")
        pf, ph = EO.power_factor(x["P"], x["S"])
        want[f"pf3_{t}_power_factor"], want[f"pf3_{t}_phase"], want[f"pf1_{t}_power_factor"] = pf.ravel(), ph.ravel(), pf[0]
        want[f"ub3_{t}_P_total"], want[f"ub3_{t}_U_unbalance"], want[f"ub3_{t}_I_unbalance"] = EO.system_unbalance(x["U"], x["I"], x["P"])
        _, want[f"ub2_{t}_U_unbalance"], want[f"ub2_{t}_I_unbalance"] = EO.system_unbalance(x["U"][:2], x["I"][:2], x["P"][:2])
        if t == "f32":  # ub3t: the total power alone connected, the first 256 samples
            want["ub3t_f32_P_total"] = np.ascontiguousarray(want["ub3_f32_P_total"][:256])
    for k, v in want.items():
        v.setflags(write=False)
        v.tofile(d / f"want_{k}.bin")
    return want


def check_graph_files(d, want, phase_bound):
    """what the program wrote, against the oracle once more: the phase within phase_bound[type] ulp, the rest bit for bit; returns the largest phase distances"""
    worst = {}
    for k, w in want.items():
        got = np.fromfile(d / f"{k}.bin", dtype=w.dtype)
        assert got.shape == w.shape, k
        if k.endswith("_phase"):
            t = TNAME[w.dtype]
            worst[t] = float(EO.ulp_distance(got, w).max())
            print(f"{k}: {worst[t]} ulp from the oracle")
            assert worst[t] <= phase_bound[t], (k, worst[t])
        else:
            assert EO.same_bits(got, w), (k, np.nonzero(got.view(f"u{w.itemsize}") != w.view(f"u{w.itemsize}"))[0][:5])
    return worst


def test_host_domain_graphs_equal_the_oracle(tmp_path):
    """gnuradio4_amd/host/tests/test_host_electrical.cpp on compute_domain host: the plugin instantiates the eight registered types, and the mirror blocks' own CPU
    processBulk gives the oracle's values: bit for bit, the phase (std::acos in the sample type) within 2 ulp"""
    from test_host_cpp import BIN, PLUGIN, ROOT
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    want = write_graph_files(tmp_path)
    r = subprocess.run([os.path.join(BIN, "test_host_electrical"), PLUGIN, "host", str(tmp_path), repr(HOST_PHASE_BOUND_ULP), repr(HOST_PHASE_BOUND_ULP)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all checks passed (compute_domain host)" in r.stdout, r.stdout + r.stderr
    print(r.stdout)
    check_graph_files(tmp_path, want, {"f32": HOST_PHASE_BOUND_ULP, "f64": HOST_PHASE_BOUND_ULP})
    assert not list(tmp_path.glob("chain_*.bin"))  # PowerMetrics is device-only: the chain is a device graph


def test_device_domain_fails_loudly_without_gpu(tmp_path):
    """compute_domain gpu:hip:0 without a device: work::Status::ERROR from the seam (exit code 3), never the host body"""
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from test_host_cpp import BIN, PLUGIN, ROOT
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    write_graph_files(tmp_path)
    r = subprocess.run([os.path.join(BIN, "test_host_electrical"), PLUGIN, "gpu:hip:0", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
    assert not list(tmp_path.glob("pf3_*.bin"))
