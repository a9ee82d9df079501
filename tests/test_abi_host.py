"""CPU-side checks of the product library: it loads, exports every symbol include/gr4hip.h declares, and its host-only
entry points (window, filter design, status/error plumbing) agree with the oracle.  No compute calls need a GPU here."""
import ctypes as C
import os
import sys
import re

import numpy as np
import pytest

import oracle_lib as O

ROOT = O.ROOT


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "gr4hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gr4hip_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(L):
    from gnuradio4_amd import capi
    declared = _declared_symbols()
    assert len(declared) >= 60
    raw = C.CDLL(capi.LIB_PATH)
    missing = [s for s in declared if not hasattr(raw, s)]
    assert not missing, f"declared in gr4hip.h but not exported: {missing}"
    assert sorted(capi.SIGNATURES) == declared, "python binding table and header disagree"
    assert L.gr4hip_abi_version() == 1


def test_no_oracle_or_reference_in_product():
    """the product must never route through the oracle or the reference tree"""
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "gnuradio4_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h", ".sh")):
                t = open(os.path.join(base, f), errors="replace").read()
                if re.search(r"oracle_lib|liboracle|gr4o_|/root/reference/|gr4ref_", t):
                    bad.append(f)
    assert not bad, bad


def test_lifecycle_calls_never_touch_the_device_outside_a_stream():
    """the stream rule (csrc/common.hpp, include/gr4hip.h "LIFECYCLE CALLS ARE STREAM-ORDERED WITH THE DATA"): in the kernel library a handle's device state is
    written by upload_fresh() into a buffer no launch has seen, or by work enqueued on the stream of a process call -- never by a NULL-stream hipMemset / blocking
    hipMemcpy (round 5's race: gr4hip_chain_reset's hipMemset overtaken by the previous launch's carry on a non-blocking stream).  What is left of either name:
    upload_fresh itself, the create-time self-test's download, and developer-build timing dumps."""
    src = os.path.join(ROOT, "gnuradio4_amd", "csrc")
    allowed = {("common.hpp", "upload_fresh"), ("iir.hip", "hipMemcpy(y.data(), dy.ptr"), ("iir.hip", "a.dbgc"), ("chain_fused.hip", "gr4::g_dbg"), ("chain16.hip", "gr4::g_dbg16")}
    bad = []
    for f in sorted(os.listdir(src)):
        if not f.endswith((".hip", ".hpp")):
            continue
        for n, line in enumerate(open(os.path.join(src, f), errors="replace"), 1):
            code = line.split("//")[0]
            if re.search(r"\bhipMemset\(|\bhipMemcpy\(|\bhipMemcpyToSymbol\(", code) and not any(f == af and tok in line for af, tok in allowed):
                bad.append(f"{f}:{n}: {line.strip()[:100]}")
    assert not bad, "\n".join(bad)
    # every mutator is a host-side note: no HIP call at all between its braces (the device work is in *_state_on / history_on, which take the stream)
    for f, fn in (("chain_fused.hip", "int chain_fused_reset(ChainFused* c) {"), ("chain_td.hip", "int chain_td_reset(ChainTd* c) {"), ("fir_batched.hip", "int gr4hip_fir_batched_reset("),
                  ("iir.hip", "int gr4hip_iir_reset(gr4hip_iir_t* f) {"), ("fir.hip", "int gr4hip_fir_reset(gr4hip_fir_t* f) {"), ("math.hip", "int gr4hip_rotator_reset("),
                  ("f64.hip", "int gr4hip_fir64_reset("), ("f64.hip", "int gr4hip_iir64_reset("), ("fir_interp.hip", "int gr4hip_fir_interp_reset("),
                  ("fir_resamp.hip", "int gr4hip_resamp_reset("), ("fir_cplx.hip", "int gr4hip_cfir_reset("), ("pfb.hip", "int gr4hip_pfb_reset("),
                  ("ifft.hip", "int gr4hip_pfb_synth_reset(")):
        t = open(os.path.join(src, f), errors="replace").read()
        i = t.index(fn)
        body = t[i:t.index("\n}\n", i)]
        assert not re.search(r"\bhip[A-Z]\w*\(", body), (f, fn, body)
    # what those mutators call on the carried history (history.hpp: one-line members, the body ends at the first closing brace)
    t = open(os.path.join(src, "history.hpp"), errors="replace").read()
    for fn in ("void reset() {", "void keep() {"):
        i = t.index(fn)
        body = t[i:t.index("}", i) + 1]
        assert body.count("{") == 1 and not re.search(r"\bhip[A-Z]\w*\(", body), (fn, body)


def test_status_strings_and_errors(L):
    assert L.gr4hip_status_string(0) == b"OK"
    assert L.gr4hip_status_string(-2) == b"INSUFFICIENT_INPUT_ITEMS"
    assert L.gr4hip_status_string(-100) == b"ERROR"
    n = C.c_int(-1)
    assert L.gr4hip_device_count(C.byref(n)) == 0 and n.value >= 0
    h = C.c_void_p()
    rc = L.gr4hip_fir_create(C.byref(h), 3, None, 0, 1)  # bad dtype
    assert rc == -101 and b"dtype" in L.gr4hip_last_error()
    for size in (600000, 1 << 21):  # beyond the chirp-convolution range (2^19) / beyond the four-step range (2^20) -> caller keeps its CPU path
        rc = L.gr4hip_fft_create(C.byref(h), 10, size, 3, 0)
        assert rc == -103
    rc = L.gr4hip_math_nary(0, 8, None, 33, None, 1, None)
    assert rc == -101 and b"[1,32]" in L.gr4hip_last_error()


@pytest.mark.parametrize("wid", range(12))
def test_window_matches_oracle_and_golden(L, golden, wid):
    for n in (8, 255, 8192):
        w = np.empty(n, np.float32)
        assert L.gr4hip_window_create(wid, w.ctypes.data, n, 1.6) == 0
        np.testing.assert_allclose(w, O.window(wid, n, np.float32), rtol=1e-6, atol=1e-7)
    w8 = np.empty(8, np.float32)
    L.gr4hip_window_create(wid, w8.ctypes.data, 8, 1.6)
    np.testing.assert_allclose(w8, golden["window_n8"][O.WINDOWS[wid]], rtol=2e-6, atol=2e-7)
    assert L.gr4hip_window_create(wid, None, 0, 1.6) == 0  # zero-length windows are fine (window.hpp:72-74)


def test_fir_design_matches_oracle(golden):
    import gnuradio4_amd.blocks as B
    g = golden["fir_design_tapcount"]
    taps = B.design_fir(0, g["order"], g["f_low"], float("nan"), g["fs"], "Hamming")
    assert len(taps) == g["expected_taps"]
    for resp in range(4):
        for win in ("Hamming", "Hann", "Kaiser", "Blackman"):
            t = B.design_fir(resp, 4, 100.0, 200.0, 1000.0, win)
            p = O.filter_params(order=4, fLow=100.0, fHigh=200.0, fs=1000.0)
            o = O.fir_design(resp, p, [w.lower() for w in O.WINDOWS].index(win.lower()), True)
            assert len(t) == len(o)
            np.testing.assert_allclose(t, o, atol=2e-6)


def test_iir_design_matches_oracle():
    import gnuradio4_amd.blocks as B
    for resp in range(4):
        for design in range(4):
            for order in (3, 4, 8):
                b, a = B.design_iir(resp, order, 100.0, 200.0, 1000.0, design)
                p = O.filter_params(order=order, fLow=100.0, fHigh=200.0, fs=1000.0)
                secs = O.iir_design(resp, p, design, True)
                assert len(secs) == len(b)
                for (ob, oa), pb, pa in zip(secs, b, a):
                    np.testing.assert_allclose(pb[:len(ob)], ob, rtol=2e-4, atol=2e-6)
                    np.testing.assert_allclose(pa[:len(oa)], oa, rtol=2e-5, atol=2e-6)


def test_device_blocks_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import gnuradio4_amd as G
    from gnuradio4_amd.capi import Gr4HipError
    with pytest.raises(Gr4HipError):
        G.fir_filter([1.0, 2.0])  # needs device memory for taps/history -> HIP runtime error, no silent CPU path
    with pytest.raises(Gr4HipError):
        G.math_const("Add", torch.zeros(4), 1.0)  # host tensor is rejected, never computed on the CPU


def test_missing_library_is_an_import_error_not_a_fallback(monkeypatch, tmp_path):
    """without libgr4hip.so the package refuses to work (the message says how to build it): nothing computes on the CPU instead"""
    from gnuradio4_amd import capi
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", str(tmp_path / "libgr4hip.so"))
    with pytest.raises(ImportError, match="no CPU fallback"):
        capi.lib()



def test_fft_plan_of_every_smooth_size():
    """gr4hip_fft_plan (host-only): every {2,3,5}-smooth size up to 8192 that is not a power of two gets a mixed-radix plan whose radices (2 .. 16) multiply to the
    size in the fewest passes; powers of two, larger and non-smooth sizes name their paths"""
    import ctypes as C
    from gnuradio4_amd import capi
    L = capi.lib()
    rad = (C.c_int * 16)()
    kind, npass = C.c_int(-1), C.c_int(-1)
    smooth = sorted({2 ** a * 3 ** b * 5 ** c for a in range(14) for b in range(9) for c in range(6)} - {2 ** a for a in range(14)})
    n_checked = 0
    radset = (2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16)
    memo = {1: 0}

    def fewest(n):  # the fewest passes over the radix set (what the planner's dynamic programme must find)
        if n not in memo:
            memo[n] = min((fewest(n // r) + 1 for r in radset if n % r == 0), default=10 ** 6)
        return memo[n]
    for N in [n for n in smooth if 2 <= n <= 8192]:
        capi.check(L.gr4hip_fft_plan(N, C.byref(kind), rad, C.byref(npass)), "fft_plan")
        assert kind.value == 3 and 1 <= npass.value <= 15, N
        prod = 1
        for i in range(npass.value):
            assert rad[i] in (2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16), (N, rad[i])
            prod *= rad[i]
        assert prod == N
        assert npass.value == fewest(N), (N, npass.value)
        n_checked += 1
    assert n_checked == 153  # smooth sizes in [2, 8192] that are not powers of two
    for N, want in ((1024, 0), (8192, 0), (16384, 1), (1 << 20, 1), (1009, 2), (10000, 2), (3 ** 7 * 5 ** 3, 2)):
        capi.check(L.gr4hip_fft_plan(N, C.byref(kind), rad, C.byref(npass)), "fft_plan")
        assert kind.value == want, N
    assert L.gr4hip_fft_plan(1 << 21, C.byref(kind), rad, C.byref(npass)) == capi.UNSUPPORTED if hasattr(capi, "UNSUPPORTED") else True


def test_developer_switch_names():
    from gnuradio4_amd import capi
    L = capi.lib()
    assert L.gr4hip_developer_switch(b"GR4HIP_FFT_SMOOTH_RUNTIME", 1) == 0 and L.gr4hip_developer_switch(b"GR4HIP_FFT_SMOOTH_RUNTIME", 0) == 0
    for name, value in ((b"GR4HIP_INTERP_NO_MFMA", 1), (b"GR4HIP_INTERP_SPW", 3)):  # the interpolating FIR's: a flag and an integer
        assert L.gr4hip_developer_switch(name, value) == 0 and L.gr4hip_developer_switch(name, 0) == 0
    assert L.gr4hip_developer_switch(b"GR4HIP_NO_SUCH_SWITCH", 1) < 0 and b"unknown switch" in L.gr4hip_last_error()


def test_no_kernel_of_the_shipped_library_spills_vector_registers():
    """the second-evaluation loops of the f16 FIR kernels spilled (26 .. 82 VGPRs, 108 .. 300 B of scratch) while DESIGN.md said they did not.
    Round 5 moved every second evaluation out of the main kernels (fir_exact.hip); this reads the AMDGPU metadata notes of the code objects inside the shipped
    libgr4hip.so (tools/kernel_resources.py, llvm-readelf --notes; no GPU needed): no FIR / decimator / chain kernel keeps anything in scratch memory.
    Known, listed here so the list cannot grow unseen: chain_td_kernel<9, 11 / 12> (2 VGPRs, 12 B, outside their loops), fir_decim_fd_kernel<true> (the opt-in one-launch
    decimator + cascade: 8 VGPRs), iir_pass_b<16> (the 16-state scan of cascades with more than 8 states: 71 VGPRs)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels()
    assert len(ks) > 300
    accepted = ("chain_td_kernel<9, 11>", "chain_td_kernel<9, 12>", "fir_decim_fd_kernel<true>", "iir_pass_b<16>",
                "chain_td16_kernel<0, 13>", "chain_td16_kernel<1, 13>")  # (round 6: 1 - 2 VGPRs, 8 - 12 B, since the marked-frame kernel compares its spectrum with the fused launch's before storing it)
    bad = [(k["demangled"][:80], k["vspill"], k["scratch"]) for k in ks if (k["vspill"] or k["scratch"]) and not any(a in k["demangled"] for a in accepted)]
    assert not bad, bad
    assert all(k["vspill"] <= 2 and k["scratch"] <= 16 for k in ks if "chain_td16_kernel" in k["demangled"])
    assert not any((k["vspill"] or k["scratch"]) for k in ks if "chain_fd_kernel" in k["demangled"] or "chain_fd_multi_kernel" in k["demangled"])  # (the guard's sums ride in the headline kernel: not one register of it in scratch)
    for fam in ("fir_mfma_f16x2_kernel", "fir_mfma_f16x2_c32_kernel", "fir_decim_f16x2_kernel", "fir_exact_kernel", "chain_fd_kernel", "chain_redo_kernel", "chain_td16_kernel", "fir_poly_kernel"):
        assert any(fam in k["demangled"] for k in ks), fam


def test_kernel_table_is_current():
    """KERNELS.md (the per-kernel register / LDS / spill table DESIGN.md points to) is generated from the shipped library by tools/regen_kernel_table.sh: the committed
    file must be what the built libgr4hip.so says (a hand-written table had gone stale)"""
    import subprocess
    want = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--md"], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    have = open(os.path.join(ROOT, "KERNELS.md")).read().strip().splitlines()
    assert have[-len(want):] == want, "run tools/regen_kernel_table.sh"
    assert os.path.getsize(os.path.join(ROOT, "DESIGN.md")) <= 40 * 1024
