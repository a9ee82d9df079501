"""SchmittTrigger on the host side: gr4hip_schmitt_check's validation (the same as create's, before any device work), the exported symbols and segment length,
the plugin's twelve registered names with the reference's members (gnuradio4_amd/host/tests/test_host_schmitt_trigger.cpp), the loud failure of the
device-only block without a GPU and in the host domain, and -- on the GPU -- the C++ block in a graph source -> trigger -> tag-recording sink against the oracle."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import schmitt_trigger_oracle as ST

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_schmitt_trigger")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")


@pytest.fixture(scope="module")
def L():
    from gnuradio4_amd import capi
    return capi.lib()


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    return BIN


def _params(L, **kw):
    from gnuradio4_amd import capi
    p = capi.SchmittParams()
    assert L.gr4hip_schmitt_params_default(C.byref(p)) == 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults_are_the_detectors(L):
    from gnuradio4_amd import capi
    p = _params(L)
    assert (p.offset, p.threshold, p.method, p.dtype) == (0.0, 1.0, capi.SCHMITT_NO_INTERPOLATION, capi.F32)  # SchmittTrigger.hpp:45-46
    assert L.gr4hip_schmitt_check(C.byref(p)) == 0
    for dtype in (capi.I16, capi.I32, capi.F32, capi.F64):
        for method in range(3):
            assert L.gr4hip_schmitt_check(C.byref(_params(L, dtype=dtype, method=method, offset=5.0, threshold=0.0))) == 0
    assert L.gr4hip_schmitt_check(C.byref(_params(L, dtype=capi.I16, offset=32000.0, threshold=767.0))) == 0
    assert L.gr4hip_schmitt_check(C.byref(_params(L, dtype=capi.I16, offset=-32000.0, threshold=768.0))) == 0


@pytest.mark.parametrize("kw", [dict(threshold=-1.0), dict(threshold=-0.0001), dict(threshold=math.nan), dict(threshold=math.inf), dict(offset=math.nan),
                                dict(offset=-math.inf), dict(method=4), dict(method=-1), dict(dtype=0), dict(dtype=7), dict(dtype=10), dict(dtype=99),
                                dict(dtype=5, offset=32000.0, threshold=768.0), dict(dtype=5, offset=-32000.0, threshold=769.0), dict(dtype=5, offset=40000.0, threshold=0.0),
                                dict(dtype=5, offset=0.5), dict(dtype=5, threshold=1.5), dict(dtype=6, offset=2147483647.0, threshold=1.0),
                                dict(dtype=6, offset=-2147483648.0, threshold=1.0), dict(dtype=8, offset=1e39), dict(dtype=8, threshold=1e39)])
def test_every_rejection_before_device_work(L, kw):
    from gnuradio4_amd import capi
    p = _params(L, **kw)
    assert L.gr4hip_schmitt_check(C.byref(p)) == capi.INVALID_ARGUMENT, kw
    h = C.c_void_p()
    assert L.gr4hip_schmitt_create(C.byref(h), C.byref(p)) == capi.INVALID_ARGUMENT and not h.value
    assert L.gr4hip_schmitt_check(None) == capi.INVALID_ARGUMENT


def test_the_polynomial_method_is_unsupported_not_replaced(L):
    from gnuradio4_amd import capi
    for dtype in (capi.I16, capi.I32, capi.F32, capi.F64):
        p = _params(L, method=capi.SCHMITT_POLYNOMIAL_INTERPOLATION, dtype=dtype)
        assert L.gr4hip_schmitt_check(C.byref(p)) == capi.UNSUPPORTED
        h = C.c_void_p()
        assert L.gr4hip_schmitt_create(C.byref(h), C.byref(p)) == capi.UNSUPPORTED and not h.value
        assert "Savitzky-Golay" in L.gr4hip_last_error().decode()


def test_symbols_and_segment(L):
    import gnuradio4_amd as G
    from gnuradio4_amd import capi
    for name in ("params_default", "check", "segment", "create", "set_params", "reset", "process", "destroy"):
        assert hasattr(L, f"gr4hip_schmitt_{name}")
    seg = G.SchmittTrigger.segment()
    assert seg == int(L.gr4hip_schmitt_segment()) and seg >= 1024 and seg % 16 == 0
    hdr = open(os.path.join(ROOT, "include", "gr4hip.h")).read()
    assert f"#define GR4HIP_SCHMITT_SEGMENT {seg} " in hdr
    assert capi.SCHMITT_EDGE_BYTES == 24 and "} gr4hip_schmitt_edge;" in hdr
    assert G.SchmittTrigger.METHODS == ("NO_INTERPOLATION", "BASIC_LINEAR_INTERPOLATION", "LINEAR_INTERPOLATION", "POLYNOMIAL_INTERPOLATION")


def test_plugin_makes_the_twelve_types_with_the_references_members(prog):
    r = subprocess.run([prog, PLUGIN, "host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed (compute_domain host)" in r.stdout


# ------------------------------------------------------------------------------------------------ the graphs
N, FS, T0, MARK = 1000, 1000.0, 1000000, 300
OFFSET, THRESHOLD = 0.1, 0.3


def _signal():
    """ten periods of a sine of 100 samples plus a little noise; the edges are detected near samples 27 and 74 of every period, so with calls of 50 samples no
    edge's position (a few samples in front of it) falls in front of its call"""
    rng = np.random.default_rng(3)
    return (np.sin(2 * np.pi * (np.arange(N) - 20) / 100.0) + 0.005 * rng.standard_normal(N)).astype(np.float32)


def _expected_tags(method, falling=True, forward=True, max_chunk=None):
    """the oracle's edges as the block publishes them (gr4/blocks.hpp): at sample + edge_idx, trigger_offset = (edge_idx + edge_offset) period in float,
    trigger_time = now(sample) - int64(trigger_offset) with now(sample) = trigger_time + (sample + 1) period.  With calls of at most max_chunk samples an edge
    whose position lies max_chunk or more samples in front of its detecting sample lies in front of its call, wherever the calls are cut: it is dropped.
    Returns the tags and the number of dropped edges."""
    e = ST.SchmittTrigger(OFFSET, THRESHOLD, method, np.float32).process(_signal())
    assert e["count"] == 20 and np.all(e["flags"] == 0)
    period = np.float32(int(np.float32(1e6) / np.float32(FS)))
    tags = {MARK: {"gr:marker": "7"}} if forward else {}
    dropped = 0
    for k in range(e["count"]):
        if e["kind"][k] == ST.FALLING and not falling:
            continue
        if max_chunk is not None:
            assert e["edge_idx"][k] <= -max_chunk or e["edge_idx"][k] == 0, "an edge whose fate depends on where the calls are cut"
            if e["edge_idx"][k] <= -max_chunk:
                dropped += 1
                continue
        rel = (np.float32(e["edge_idx"][k]) + e["edge_offset"][k]) * period
        now = T0 + (int(e["sample"][k]) + 1) * int(period)
        pos = int(e["sample"][k] + e["edge_idx"][k])
        assert pos not in tags
        tags[pos] = {"gr:trigger_name": "RISING" if e["kind"][k] == ST.RISING else "FALLING", "gr:trigger_time": str(now - int(rel)), "gr:trigger_time_error": "0",
                     "gr:trigger_offset": rel, "gr:context": "ctx"}
    return tags, dropped


def _read_tags(path):
    tags = {}
    for line in open(path).read().splitlines():
        idx, *kv = line.split("\t")
        tags[int(idx)] = dict(item.split("=", 1) for item in kv)
        if "gr:trigger_offset" in tags[int(idx)]:
            tags[int(idx)]["gr:trigger_offset"] = np.float32(tags[int(idx)]["gr:trigger_offset"])
    return tags


def test_host_domain_fails_loudly(prog, tmp_path):
    _signal().tofile(tmp_path / "x.f32")
    r = subprocess.run([prog, PLUGIN, "host", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
    assert "device-only" in r.stderr


def test_device_block_fails_loudly_without_gpu(prog, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _signal().tofile(tmp_path / "x.f32")
    r = subprocess.run([prog, PLUGIN, "gpu:hip:0", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_graphs_on_the_device(prog, tmp_path):
    """source -> SchmittTrigger<float32> -> sink on gpu:hip:0 as a fresh child process: tag positions, names, trigger_time and trigger_offset against the oracle for
    the three methods, the samples passed through bit for bit, the same tags from one large chunk and from calls of 50 samples, no FALLING tags with an empty
    trigger_name_falling_edge, the source's own tag forwarded, and not with forward_tag off; with calls of 2 samples every interpolated edge position lies in
    front of its call: those edges are dropped and counted"""
    x = _signal()
    x.tofile(tmp_path / "x.f32")
    r = subprocess.run([prog, PLUGIN, "gpu:hip:0", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "threshold by settings in mid-stream:" in r.stdout and "those of a detector started there: yes" in r.stdout  # set_params on the live handle resets it
    calls = {line.split(":")[0]: int(line.split(" tags, ")[1].split(" device calls")[0]) for line in r.stdout.splitlines() if " device calls" in line}
    drops = {line.split(":")[0]: int(line.split(" device calls, ")[1].split(" dropped edges")[0]) for line in r.stdout.splitlines() if " dropped edges" in line}
    for graph, method, kw in (("no", ST.NO_INTERPOLATION, {}), ("basic", ST.BASIC_LINEAR_INTERPOLATION, {}), ("linear", ST.LINEAR_INTERPOLATION, {}),
                              ("small", ST.LINEAR_INTERPOLATION, {}), ("nofall", ST.LINEAR_INTERPOLATION, {"falling": False}),
                              ("nofwd", ST.LINEAR_INTERPOLATION, {"forward": False}), ("cut", ST.LINEAR_INTERPOLATION, {"max_chunk": 2})):
        y = np.fromfile(tmp_path / f"{graph}.f32", np.float32)
        assert np.array_equal(y.view(np.int32), x.view(np.int32)), graph
        got, (want, dropped) = _read_tags(tmp_path / f"{graph}.tags"), _expected_tags(method, **kw)
        assert got == want, (graph, got, want)
        assert drops[graph] == dropped, (graph, drops[graph], dropped)
    assert calls["small"] >= N // 50 > calls["linear"] and calls["cut"] >= N // 2
    want, _ = _expected_tags(ST.LINEAR_INTERPOLATION, falling=False)
    assert all(t.get("gr:trigger_name", "RISING") == "RISING" for t in want.values()) and len(want) == 11
    want, dropped = _expected_tags(ST.LINEAR_INTERPOLATION, max_chunk=2)
    assert dropped == 20 and want == {MARK: {"gr:marker": "7"}}, "every edge of the cut graph is an interpolated one in front of its call"
    assert MARK not in _expected_tags(ST.LINEAR_INTERPOLATION, forward=False)[0]
