"""CPU-side checks of the converter entry points (include/gr4hip.h "Type converters"): gr4hip_convert_params_check against the requires clauses of
ConverterBlocks.hpp for every kind / dtype pair, the defaults, the tile, and the refusal to create a handle without a device."""
import ctypes as C

import numpy as np
import pytest

import converter_oracle as CO

NP_OF_ID = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64, np.complex64, np.complex128]


@pytest.fixture(scope="module")
def capi():
    from gnuradio4_amd import capi
    capi.lib()
    return capi


def test_kind_names_follow_the_header(capi):
    assert capi.CONVERT_KINDS == CO.KINDS


def test_params_check_admits_exactly_the_reference_pairs(capi):
    L = capi.lib()
    n_ok = 0
    for k, kind in enumerate(CO.KINDS):
        ok = {(NP_OF_ID.index(t.type), NP_OF_ID.index(r.type)) for t, r in CO.accepted_pairs(kind)}
        for i in range(-1, 15):  # the 12 sample types, the two UncertainValue ids and two numbers that are no dtype
            for o in range(-1, 15):
                p = capi.ConvertParams(k, i, o, 1.0)
                rc = L.gr4hip_convert_params_check(C.byref(p))
                assert rc == (capi.OK if (i, o) in ok else capi.INVALID_ARGUMENT), (kind, i, o, rc)
                assert (L.gr4hip_convert_tile(C.byref(p)) > 0) == ((i, o) in ok)
                n_ok += rc == capi.OK
    assert n_ok == 100 + 100 + 12 + 2 * 9 + 8 + 8
    for k in (-1, 14, 1000):
        assert L.gr4hip_convert_params_check(C.byref(capi.ConvertParams(k, capi.F32, capi.F32, 1.0))) == capi.INVALID_ARGUMENT
    assert L.gr4hip_convert_params_check(None) == capi.INVALID_ARGUMENT and L.gr4hip_convert_tile(None) == 0


def test_params_default_gives_the_blocks_result_type(capi):
    L = capi.lib()
    for k, kind in enumerate(CO.KINDS):
        for t, r in CO.accepted_pairs(kind):
            p = capi.ConvertParams()
            assert L.gr4hip_convert_params_default(C.byref(p), k, NP_OF_ID.index(t.type)) == capi.OK
            assert p.kind == k and p.in_dtype == NP_OF_ID.index(t.type) and p.scale == 1.0
            if kind not in ("Convert", "ScalingConvert", "ComplexToInterleaved", "InterleavedToComplex"):
                assert p.out_dtype == NP_OF_ID.index(r.type), (kind, t)
                assert L.gr4hip_convert_params_check(C.byref(p)) == capi.OK


def test_tile_is_the_wider_port_at_sixteen_bytes_per_lane(capi):
    """256 lanes x L items x the vectors a lane holds, L = 16 bytes / the wider port's item: 1 B -> 8 B moves two items per lane and access"""
    L = capi.lib()

    def tile(kind, i, o):
        return L.gr4hip_convert_tile(C.byref(capi.ConvertParams(capi.CONVERT_KINDS.index(kind), i, o, 1.0)))
    assert tile("Convert", capi.U8, capi.F64) == tile("Convert", capi.F64, capi.I8) == 256 * 2 * 4
    assert tile("Convert", capi.U8, capi.I8) == 256 * 16
    assert tile("InterleavedToComplex", capi.I16, capi.C32) == 256 * 2 * 4  # items are complex samples
    assert tile("ToMagPhase", capi.C64, capi.F64) == 256  # a transcendental per item: one vector per lane
    assert tile("ComplexToInterleaved", capi.C64, capi.I8) == 256 * 4


def test_create_without_a_device_is_no_device(capi):
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = capi.lib()
    h = C.c_void_p()
    p = capi.ConvertParams(capi.CONVERT_KINDS.index("Abs"), capi.C32, capi.F32, 1.0)
    assert L.gr4hip_convert_create(C.byref(h), C.byref(p)) == capi.NO_DEVICE and not h.value
    assert b"no HIP device" in L.gr4hip_last_error()
    bad = capi.ConvertParams(capi.CONVERT_KINDS.index("Abs"), capi.C32, capi.C32, 1.0)
    assert L.gr4hip_convert_create(C.byref(h), C.byref(bad)) == capi.INVALID_ARGUMENT  # the check comes first
    import gnuradio4_amd as G
    with pytest.raises(capi.Gr4HipError) as e:
        G.Abs(torch.complex64)
    assert e.value.status == capi.NO_DEVICE


# ---- the host mirror blocks (gr4/blocks.hpp) against the oracle
TNAME = {np.dtype(t): n for t, n in zip(NP_OF_ID, ["u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64", "f32", "f64", "c32", "c64"])}
PORTS = {"Convert": ["out"], "ScalingConvert": ["out"], "Abs": ["abs"], "Real": ["real"], "Imag": ["imag"], "Arg": ["arg"], "RadiansToDegree": ["deg"], "DegreeToRadians": ["rad"],
         "ToRealImag": ["real", "imag"], "RealImagToComplex": ["out"], "ToMagPhase": ["mag", "phase"], "MagPhaseToComplex": ["out"], "ComplexToInterleaved": ["interleaved"],
         "InterleavedToComplex": ["out"]}
HOST_SCALE = 3.0
# The host blocks evaluate the transcendental kinds with the C library in the sample type (hypotf, atan2f, cosf / sinf for float), the oracle in float64 rounded
# once.  Largest distance measured on these inputs with glibc 2.39 on x86-64, per kind and sample type, in ulp of the sample type.  The bound is 2 ulp for every
# one of them: twice the largest measured distance, and for double what two libraries that are each within 1 ulp of the true value can differ by (numpy takes its
# float64 sine and cosine from a vector library on some processors).  The float product r * cosf(theta) rounds twice in float: the reference's arithmetic.
HOST_MEASURED_ULP = {("Abs", "f32"): 0, ("Abs", "f64"): 0, ("Arg", "f32"): 1, ("Arg", "f64"): 1, ("ToMagPhase", "f32"): 1, ("ToMagPhase", "f64"): 1,
                     ("MagPhaseToComplex", "f32"): 1, ("MagPhaseToComplex", "f64"): 0}
HOST_BOUND_ULP = 2.0


def write_inputs(d):
    """the two input streams of every sample type as <d>/in0_<type>.bin, in1_<type>.bin (what test_host_converter reads); returns them, read-only"""
    rng = np.random.default_rng(11)
    inputs = {}
    for dt in NP_OF_ID:
        a = CO.special_values(dt, rng, 300)
        a = a[:a.size - a.size % 2]
        b = rng.permutation(a)
        for v in (a, b):
            v.setflags(write=False)
        a.tofile(d / f"in0_{TNAME[np.dtype(dt)]}.bin")
        b.tofile(d / f"in1_{TNAME[np.dtype(dt)]}.bin")
        inputs[np.dtype(dt)] = (a, b)
    return inputs


GRAPH_CASES = [("Convert", np.float32, np.int16), ("ScalingConvert", np.uint8, np.float32), ("Abs", np.complex64, np.float32), ("Real", np.complex64, np.float32),
               ("Imag", np.complex64, np.float32), ("Arg", np.complex64, np.float32), ("RadiansToDegree", np.float32, np.float32), ("DegreeToRadians", np.float64, np.float64),
               ("ToRealImag", np.complex64, np.float32), ("RealImagToComplex", np.float32, np.complex64), ("ToMagPhase", np.complex64, np.float32),
               ("MagPhaseToComplex", np.float32, np.complex64), ("ComplexToInterleaved", np.complex64, np.int16), ("InterleavedToComplex", np.int16, np.complex64)]


def test_device_domain_fails_loudly_without_gpu(tmp_path):
    """compute_domain gpu:hip:0 on a converter block without a device: work::Status::ERROR from the seam (exit code 3), never the host body"""
    import os
    import subprocess
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from test_host_cpp import BIN, PLUGIN, ROOT
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    write_inputs(tmp_path)
    r = subprocess.run([os.path.join(BIN, "test_host_converter"), "--device", str(tmp_path), PLUGIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
    assert not list(tmp_path.glob("dev_*.bin"))


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    """the inputs (shared, unchanged) and the files test_host_converter wrote for them"""
    import os
    import subprocess
    from test_host_cpp import BIN, ROOT
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("converter")
    inputs = write_inputs(d)
    r = subprocess.run([os.path.join(BIN, "test_host_converter"), str(d), repr(HOST_SCALE)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "246 converter blocks, 14 graphs, 0 failed" in r.stdout, r.stdout
    return d, inputs


def _same_bits(a, b):
    if a.dtype.kind in "fc":
        f = CO.base_of(a.dtype)
        a, b = a.view(f), b.view(f)
        u = np.dtype(f"u{f.itemsize}")
        return a.shape == b.shape and bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))
    return np.array_equal(a, b)


@pytest.mark.parametrize("kind", CO.KINDS)
def test_host_blocks_equal_the_oracle(host_run, kind):
    """every registered type pair: bit for bit (two NaNs are equal whatever their payload); the four transcendental kinds within their measured bound"""
    d, inputs = host_run
    for t, r in CO.accepted_pairs(kind):
        x = inputs[t][:2 if kind in ("RealImagToComplex", "MagPhaseToComplex") else 1]
        want = CO.run(kind, x, r, HOST_SCALE)
        for port, w in zip(PORTS[kind], want):
            got = np.fromfile(d / f"{kind}_{TNAME[t]}_{TNAME[r]}_{port}.bin", dtype=w.dtype)
            assert got.shape == w.shape, (kind, t, r, port)
            if CO.is_transcendental(kind, t):
                f = CO.base_of(w.dtype)
                dist = float(CO.ulp_distance(got.view(f), w.view(f)).max())
                m = HOST_MEASURED_ULP[(kind, TNAME[CO.base_of(t)])]
                print(f"host {kind}<{TNAME[t]}> {port}: {dist} ulp from the oracle")
                assert 2 * m <= HOST_BOUND_ULP and dist <= HOST_BOUND_ULP, (kind, t, port, dist, m)
            else:
                assert _same_bits(got, w), (kind, t, r, port, np.nonzero(got != w)[0][:5])


def test_host_graphs_equal_the_direct_calls(host_run):
    """the blocks in a graph, ports under the reference's names, both Resampling kinds included: the work loop hands every block what processOne / processBulk got"""
    d, _ = host_run
    graphs = sorted(p.name for p in d.glob("graph_*.bin"))
    assert len(graphs) == 14 + 2 and {g.split("_")[1] for g in graphs} == set(CO.KINDS)
    for g in graphs:
        a, b = (d / g).read_bytes(), (d / g[len("graph_"):]).read_bytes()
        assert len(a) > 0 and a == b, g


def test_helpers_are_defined_behaviour_under_sanitizers(tmp_path):
    """gr4/converter_ops.hpp on every type pair's edge cases in a stand-alone program built with -fsanitize=address,undefined (no recovery): float -> integer out of
    range, NaN, signed overflow of the product and of abs are all defined here"""
    import os
    import subprocess
    from test_host_cpp import ROOT
    exe = tmp_path / "converter_ops_selftest"
    host = os.path.join(ROOT, "gnuradio4_amd", "host")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(host, "include"),
                           os.path.join(host, "tests", "converter_ops_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_converter_mutators_are_host_side_notes():
    """the stream rule for this handle (include/gr4hip.h): set_scale / set_prologue / set_epilogue / reset make no HIP call at all -- a replaced program's device copy
    is retired and freed by the next process call or with the handle"""
    import os
    import re
    from test_host_cpp import ROOT
    src = open(os.path.join(ROOT, "gnuradio4_amd", "csrc", "convert.hip")).read()
    for fn in ("static int set_hook(gr4hip_convert* h,", "int gr4hip_convert_set_scale(", "int gr4hip_convert_reset("):
        i = src.index(fn)
        body = src[i:src.index("\n}\n", i)]
        assert not re.search(r"\bhip[A-Z]\w*\(|\bdelete\b", body), (fn, body)
    assert "retired.push_back(slot)" in src
