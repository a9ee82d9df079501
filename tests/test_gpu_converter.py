"""The device type-converter blocks (gnuradio4_amd/csrc/convert.hip, G.Convert ... G.InterleavedToComplex) against tests/converter_oracle.py: every kind and type
pair, the lengths around a workgroup's tile, any element alignment, unconnected outputs, absorbed neighbours (hooks), independence of the cutting into calls,
refusals and two streams.

Comparison is bit for bit (two NaNs compare equal whatever their sign and payload: IEEE 754 leaves both to the implementation), except for the four transcendental
kinds, which are held to a distance in units in the last place from the float64 oracle:
  float samples   1 ulp of float32: the device evaluates in float64 on the float arguments and rounds once (0.5), the oracle is float64 rounded once (0.5); the
                  float64 evaluations' own errors are 2^-29 of that.
  double samples  twice the largest distance measured between the device and the numpy (glibc) oracle on THESE inputs at the first run on an MI355X (below:
                  F64_MEASURED_ULP); glibc is itself up to 1 ulp from the true value and the inputs are a finite sample."""
import ctypes as C
import itertools

import numpy as np
import pytest

import converter_oracle as CO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# largest |device - oracle| in ulp of float64 over the inputs of this file, first run on an MI355X (CONVERTERS.md); the bound is twice that
F64_MEASURED_ULP = {"Abs": 1.0, "Arg": 1.0, "ToMagPhase": 1.0, "MagPhaseToComplex": 2.0}
F32_BOUND_ULP = 1.0


def G():
    import gnuradio4_amd
    return gnuradio4_amd


def tdtype(np_dtype):
    return torch.from_numpy(np.zeros(1, np_dtype)).dtype


def make(kind, in_dtype, out_dtype=None, scale=1.0):
    g = G()
    if kind == "ScalingConvert":
        return g.ScalingConvert(tdtype(in_dtype), tdtype(out_dtype), scale)
    if kind in ("Convert", "ComplexToInterleaved", "InterleavedToComplex"):
        return getattr(g, kind)(tdtype(in_dtype), tdtype(out_dtype))
    return getattr(g, kind)(tdtype(in_dtype))


def device(kind, inputs, out_dtype=None, scale=1.0, conv=None):
    conv = conv or make(kind, inputs[0].dtype, out_dtype, scale)
    got = conv.process_bulk(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in inputs])
    got = got if isinstance(got, tuple) else (got,)
    return tuple(t.cpu().numpy() for t in got)


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind in "fc":
        f = CO.base_of(a.dtype)
        a, b = a.view(f), b.view(f)
        u = np.dtype(f"u{f.itemsize}")
        return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def ulp_bound(kind, in_dtype):
    if CO.base_of(in_dtype) == np.float32:
        return F32_BOUND_ULP
    m = F64_MEASURED_ULP[kind]
    return None if m is None else 2.0 * m


_measured = {}


def compare(kind, in_dtype, got, want, what=""):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (kind, in_dtype, q, g.dtype, w.dtype, g.shape, w.shape)
        if CO.is_transcendental(kind, in_dtype):
            f = CO.base_of(g.dtype)
            d = float(CO.ulp_distance(g.view(f), w.view(f)).max()) if g.size else 0.0
            key = (kind, str(CO.base_of(in_dtype)))
            _measured[key] = max(_measured.get(key, 0.0), d)
            print(f"{what}{kind}<{np.dtype(in_dtype)}> port {q}: max distance {d} ulp (largest so far {_measured[key]})")
            bound = ulp_bound(kind, in_dtype)
            assert bound is not None, f"{kind}<{in_dtype}>: no measured float64 bound yet (this run measured {d} ulp)"
            assert d <= bound, (kind, in_dtype, q, d, bound)
        else:
            if not same_bits(g, w):
                bad = np.nonzero(~((g == w) | ((g != g) & (w != w))))[0][:5]
                raise AssertionError((what, kind, np.dtype(in_dtype).name, q, bad, g[bad], w[bad]))


def inputs_for(kind, in_dtype, n, seed=1):
    """n elements per input port: the special values of the type, then random ones, repeated to the length"""
    rng = np.random.default_rng(seed)
    a = np.resize(CO.special_values(in_dtype, rng), n)
    if kind in ("RealImagToComplex", "MagPhaseToComplex"):
        b = np.resize(rng.permutation(CO.special_values(in_dtype, rng)), n)
        return (a, b)
    return (a,)


def scales_for(dt):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return [1.0, -2.5, 0.37, 1e30 if dt == np.float32 else 1e300]  # the last overflows the product
    over = {1: float(np.iinfo(dt).max), 2: float(np.iinfo(dt).max), 4: 100003.0, 8: float(2 ** 40 + 1)}[dt.itemsize]  # uint16: 65535^2 is past 2^31
    return [1.0, -3.0, 3.0, over]


def tile(kind, in_dtype, out_dtype=None):
    return make(kind, in_dtype, out_dtype).tile()


ONE_TYPE_KINDS = [(k, t) for k in ("Abs", "Real", "Imag", "Arg", "RadiansToDegree", "DegreeToRadians", "ToRealImag", "RealImagToComplex", "ToMagPhase", "MagPhaseToComplex")
                  for t, _ in CO.accepted_pairs(k)]
INTERLEAVED = [(k, t, r) for k in ("ComplexToInterleaved", "InterleavedToComplex") for t, r in CO.accepted_pairs(k)]


@pytest.mark.parametrize("in_dtype", CO.ARITH, ids=lambda d: np.dtype(d).name)
def test_scaling_convert_and_convert_every_pair(in_dtype):
    """all 100 pairs, both kinds: extremes, +-0, NaN, +-inf, out-of-range floats and random values; scale 1, negative, overflowing, non-integer"""
    for out_dtype in CO.ARITH:
        n = 2 * tile("Convert", in_dtype, out_dtype) + 5
        x = inputs_for("Convert", in_dtype, n)
        compare("Convert", in_dtype, device("Convert", x, out_dtype), CO.run("Convert", x, out_dtype))
        conv = make("ScalingConvert", in_dtype, out_dtype, 1.0)
        for scale in scales_for(in_dtype):
            conv.set_scale(scale)
            compare("ScalingConvert", in_dtype, device("ScalingConvert", x, conv=conv), CO.run("ScalingConvert", x, out_dtype, scale), f"scale {scale} -> {np.dtype(out_dtype)}: ")
        w = conv.tile()  # every instantiation's own tile: the guard of its last vector, one item short of and one past a whole workgroup
        for n in (w - 1, w + 1):
            x = inputs_for("Convert", in_dtype, n, seed=n)
            compare("ScalingConvert", in_dtype, device("ScalingConvert", x, conv=conv), CO.run("ScalingConvert", x, out_dtype, scale), f"n = {n} -> {np.dtype(out_dtype)}: ")


def test_scaling_convert_known_answers():
    assert device("ScalingConvert", (np.array([200], np.uint8),), np.float32, 200)[0][0] == np.float32(40000)
    assert device("ScalingConvert", (np.array([-300], np.int16),), np.int16, 300)[0][0] == -24464
    assert device("Convert", (np.array([2 ** 60 + 2 ** 36 + 1], np.int64),), np.float32)[0][0] == np.float32(float.fromhex("0x1.000002p+60"))  # one rounding
    assert device("Abs", (np.array([200], np.uint8),))[0][0] == 56
    assert device("Abs", (np.array([-2 ** 31], np.int32),))[0][0] == -2 ** 31
    assert device("Arg", (np.array([complex(-0.0, -0.0)], np.complex64),))[0][0] == -np.float32(np.pi)
    x = np.linspace(0.1, 6.3, 100000, dtype=np.float32)
    assert np.array_equal(device("RadiansToDegree", (x,))[0], (x / np.float32(np.pi)) * np.float32(180))


@pytest.mark.parametrize("kind,in_dtype", ONE_TYPE_KINDS, ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_every_other_kind(kind, in_dtype):
    n = 2 * tile(kind, in_dtype) + 5
    x = inputs_for(kind, in_dtype, n)
    compare(kind, in_dtype, device(kind, x), CO.run(kind, x))


@pytest.mark.parametrize("kind,in_dtype,out_dtype", INTERLEAVED, ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_interleaved_kinds(kind, in_dtype, out_dtype):
    n = 2 * tile(kind, in_dtype, out_dtype) + 5
    x = inputs_for(kind, in_dtype, n * (2 if kind == "InterleavedToComplex" else 1))
    compare(kind, in_dtype, device(kind, x, out_dtype), CO.run(kind, x, out_dtype))


LENGTH_CASES = ([("ScalingConvert", np.dtype(t), np.dtype(r)) for t, r in ((np.uint8, np.float64), (np.float64, np.int8), (np.float32, np.int16), (np.int16, np.int16), (np.int64, np.float32))]
                + [(k, t, None) for k, t in ONE_TYPE_KINDS] + [(k, t, r) for k, t, r in INTERLEAVED if np.dtype(r if k[0] == "C" else t) in (np.int16, np.float64)])


@pytest.mark.parametrize("kind,in_dtype,out_dtype", LENGTH_CASES, ids=lambda v: "-" if v is None else v if isinstance(v, str) else np.dtype(v).name)
def test_lengths_around_the_tile(kind, in_dtype, out_dtype):
    w = tile(kind, in_dtype, out_dtype)
    conv = make(kind, in_dtype, out_dtype, -3.0)
    for n in (0, 1, 2, 3, w - 1, w, w + 1, 2 * w + 5):
        if kind == "InterleavedToComplex":
            n -= n % 2
        x = inputs_for(kind, in_dtype, n, seed=n + 2)
        compare(kind, in_dtype, device(kind, x, conv=conv), CO.run(kind, x, out_dtype, -3.0), f"n = {n}: ")


def raw_process(conv, ins, outs, n_in):
    pin = (C.c_void_p * len(ins))(*ins)
    pout = (C.c_void_p * len(outs))(*outs)
    return G().capi.lib().gr4hip_convert_process(conv._h, pin, pout, n_in, None, torch.cuda.current_stream().cuda_stream)


def test_refusals():
    g = G()
    capi, L = g.capi, g.capi.lib()
    conv = make("InterleavedToComplex", np.int16, np.complex64)
    x = torch.zeros(8, dtype=torch.int16, device="cuda")
    y = torch.full((8,), 7, dtype=torch.complex64, device="cuda")
    for odd in (1, 3):
        assert raw_process(conv, [x.data_ptr()], [y.data_ptr()], odd) == capi.INVALID_ARGUMENT
    assert raw_process(conv, [None], [y.data_ptr()], 4) == capi.INVALID_ARGUMENT
    assert raw_process(conv, [x.data_ptr() + 1], [y.data_ptr()], 4) == capi.INVALID_ARGUMENT  # not aligned to an int16
    assert L.gr4hip_convert_process(None, None, None, 4, None, None) == capi.INVALID_ARGUMENT
    assert L.gr4hip_convert_reset(None) == capi.INVALID_ARGUMENT and L.gr4hip_convert_set_scale(None, 1.0) == capi.INVALID_ARGUMENT
    assert L.gr4hip_convert_set_scale(conv._h, 2.0) == capi.INVALID_ARGUMENT  # not a ScalingConvert
    torch.cuda.synchronize()
    assert bool((y == 7).all()), "a refused call wrote to its output"
    h = C.c_void_p()
    for kind, (i, o) in (("Abs", (capi.C32, capi.C32)), ("Convert", (capi.C32, capi.F32)), ("Real", (capi.F32, capi.F32)), ("InterleavedToComplex", (capi.I32, capi.C32)),
                         ("ComplexToInterleaved", (capi.C32, capi.U8)), ("RadiansToDegree", (capi.I32, capi.I32)), ("MagPhaseToComplex", (capi.F32, capi.C64))):
        p = capi.ConvertParams(capi.CONVERT_KINDS.index(kind), i, o, 1.0)
        assert L.gr4hip_convert_create(C.byref(h), C.byref(p)) == capi.INVALID_ARGUMENT and not h.value, kind
    with pytest.raises(capi.Gr4HipError):
        conv.process_bulk(torch.zeros(3, dtype=torch.int16, device="cuda"))
    with pytest.raises(capi.Gr4HipError):
        conv.process_bulk(torch.zeros(4, dtype=torch.int16))  # a host tensor


class Placed:
    """a device tensor of n elements that starts `off` elements behind a 256-byte boundary, with 0xA5 sentinel bytes around it"""
    GUARD = 256

    def __init__(self, np_dtype, n, off, data=None):
        dt = np.dtype(np_dtype)
        self.nbytes = n * dt.itemsize
        self.buf = torch.full((self.nbytes + 3 * self.GUARD + 64 * dt.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        self.start = (-self.buf.data_ptr()) % 256 + self.GUARD + off * dt.itemsize
        self.t = self.buf[self.start:self.start + self.nbytes].view(tdtype(dt))
        assert (self.t.data_ptr() - off * dt.itemsize) % 256 == 0 and self.t.numel() == n
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def sentinels_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[self.start - 64:self.start] == 0xA5).all() and (b[self.start + self.nbytes:self.start + self.nbytes + 64] == 0xA5).all())


ALIGN_CASES = [("Convert", np.uint8, np.float64), ("Convert", np.float64, np.int8), ("InterleavedToComplex", np.int16, np.complex64), ("ToMagPhase", np.complex64, None),
               ("RealImagToComplex", np.float32, None)]


@pytest.mark.parametrize("kind,in_dtype,out_dtype", ALIGN_CASES, ids=lambda v: "-" if v is None else v if isinstance(v, str) else np.dtype(v).name)
def test_any_element_alignment(kind, in_dtype, out_dtype):
    conv = make(kind, in_dtype, out_dtype)
    n = 2 * conv.tile() + 5
    x = inputs_for(kind, in_dtype, n * conv.in_chunk)
    aligned = device(kind, x, conv=conv)
    out_np = aligned[0].dtype
    n_out = aligned[0].size
    for offs in itertools.product((1, 2, 3), repeat=conv.n_inputs + conv.n_outputs):  # agreeing and disagreeing misalignments of the ports
        ins = [Placed(in_dtype, x[p].size, offs[p], x[p]) for p in range(conv.n_inputs)]
        outs = [Placed(out_np, n_out, offs[conv.n_inputs + q]) for q in range(conv.n_outputs)]
        conv.process_bulk(*[i.t for i in ins], out=[o.t for o in outs] if conv.n_outputs > 1 else outs[0].t)
        for q, o in enumerate(outs):
            assert np.array_equal(o.t.cpu().numpy().view(np.uint8), aligned[q].view(np.uint8)), (kind, offs, q)
            assert o.sentinels_intact(), (kind, offs, q)
    if conv.n_outputs == 2:  # an unconnected port is skipped and the other is unchanged
        for connected in ((True, False), (False, True)):
            keep = connected.index(True)
            o = Placed(out_np, n_out, 1)
            res = conv.process_bulk(torch.from_numpy(x[0]).cuda(), out=[o.t if c else None for c in connected], connected=connected)
            assert res[1 - keep] is None
            assert np.array_equal(res[keep].cpu().numpy().view(np.uint8), aligned[keep].view(np.uint8)) and o.sentinels_intact()


def test_ingest_run_as_one_launch():
    """InterleavedToComplex<int16, complex<float>> -> MultiplyConst -> Rotator: the converter with the two neighbours as its epilogue equals the three handles run
    one after the other, in one call and cut into calls, the position carried; reset starts the stream again"""
    g = G()
    conv = make("InterleavedToComplex", np.int16, np.complex64)
    w = conv.tile()
    n = 3 * w + 7  # complex samples
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-32768, 32767, 2 * n, dtype=np.int16, endpoint=True)).cuda()
    gain = ("Multiply", 1.0 / 32768)
    rot = ("Rotator", 0.0123, 0.5)
    m1, m2 = g.Merged(torch.complex64, [gain]), g.Merged(torch.complex64, [rot])
    want = m2.process_bulk(m1.process_bulk(conv.process_bulk(x))).cpu().numpy()
    fused = make("InterleavedToComplex", np.int16, np.complex64)
    fused.set_epilogue(g.Merged(torch.complex64, [gain, rot]))
    one = fused.process_bulk(x).cpu().numpy()
    assert np.array_equal(one.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(one, conv.process_bulk(x).cpu().numpy())
    again = fused.process_bulk(x[:64]).cpu().numpy()  # the position went on: not the start of the stream
    assert not np.array_equal(again, want[:32])
    for _ in range(2):
        fused.reset()
        out = torch.empty(n, dtype=torch.complex64, device="cuda")
        at = 0
        for m in (2, w - 2, w, n - 2 * w):
            fused.process_bulk(x[2 * at:2 * (at + m)], out=out[at:at + m])
            at += m
        assert at == n and np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    fused.set_epilogue(None)
    assert np.array_equal(fused.process_bulk(x).cpu().numpy(), conv.process_bulk(x).cpu().numpy())


def test_prologue_on_a_narrowing_convert():
    g = G()
    conv = make("Convert", np.float32, np.int16)
    n = 2 * conv.tile() + 5
    x = torch.from_numpy(inputs_for("Convert", np.float32, n)[0]).cuda()
    gain = g.Merged(torch.float32, [("Multiply", 1000.5)])
    want = conv.process_bulk(gain.process_bulk(x)).cpu().numpy()
    fused = make("Convert", np.float32, np.int16)
    fused.set_prologue(gain)
    out = torch.empty(n, dtype=torch.int16, device="cuda")
    at = 0
    for m in (2, conv.tile() - 2, conv.tile(), 5):
        fused.process_bulk(x[at:at + m], out=out[at:at + m])
        at += m
    assert at == n and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(fused.process_bulk(x).cpu().numpy(), want)
    assert not np.array_equal(want, conv.process_bulk(x).cpu().numpy())


def test_hooks_that_do_not_fit_are_refused():
    g = G()
    capi = g.capi
    cases = [(make("InterleavedToComplex", np.int16, np.complex64), "set_epilogue", torch.float32),  # the output is complex<float>
             (make("InterleavedToComplex", np.int16, np.complex64), "set_prologue", torch.complex64),  # the input is int16
             (make("Convert", np.float32, np.int16), "set_prologue", torch.int16),
             (make("ToMagPhase", np.complex64), "set_epilogue", torch.float32),  # two outputs
             (make("RealImagToComplex", np.float32), "set_prologue", torch.float32)]  # two inputs
    for conv, which, dtype in cases:
        with pytest.raises(capi.Gr4HipError) as e:
            getattr(conv, which)(g.Merged(dtype, [("Multiply", 2)]))
        assert e.value.status == capi.UNSUPPORTED
    make("ToMagPhase", np.complex64).set_prologue(g.Merged(torch.complex64, [("Multiply", 2)]))  # one input: accepted


@pytest.mark.parametrize("kind,in_dtype,out_dtype", ALIGN_CASES + [("ComplexToInterleaved", np.complex128, np.int8)],
                         ids=lambda v: "-" if v is None else v if isinstance(v, str) else np.dtype(v).name)
def test_chunk_invariance(kind, in_dtype, out_dtype):
    """any split of a call into even-length pieces gives the same bytes (the pieces start at every alignment)"""
    conv = make(kind, in_dtype, out_dtype)
    n = 2 * conv.tile() + 6
    x = inputs_for(kind, in_dtype, n * conv.in_chunk)
    whole = device(kind, x, conv=conv)
    rng = np.random.default_rng(9)
    cuts = np.unique(np.concatenate([[0, n], 2 * rng.integers(0, n // 2, 9), [2, n - 2]]))
    xs = [torch.from_numpy(a).cuda() for a in x]
    outs = [torch.empty(whole[q].size, dtype=tdtype(whole[q].dtype), device="cuda") for q in range(conv.n_outputs)]
    ic, oc = conv.in_chunk, conv.out_chunk
    for a, b in zip(cuts[:-1], cuts[1:]):
        a, b = int(a), int(b)
        pieces = [o[a * oc:b * oc] for o in outs]
        conv.process_bulk(*[t[a * ic:b * ic] for t in xs], out=pieces if conv.n_outputs > 1 else pieces[0])
    for q in range(conv.n_outputs):
        assert np.array_equal(outs[q].cpu().numpy().view(np.uint8), whole[q].view(np.uint8)), (kind, q)


def test_two_handles_on_two_streams():
    n = 1 << 16
    rng = np.random.default_rng(3)
    xa = rng.integers(-32768, 32767, 2 * n, dtype=np.int16, endpoint=True)
    xb = (rng.standard_normal(n) * 3e4).astype(np.float32)
    a, b = make("InterleavedToComplex", np.int16, np.complex64), make("Convert", np.float32, np.int16)
    ta, tb = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    oa, ob = torch.empty(n, dtype=torch.complex64, device="cuda"), torch.empty(n, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    step = n // 8
    for k in range(8):
        with torch.cuda.stream(sa):
            a.process_bulk(ta[2 * k * step:2 * (k + 1) * step], out=oa[k * step:(k + 1) * step])
        with torch.cuda.stream(sb):
            b.process_bulk(tb[k * step:(k + 1) * step], out=ob[k * step:(k + 1) * step])
    sa.synchronize()
    sb.synchronize()
    assert np.array_equal(oa.cpu().numpy(), CO.interleaved_to_complex(xa, np.complex64))
    assert np.array_equal(ob.cpu().numpy(), CO.convert(xb, np.int16))


def test_graphs_on_the_device(tmp_path):
    """test_host_converter --device: every kind with compute_domain gpu:hip:0 through the seam (bit for bit with the oracle; the transcendental kinds within 1 ulp of
    float32), the ingest graph planned by hip::plan with converter, gain and rotator as ONE stage and within 1e-5 of the host-domain front end, the narrowing graph
    PowerSpectrum (gpu) -> Convert<float, int16> bit for bit with the host-domain Convert, all 246 registered names, and ToMagPhase made by its registered name
    feeding two sinks"""
    import os
    import subprocess
    from test_converter_host import GRAPH_CASES, HOST_SCALE, PORTS, TNAME, write_inputs
    from test_host_cpp import BIN, PLUGIN, ROOT
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    inputs = write_inputs(tmp_path)
    r = subprocess.run([os.path.join(BIN, "test_host_converter"), "--device", str(tmp_path), PLUGIN], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all converter device checks passed" in r.stdout
    assert "ToRealImag with `imag` open:" in r.stdout and "ScalingConvert scale by settings in mid-stream:" in r.stdout  # (a FAILED line fails the program)
    assert "ingest run: convert_InterleavedToComplex_i16_c32[post: mul,rot] -> fir_c32" in r.stdout
    for kind, t, o in GRAPH_CASES:
        t, o = np.dtype(t), np.dtype(o)
        x = inputs[t][:2 if kind in ("RealImagToComplex", "MagPhaseToComplex") else 1]
        want = CO.run(kind, x, o, HOST_SCALE)
        got = tuple(np.fromfile(tmp_path / f"dev_{kind}_{TNAME[t]}_{TNAME[o]}_{port}.bin", dtype=w.dtype) for port, w in zip(PORTS[kind], want))
        compare(kind, t, got, want, "graph: ")
    x = inputs[np.dtype(np.complex64)][:1]
    got = (np.fromfile(tmp_path / "plugin_mag.bin", dtype=np.float32), np.fromfile(tmp_path / "plugin_phase.bin", dtype=np.float32))
    compare("ToMagPhase", np.complex64, got, CO.run("ToMagPhase", x), "plugin: ")
