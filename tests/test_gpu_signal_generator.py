"""The device SignalGenerator (gnuradio4_amd/csrc/signal_generator.hip, G.SignalGenerator) against the oracle (tests/signal_generator_oracle.py) and the
reference-made fixture tests/golden/signal_generator_reference.npz: values, independence of the cutting into calls, the Gaussian tail kernel, deep jumps of the
noise stream, the stall of the float time base, output alignment, the life cycle, and the C++ blocks in a graph.  Bounds: tests/test_signal_generator_oracle.py."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import signal_generator_oracle as SG
from test_host_cpp import host_bins  # noqa: F401  (the fixture that builds the host programs)
from test_signal_generator_oracle import CASES, EXACT, N, bound_for, fixture_generator

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TORCH = {"f32": torch.float32, "f64": torch.float64, "c32": torch.complex64, "i16": torch.int16}
ALL = [(d, t) for d in CASES for t in range(11)]
_cache = {}


def G():
    import gnuradio4_amd
    return gnuradio4_amd


def device_generator(dtype, t, **kw):
    amp, off = CASES[dtype]
    s = dict(sample_rate=1000.0, frequency=37.5, amplitude=amp, offset=off, phase=0.3, seed=12345)
    s.update(kw)
    return G().SignalGenerator(t, TORCH[dtype], **s)


def one_call(dtype, t):
    """the device's 200 000 fixture samples in one call, and the oracle's: computed once, shared, not modified"""
    if (dtype, t) not in _cache:
        got = device_generator(dtype, t).generate(N).cpu().numpy()
        want = fixture_generator(dtype, t).generate(N)
        got.setflags(write=False)
        want.setflags(write=False)
        _cache[(dtype, t)] = (got, want)
    return _cache[(dtype, t)]


def err(a, b):
    return float(np.abs(a.astype(np.complex128) - b.astype(np.complex128)).max()) if len(a) else 0.0


def check(got, want, dtype, t, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (dtype, t, what)
    e = err(got, want)
    print(f"{what}{dtype} {SG.TYPES[t]}: max |device - oracle| {e:.3e}")
    if t in EXACT:
        assert np.array_equal(got, want), (dtype, t, what, e)
    else:
        assert e <= bound_for(dtype, t), (dtype, t, what, e)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(O.ROOT, "tests", "golden", "signal_generator_reference.npz"))


@pytest.mark.parametrize("dtype,t", ALL)
def test_fixture_every_type(fx, dtype, t):
    got, want = one_call(dtype, t)
    check(got, want, dtype, t)
    e = err(got[fx["index"]], fx[f"{dtype}_{t}"])
    print(f"{dtype} {SG.TYPES[t]}: max |device - reference| at the fixture's positions {e:.3e}")
    if t in EXACT:
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(fx[f"{dtype}_{t}_sha256"]), (dtype, t, e)
    else:
        assert e <= bound_for(dtype, t), (dtype, t, e)


@pytest.mark.parametrize("dtype,t", ALL)
def test_chunking_is_bit_identical(dtype, t):
    whole, _ = one_call(dtype, t)
    run, tile = G().SignalGenerator.run(), G().SignalGenerator.tile()
    lengths = [1, 2, 3, run - 1, run, run + 1, tile - 1, tile, tile + 1, 65535, 1, 1]
    lengths.append(N - sum(lengths))
    gen = device_generator(dtype, t)
    out = torch.empty(N, dtype=TORCH[dtype], device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # one non-default stream, nothing waits between the calls
        at = 0
        for m in lengths:
            gen.generate_into(out[at:at + m])
            at += m
    stream.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint8), whole.view(np.uint8)), (dtype, t, int(np.nonzero(got != whole)[0][0]))


@pytest.mark.parametrize("dtype", list(CASES))
def test_gaussian_tail_kernel(dtype):
    """too few launched attempts: the tail kernel finishes the call sequentially, with the same values and the same stream state afterwards"""
    t, lengths = SG.GAUSSIAN, [5001, 4, 7, 1, 1, 10, 2048]
    total = sum(lengths)
    want = fixture_generator(dtype, t).generate(total)
    default = device_generator(dtype, t).generate(total).cpu().numpy()
    check(default, want, dtype, t, "one call, default attempts: ")
    try:
        for permille in (1000, 500, 1):
            G().capi.developer_switch("GR4HIP_SIGGEN_GAUSS_PERMILLE", permille)
            gen = device_generator(dtype, t)
            got = torch.cat([gen.generate(m) for m in lengths]).cpu().numpy()
            assert np.array_equal(got.view(np.uint8), default.view(np.uint8)), (dtype, permille, int(np.nonzero(got != default)[0][0]))
            check(got, want, dtype, t, f"{permille} attempts per 1000 pairs: ")
            assert np.array_equal(device_generator(dtype, t).generate(5001).cpu().numpy().view(np.uint8), default[:5001].view(np.uint8)), (dtype, permille)
    finally:
        G().capi.developer_switch("GR4HIP_SIGGEN_GAUSS_PERMILLE", 0)


def c_draws_from(state, n):
    """n draws of the C oracle's generator (oracle/gr4_oracle.c) from a given state"""
    st = (C.c_uint64 * 4)(*state)
    return np.array([O.lib().gr4o_xoshiro_next(st) for _ in range(n)], dtype=np.uint64)


@pytest.mark.parametrize("dtype,t,n", [("f32", SG.UNIFORM, (1 << 24) + 3), ("c32", SG.TRIANGULAR, (1 << 22) + 1)])
def test_deep_jumps_are_exact(dtype, t, n):
    per = 1 if dtype == "f32" else 4
    st = SG.seed_state(777)
    raw = SG.draws(st, per * n)
    # the numpy stream is the C oracle's: at the start, and stepped by the C code from a jumped state at the far end
    assert np.array_equal(raw[:2048], O.xoshiro_draws(777, 2048))
    assert np.array_equal(raw[-2048:], c_draws_from(SG.jump(st, per * n - 2048), 2048))
    want = SG.Generator(dtype, signal_type=t, amplitude=1.5, offset=0.25, seed=777).generate(n)
    gen = G().SignalGenerator(t, TORCH[dtype], amplitude=1.5, offset=0.25, seed=777)
    got = gen.generate(n).cpu().numpy()
    assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])
    # ... and the state the kernel left on the device is the one behind the last draw
    more = gen.generate(1000).cpu().numpy()
    o = SG.Generator(dtype, signal_type=t, amplitude=1.5, offset=0.25, seed=777)
    o.state = SG.jump(st, per * n)
    assert np.array_equal(more, o.generate(1000))


def test_float_time_stall_is_reproduced():
    """complex<float> at 1 kHz: every segment of the float time base up to 2^24 + 2^20 samples in one call, then on through the stall (n = 25 150 896, t = 32768)"""
    n1, n2 = (1 << 24) + (1 << 20), 1 << 23
    gen = G().SignalGenerator("Saw", torch.complex64, sample_rate=1000.0, frequency=37.5, amplitude=1.5, offset=0.25, phase=0.3)
    o = SG.Generator("c32", signal_type=SG.SAW, sample_rate=1000.0, frequency=37.5, amplitude=1.5, offset=0.25, phase=0.3, table_time=True)
    for n in (n1, n2):
        got, want = gen.generate(n).cpu().numpy(), o.generate(n)
        assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])
    assert o.n > 25_150_896 and np.all(want[-1000:] == want[-1])  # the time stands still: so does the signal


def test_double_time_in_far_binades_from_the_start():
    n = 1 << 20
    kw = dict(sample_rate=3e9, frequency=1e6, amplitude=1.5, offset=0.25, phase=0.3)
    got = G().SignalGenerator("Saw", torch.float64, **kw).generate(n).cpu().numpy()
    want = SG.Generator("f64", signal_type=SG.SAW, **kw).generate(n)  # (sequential additions)
    assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])


@pytest.mark.parametrize("dtype", ["f32", "i16", "c32"])
@pytest.mark.parametrize("t", [SG.SIN, SG.UNIFORM, SG.GAUSSIAN])
def test_any_output_alignment(dtype, t):
    n = G().SignalGenerator.run() * G().SignalGenerator.tile() + 1
    aligned = device_generator(dtype, t).generate(n)
    for off in (1, 3):
        buf = torch.zeros(n + 8, dtype=TORCH[dtype], device="cuda")
        device_generator(dtype, t).generate_into(buf[off:off + n])
        assert torch.equal(buf[off:off + n], aligned), (dtype, t, off)
        edges = torch.cat([buf[:off], buf[off + n:]])
        assert not (torch.view_as_real(edges) if edges.is_complex() else edges).ne(0).any()  # nothing outside the span


@pytest.mark.parametrize("dtype", list(CASES))
def test_life_cycle(dtype):
    gen, o = device_generator(dtype, SG.FAST_SIN), fixture_generator(dtype, SG.FAST_SIN)

    def both(n, t):
        got = gen.generate(n).cpu().numpy()
        check(got, o.generate(n), dtype, t, "life cycle: ")
        return got
    both(1000, SG.FAST_SIN)
    # configure: the time keeps running (Saw shows it), the phasor count restarts, the noise is re-seeded
    for t, kw in ((SG.SAW, {}), (SG.FAST_COS, {}), (SG.GAUSSIAN, dict(seed=99)), (SG.UNIFORM, dict(seed=99)), (SG.TRIANGLE, dict(sample_rate=48000.0)),
                  (SG.SIN, dict(frequency=0.0))):
        gen.configure(signal_type=t, **kw)
        o.configure(signal_type=t, **kw)
        got = both(1001, t)
    assert np.all(got == got[0])  # frequency = 0: Const (ToneGenerator.hpp:48)
    # n = 0 changes nothing
    gen.configure(signal_type=SG.GAUSSIAN, frequency=37.5, sample_rate=1000.0)
    o.configure(signal_type=SG.GAUSSIAN, frequency=37.5, sample_rate=1000.0)
    both(3, SG.GAUSSIAN)
    assert gen.generate(0).numel() == 0
    both(4, SG.GAUSSIAN)
    # reset zeroes the time
    gen.configure(signal_type=SG.SAW)
    gen.reset()
    first = gen.generate(2000).cpu().numpy()
    fresh = device_generator(dtype, SG.SAW).generate(2000).cpu().numpy()
    assert np.array_equal(first, fresh)
    with pytest.raises(G().capi.Gr4HipError):
        gen.configure(sample_rate=0.0)
    assert np.array_equal(gen.generate(5).cpu().numpy(), device_generator(dtype, SG.SAW).generate(2005).cpu().numpy()[2000:])  # a refused configure changes nothing


def test_blocks_in_a_graph(host_bins):  # noqa: F811
    """gr::basic::SignalGenerator<float> with compute_domain gpu:hip:0 against the host-domain block through a sink, and hip::SignalSource<complex<float>> ->
    OnDevice<fir_filter> -> D2H -> sink against the same graph fed from the host block through H2D (gnuradio4_amd/host/tests/test_host_signal_generator.cpp)"""
    r = subprocess.run([os.path.join(host_bins, "test_host_signal_generator"), "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "SignalGenerator<float> UniformNoise gpu:hip:0 == host domain: bit for bit" in r.stdout
    assert "SignalGenerator<float> new settings, then reset, between chunks, gpu:hip:0 == host domain: bit for bit" in r.stdout  # configure and reset on the live handle
    assert "hip::SignalSource<complex<float>> -> OnDevice<fir_filter> -> D2H == host SignalGenerator -> H2D -> OnDevice<fir_filter> -> D2H: bit for bit" in r.stdout
    assert "FAILED" not in r.stdout and "all signal generator graph checks passed" in r.stdout
