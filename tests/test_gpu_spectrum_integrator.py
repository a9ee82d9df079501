"""The spectrum integrator on the device (gr4hip_specint_*, gr4hip_fft_mag2_integrate, gr4hip_pfb_power_integrate; csrc/spectrum_integrator.hip,
csrc/specint_kernels.hpp) against its oracle (tests/spectrum_integrator_oracle.py): parity with the float64 sums, the defined order of additions bit for bit, the
fused entries against the two-call composition bit for bit, cuts, state, non-finite values, the paths and the refusals.  TOL is the parity contract's 1e-5.

Every fused entry runs twice: as it dispatches by default, and with its sink kernel forced through the test hook gr4hip_internal_specint_set_path (the sink is the
default only where it measured faster than the composition, SPECTRUM_INTEGRATOR.md; the other sizes keep theirs behind the hook, and it is tested all the same).

Shapes: N = 8 and 64 (the FFT block's LDS kernel: composition), 256 / 1024 / 8192 (the fused sink with 32 / 8 / 1 leaves per workgroup), 1000 (mixed radix) and
16384 (four-step): composition.  A = 1, 2, 31, 32, 33, 67: below, at and above a leaf, and a ragged last leaf.  2 A + 3 frames: two spectra and a dropped tail;
the sink sizes once with 2 FPB 32 + 5 frames, so that the grid has more than two workgroups and a ragged last one.  8192 points stay below 256 frames (above,
gr4hip_fft_mag2 takes another kernel) except in the one test about exactly that."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
import pfb_oracle as PO
import spectrum_integrator_oracle as SO

pytestmark = pytest.mark.gpu
TOL = 1e-5
SIZES = [8, 64, 256, 1024, 8192, 1000, 16384]
BANK_SIZES = [8, 64, 256, 1024, 8192]  # the bank's sizes (powers of two <= 8192)
SINK_SIZES = [256, 1024, 8192]
LENGTHS = [1, 2, 31, 32, 33, 67]
P = 4
LONG_A = 33  # the A of the long runs (several workgroups)
CANARY = -77.25
HOST_BIN = os.path.join(O.ROOT, "build", "host", "test_host_spectrum_integrator")
PLUGIN = os.path.join(O.ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")


def fpb(N):
    return 8192 // N


def n_frames(N, A):
    return max(2 * A + 3, 2 * fpb(N) * 32 + 5) if N in SINK_SIZES and A == LONG_A else 2 * A + 3


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


@pytest.fixture
def devsw(G):
    """developer switches of the library, restored when the test ends"""
    used = set()

    def set_(name, value=1):
        used.add(name)
        G.capi.developer_switch(name, value)
    yield set_
    for name in used:
        G.capi.developer_switch(name, 0)


_cases = {}


def case(N):
    """input, float64 |X|^2 of the Hann FFT block and (bank sizes) of the bank with P = 4, for the longest run of this size: computed once, shared, read-only"""
    if N not in _cases:
        frames = max(n_frames(N, A) for A in LENGTHS)
        x = SO.signal(frames * N, 7 * N + 1)
        w = O.window([s.lower() for s in O.WINDOWS].index("hann"), N, np.float32).astype(np.float64)  # the block multiplies by its float32 window
        t_fft = np.stack([np.abs(O.dft64(fr.astype(np.complex128) * w)) ** 2 for fr in x.reshape(frames, N)])
        t_pfb = np.abs(PO.pfb(PO.design(N, P, "Hamming"), x, N, P)) ** 2 if N in BANK_SIZES else None
        for a in (x, t_fft, t_pfb):
            if a is not None:
                a.setflags(write=False)
        _cases[N] = (x, t_fft, t_pfb)
    return _cases[N]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared cases are read-only)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def last_path(G, si):
    v = C.c_int(-1)
    assert G.capi.lib().gr4hip_internal_specint_last_path(si._h, C.byref(v)) == 0  # (test hook, not in include/gr4hip.h)
    return v.value


def set_path(G, si, path):
    """test hook: 1 = the sink wherever a kernel exists, 2 = the composition, 0 = the measured default"""
    assert G.capi.lib().gr4hip_internal_specint_set_path(si._h, C.c_int(path)) == 0
    return si


# where the sink kernel is the default: the FFT block up to 4096 points, the bank with one tap per channel ("pfb" is this file's bank, P = 4)
SINK_DEFAULT = {"fft": {256, 512, 1024, 2048, 4096}, "pfb": set(), "pfb1": {256, 512, 1024, 2048, 4096, 8192}}
PATHS = [0, 1]  # every fused entry is tested as it runs by default and with its sink kernel forced (the sizes whose sink measured slower keep it behind the hook)


def default_path(N, name):
    """SPECTRUM_INTEGRATOR.md: the sink is the default where it measured faster than the composition"""
    return 1 if N in SINK_DEFAULT[name] else 2


def torch_ordered(m, A, mean):
    """the definition with torch element-wise ops on the device: float32 adds frame by frame, float64 adds leaf by leaf (IEEE, in the stated order)"""
    m = m.reshape(-1, m.shape[-1])
    q = m.shape[0] // A
    out = torch.empty((q, m.shape[1]), dtype=torch.float32, device=m.device)
    for i in range(q):
        acc = torch.zeros(m.shape[1], dtype=torch.float64, device=m.device)
        for s in range(0, A, SO.LEAF):
            leaf = torch.zeros(m.shape[1], dtype=torch.float32, device=m.device)
            for f in range(i * A + s, i * A + min(s + SO.LEAF, A)):
                leaf = leaf + m[f]
            acc = acc + leaf.double()
        out[i] = (acc / float(A) if mean else acc).float()
    return out


def entries(G, N):
    """(name, transform factory, |X|^2 of the transform, fused call) of the entries this size has"""
    e = [("fft", lambda: G.FFT(N, "Hann"), lambda f, x: f.mag2(x), lambda f, x, si, **k: f.power_integrated(x, si, **k))]
    if N in BANK_SIZES:
        e.append(("pfb", lambda: G.PolyphaseFilterBank(N, P), lambda f, x: f.power(x), lambda f, x, si, **k: f.power_integrated(x, si, **k)))
    return e


def integ(G, N, A, mean=False, path=0):
    return set_path(G, G.SpectrumIntegrator(N, A, mean), path)


@pytest.mark.parametrize("A", LENGTHS)
@pytest.mark.parametrize("N", SIZES)
def test_parity(G, N, A):
    """sum and mean through both fused entries and through specint_process on gr4hip_fft_mag2's output, against the float64 sums of the float64 |X|^2"""
    x, t_fft, t_pfb = case(N)
    M = n_frames(N, A)
    xd = dev(x[:M * N])
    for mean in (False, True):
        for name, make, _, fused in entries(G, N):
            truth = SO.integrate((t_fft if name == "fft" else t_pfb)[:M], A, mean)
            for path in PATHS:
                got = fused(make(), xd, integ(G, N, A, mean, path)).cpu().numpy()
                assert got.shape == truth.shape and got.dtype == np.float32
                e = PO.rel(got, truth)
                print(f"N {N} A {A} mean {mean} {name} fused entry ({'default' if path == 0 else 'sink forced'}): {e:.2e}")
                assert e <= TOL
        got = G.SpectrumIntegrator(N, A, mean).process_bulk(G.FFT(N, "Hann").mag2(xd)).cpu().numpy()
        e = PO.rel(got, SO.integrate(t_fft[:M], A, mean))
        print(f"N {N} A {A} mean {mean} mag2 -> specint_process: {e:.2e}")
        assert e <= TOL


@pytest.mark.parametrize("A", LENGTHS)
@pytest.mark.parametrize("N", SIZES)
def test_the_order_bit_for_bit(G, N, A):
    """specint_process is the definition (torch element-wise ops on the device); both fused entries are |X|^2 -> specint_process"""
    x, _, _ = case(N)
    M = n_frames(N, A)
    xd = dev(x[:M * N])
    for mean in (False, True):
        for name, make, mag2, fused in entries(G, N):
            m = mag2(make(), xd)
            two = G.SpectrumIntegrator(N, A, mean).process_bulk(m)
            assert two.shape == (M // A, N)
            if name == "fft":
                assert same(two, torch_ordered(m, A, mean)), (name, mean)
            for path in PATHS:
                si = integ(G, N, A, mean, path)
                assert same(fused(make(), xd, si), two), (name, mean, path)
                if path == 1:
                    assert last_path(G, si) == (1 if N in SINK_SIZES else 2)


def test_8192_points_do_not_depend_on_the_frame_count(G, devsw):
    """300 frames of 8192 points: gr4hip_fft_mag2 would take the frame pipeline (equal to the block kernel to rounding only); the integrating entry never does"""
    N, A, M = 8192, 67, 300
    xd = dev(SO.signal(M * N, 5))
    devsw("GR4HIP_FFT_NO_PIPELINE", 1)
    m = G.FFT(N, "Hann").mag2(xd)
    devsw("GR4HIP_FFT_NO_PIPELINE", 0)
    want = G.SpectrumIntegrator(N, A).process_bulk(m)
    for path in PATHS:
        si = integ(G, N, A, path=path)
        got = G.FFT(N, "Hann").power_integrated(xd, si)
        assert last_path(G, si) == (1 if path == 1 else default_path(N, "fft"))
        assert same(got, want), path
        # and a cut of it: 200 + 100 frames, both below the pipeline's threshold, give the same bits
        si2, f2 = integ(G, N, A, path=path), G.FFT(N, "Hann")
        parts = [f2.power_integrated(xd[:200 * N], si2), f2.power_integrated(xd[200 * N:], si2)]
        assert same(torch.cat(parts), want), path


def _call(G, entry, first, si, x, frames, out):
    """the C entry itself: (status, n_out)"""
    n = C.c_size_t(12345)
    args = (first._h,) if first is not None else ()
    rc = entry(*args, si._h, x.data_ptr() if x is not None else None, frames, out.data_ptr() if out is not None else None, C.byref(n), torch.cuda.current_stream().cuda_stream)
    return rc, n.value


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("A", [2, 33, 67])
@pytest.mark.parametrize("N", [64, 1024, 8192, 1000])
def test_cuts(G, N, A, path):
    """one call = calls of 1, 2, 31, 5 (ends mid-leaf), A // 2 + 1 (ends mid-integration) frames and the rest, bit for bit, for all three entries; n_out is what
    pending said; a call that completes nothing leaves the output untouched"""
    x, _, _ = case(N)
    M = n_frames(N, A)
    xd = dev(x[:M * N])
    L = G.capi.lib()
    m = G.FFT(N, "Hann").mag2(xd)
    runs = [("specint", None, L.gr4hip_specint_process, m), ("fft", G.FFT(N, "Hann"), L.gr4hip_fft_mag2_integrate, xd)]
    if N in BANK_SIZES:
        runs.append(("pfb", G.PolyphaseFilterBank(N, P), L.gr4hip_pfb_power_integrate, xd))
    for name, first, entry, data in runs:
        data = data.reshape(M, N)
        si = integ(G, N, A, path=path)
        whole = torch.full((M // A, N), CANARY, dtype=torch.float32, device="cuda")
        rc, n = _call(G, entry, first, si, data, M, whole)
        assert rc == 0 and n == M // A
        if first is not None and hasattr(first, "reset"):
            first.reset()
        si = integ(G, N, A, path=path)
        at, got = 0, []
        for cut in (1, 2, 31, 5, A // 2 + 1, M):
            c = min(cut, M - at)
            if c == 0:
                break
            want = si.pending(c)
            out = torch.full((want + 1, N), CANARY, dtype=torch.float32, device="cuda")
            rc, n = _call(G, entry, first, si, data[at:at + c], c, out)
            assert rc == 0 and n == want, (name, at, c)
            assert bool((out[want:] == CANARY).all()), (name, at, c)
            got.append(out[:want])
            at += c
        assert at == M and same(torch.cat(got), whole), name


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("N", [64, 1024, 8192])
def test_identity_and_state(G, N, path):
    x, _, _ = case(N)
    M = 40
    xd = dev(x[:M * N])
    fft = G.FFT(N, "Hann")
    m = fft.mag2(xd)
    for mean in (False, True):  # A = 1: |X|^2 value for value
        assert same(G.SpectrumIntegrator(N, 1, mean).process_bulk(m), m)
        assert same(fft.power_integrated(xd, integ(G, N, 1, mean, path)), m)
        if N in BANK_SIZES:
            bank = G.PolyphaseFilterBank(N, P)
            mb = bank.power(xd)
            bank.reset()
            assert same(bank.power_integrated(xd, integ(G, N, 1, mean, path)), mb)
    A = 33
    want = G.SpectrumIntegrator(N, A).process_bulk(m[7:7 + A])
    for fused in (False, True):
        run = (lambda si, lo, hi: fft.power_integrated(xd[lo * N:hi * N], si)) if fused else (lambda si, lo, hi: si.process_bulk(m[lo:hi]))
        si = integ(G, N, A, path=path)
        assert run(si, 0, 7).shape == (0, N)
        si.reset()  # drops the 7 frames
        assert si.pending(A - 1) == 0 and si.pending(A) == 1
        assert same(run(si, 7, 7 + A), want)
        si = integ(G, N, 5, path=path)
        assert run(si, 0, 7).shape == (1, N)  # 2 frames of the next integration are held
        si.set_length(A)  # drops them
        assert si.pending(A - 1) == 0
        assert same(run(si, 7, 7 + A), want)


@pytest.mark.parametrize("mean", [False, True])
def test_the_carried_state_through_cuts_set_length_and_reset(G, mean):
    """the state the integrating blocks share (csrc/leaf_integrator.hpp) behind the public entries alone, at N = 7 (the scalar leaf kernel, a carry that is no
    multiple of four floats) and A = 33: calls of 1, 31, 1, 0, 33, 2 frames, set_length(2) in mid-integration, 3 frames, one more, reset(), 4 frames -- every
    call returns what pending said, and the rows are the ordered definition of the segments between the drops, bit for bit"""
    N, A = 7, 33
    m = np.abs(SO.signal(76 * N, 11)).astype(np.float32).reshape(76, N) ** 2
    md = dev(m)
    si, at, got = G.SpectrumIntegrator(N, A, mean), 0, []

    def feed(n):
        nonlocal at
        want = si.pending(n)
        out = si.process_bulk(md[at:at + n])
        assert out.shape == (want, N)
        got.append(out)
        at += n

    for n in (1, 31, 1, 0, 33, 2):
        feed(n)
    assert at == 68 and si.pending(A - 2) == 1
    si.set_length(2)  # frames 66, 67 are dropped
    assert si.pending(1) == 0 and si.pending(2) == 1
    feed(3)
    feed(1)
    si.reset()
    assert si.pending(1) == 0
    feed(4)
    assert at == 76
    want = np.concatenate([SO.integrate_ordered(m[:68], A, mean), SO.integrate_ordered(m[68:72], 2, mean), SO.integrate_ordered(m[72:], 2, mean)])
    assert want.shape == (6, N) and same(torch.cat(got), torch.from_numpy(want))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("N", [64, 1024, 8192])
def test_non_finite_values_reach_exactly_their_integration(G, N, path):
    x, _, _ = case(N)
    A, M = 33, 4 * 33 + 2
    clean = np.array(x[:M * N])
    bad = clean.copy()
    bad[40 * N + 5] = np.nan  # frame 40: integration 1
    bad[(3 * A + 2) * N + 6] = np.inf  # frame 101: integration 3
    xc, xb = dev(clean), dev(bad)
    for name, make, mag2, fused in entries(G, N):
        reach = P - 1 if name == "pfb" else 0  # a bank's frame holds the P - 1 frames before it: frames 40 .. 43 and 101 .. 104, still integrations 1 and 3
        assert (40 + reach) // A == 1 and (3 * A + 2 + reach) // A == 3
        for run in (lambda d: fused(make(), d, integ(G, N, A, path=path)), lambda d: G.SpectrumIntegrator(N, A).process_bulk(mag2(make(), d))):
            want, got = run(xc), run(xb)
            assert got.shape == (4, N)
            assert same(got[0], want[0]) and same(got[2], want[2]), name
            assert bool(torch.isnan(got[1]).all()) and not bool(torch.isfinite(got[3]).any()), name
            assert bool(torch.isfinite(want).all())


def test_paths(G):
    """A sink kernel exists for complex frames of 256 .. 8192 points without an epilogue (path 1 with the hook at 1); it is the default where it measured faster
    than the composition (SINK_DEFAULT = the table of SPECTRUM_INTEGRATOR.md).  Everything else is the composition whatever the hook says; values with an
    epilogue are the composition's."""
    A = 33
    for N in SIZES:
        x, _, _ = case(N)
        xd = dev(x[:(A + 1) * N])
        for name, make, _, fused in entries(G, N):
            for path, want in ((0, default_path(N, name)), (1, 1 if N in SINK_SIZES else 2), (2, 2)):
                si = integ(G, N, A, path=path)
                fused(make(), xd, si)
                assert last_path(G, si) == want, (N, name, path)
    for N in (512, 2048, 4096):  # the sink sizes outside the table, one call each
        xd = dev(SO.signal((A + 1) * N, N))
        for name, make, mag2, fused in entries(G, N):
            two = G.SpectrumIntegrator(N, A).process_bulk(mag2(make(), xd))
            for path, want in ((0, default_path(N, name)), (1, 1), (2, 2)):
                si = integ(G, N, A, path=path)
                assert same(fused(make(), xd, si), two) and last_path(G, si) == want, (N, name, path)
    one = G.PolyphaseFilterBank(1024, 1)  # one tap per channel: the bank's sink is the default (no re-reads)
    si = G.SpectrumIntegrator(1024, A)
    one.power_integrated(dev(case(1024)[0][:(A + 1) * 1024]), si)
    assert last_path(G, si) == default_path(1024, "pfb1")
    N = 1024
    x, _, _ = case(N)
    xd = dev(x[:(A + 1) * N])
    fft, si = G.FFT(N, "Hann"), integ(G, N, A, path=1)
    fft.set_epilogue(G.Merged(torch.float32, [("Multiply", 1.0 / N), ("Add", 0.25)]))
    got = fft.power_integrated(xd, si)
    assert last_path(G, si) == 2
    assert same(got, G.SpectrumIntegrator(N, A).process_bulk(fft.mag2(xd)))
    real, si = G.FFT(N, "Hann", dtype=torch.float32), integ(G, N, A, path=1)
    xr = xd.real.contiguous()
    assert same(real.power_integrated(xr, si), G.SpectrumIntegrator(N, A).process_bulk(real.mag2(xr))) and last_path(G, si) == 2


def test_graph_planned_and_unplanned(G, tmp_path):
    """source -> PowerSpectrum(1024, Hann) | PfbPowerSpectrum(1024, P = 4) -> SpectrumIntegrator(33) -> sink on gpu:hip:0: hip::plan makes one fused stage of the
    pair (the kinds are EXPECTs of the program), unplanned two device blocks run; both give the bits of the Python entry"""
    assert os.path.exists(HOST_BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_spectrum_integrator.cpp and the plugin"
    prefix = str(tmp_path / "dev")
    r = subprocess.run([HOST_BIN, "device", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "spectrum integrator device: ok" in r.stdout and "FAIL" not in r.stdout
    assert "power_spectrum_integrated_c32" in r.stdout and "pfb_mag2_integrated_c32" in r.stdout
    N, A = 1024, 33
    xd = torch.from_numpy(np.fromfile(prefix + ".in", np.float32).view(np.complex64)).cuda()
    want = {"fft": G.FFT(N, "Hann").power_integrated(xd, G.SpectrumIntegrator(N, A)), "pfb": G.PolyphaseFilterBank(N, P).power_integrated(xd, G.SpectrumIntegrator(N, A))}
    for name, w in want.items():
        for how in ("planned", "seam"):
            got = np.fromfile(f"{prefix}.{name}.{how}", np.float32).reshape(-1, N)
            assert got.shape == (2, N) and np.array_equal(got.view(np.uint32), bits(w)), (name, how)


def test_refusals_leave_the_outputs_untouched(G):
    L = G.capi.lib()
    N, A = 1024, 2
    x, _, _ = case(N)
    xd = dev(x[:4 * N])
    before = xd.clone()
    out = torch.full((2, N), CANARY, dtype=torch.float32, device="cuda")
    fft, bank = G.FFT(N, "Hann"), G.PolyphaseFilterBank(N, P)
    for entry, first in ((L.gr4hip_fft_mag2_integrate, fft), (L.gr4hip_pfb_power_integrate, bank)):
        rc, n = _call(G, entry, first, G.SpectrumIntegrator(512, A), xd, 4, out)  # mismatched n_bins
        assert rc == G.capi.INVALID_ARGUMENT and n == 12345
        si = G.SpectrumIntegrator(N, A)
        inside = xd.view(torch.float32)[N:]  # the output inside the input
        rc, n = _call(G, entry, first, si, xd, 4, inside)
        assert rc == G.capi.INVALID_ARGUMENT and n == 12345 and si.pending(0) == 0 and si.pending(A) == 1
        rc, n = _call(G, entry, first, si, xd, 4, None)  # no output in a call that completes two integrations
        assert rc == G.capi.INVALID_ARGUMENT and n == 12345
    si = G.SpectrumIntegrator(N, A)
    m = fft.mag2(xd)
    keep = m.clone()
    rc, n = _call(G, L.gr4hip_specint_process, None, si, m, 4, m.reshape(-1)[N // 2:])
    assert rc == G.capi.INVALID_ARGUMENT and n == 12345
    rc, n = _call(G, L.gr4hip_specint_process, None, si, m, 0, None)  # no frames: a no-op
    assert rc == 0 and n == 0
    torch.cuda.synchronize()
    assert torch.equal(xd, before) and torch.equal(m, keep) and bool((out == CANARY).all())
