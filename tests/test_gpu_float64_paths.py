"""The float64 instantiations of csrc/f64.hip -- fir_filter<double> (direct kernel fir64_kernel<R>, matrix-pipe kernel fir64_mfma_kernel<KSC>), iir_filter<double, form>
(three passes), FFT<double> (per-frame radix-2 kernel fft64_kernel, half-size Stockham kernel fft64_r2c_kernel) and Rotator<complex<double>>: which kernel serves a
call, in which instantiation, grid and LDS size, and whether the values survive the tile edges inside a call and the hand-offs between calls.  Every FIR and FFT call
asserts the exact record of what it enqueued, read from the library's test hooks gr4hip_internal_fir64_last_path / gr4hip_internal_fft64_last_path, against the
dispatch rule restated here: a routing table here cannot go stale when a threshold moves.  (The IIR and the rotator have one route each.)  Every output is a view into a
larger allocation of a sentinel word, PAD elements of it on either side, which must stay as they were, like the input.

Truth is float64 numpy / scipy over the whole stream since the state last became zero; the bar is the float64 parity bar TOL64 = 1e-12 under the parity metric _rel
unless a test says otherwise.  Every test is a PLAN (a list of steps on one handle); test_plans_reach_every_path_and_state_the_dispatch_rule walks all of them without
running anything and lists what the asserted records cover."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL64 = 1e-12
SENT, PAD = 0x4B1D5EED, 64  # sentinel word, and elements of it on either side of every output
NONE, DIRECT, MATRIX = 0, 1, 2       # the FIR record's kernel number
RADIX2, STOCKHAM = 1, 2              # the FFT record's kernel number
MIN_N = 32768                        # shorter spans stay off the matrix pipe
SEG, SEG_PER_WG = 4096, 4            # kF64Seg, kF64SegPerWg
MAX_SPAN = 270_000                   # samples of a plan (the rotator's long span apart)


def _rel(got, truth):
    """THE parity metric (include/gr4hip.h, "PARITY CONTRACT"): max_k |got_k - truth_k| / max(|truth_k|, rms(truth))"""
    got = np.asarray(got).astype(np.complex128 if np.iscomplexobj(got) else np.float64).ravel()
    truth = np.asarray(truth).ravel()
    if got.shape != truth.shape:
        return float("inf")
    if truth.size == 0:
        return 0.0
    rms = np.sqrt(np.mean(np.abs(truth) ** 2))
    return float(np.max(np.abs(got - truth) / np.maximum(np.abs(truth), rms if rms > 0 else 1.0)))


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    G.capi.lib()
    return G


def _cdiv(a, b):
    return -(-a // b)


def _bit_ceil(n):
    return 1 << (n - 1).bit_length()


# ------------------------------------------------------------------ framed outputs
class _Framed:
    """n elements of `dtype`, `yoff` elements past a 16-byte boundary of a fresh allocation of sentinel words"""

    def __init__(self, n, dtype=torch.float64, yoff=0):
        self.w = 2 if dtype == torch.float64 else 4  # 32-bit words per element
        self.n, self.lo = n, PAD + yoff
        self.words = torch.full(((n + 2 * PAD + 2) * self.w,), SENT, dtype=torch.int32, device="cuda")
        self.view = self.words.view(dtype)[self.lo:self.lo + n]
        assert (self.view.data_ptr() % 16 == 0) == (yoff % 2 == 0 or dtype != torch.float64)

    def intact(self):
        a, b = self.lo * self.w, (self.lo + self.n) * self.w
        return bool((self.words[:a] == SENT).all()) and bool((self.words[b:] == SENT).all())

    def numpy(self):
        return self.view.cpu().numpy().copy()


def _dev_at(a, off=0):
    """a on the device, `off` elements past a 16-byte boundary"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(len(a) + 2, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    v = buf[off:off + len(a)]
    v.copy_(torch.from_numpy(a))
    return v


def _status(G, fn):
    with pytest.raises(G.capi.Gr4HipError) as e:
        fn()
    return e.value.status


# ================================================================== FIR
def _kp(K):
    return 64 if K <= 64 else 128 if K <= 128 else 256 if K <= 256 else _cdiv(K, 64) * 64


def _R(D):
    return 4 if D <= 8 else 2 if D <= 16 else 1


class _FirModel:
    """what the handle keeps between calls (fir64_upload) and what gr4hip_fir64_process decides from it"""

    def __init__(self, K, D):
        self.D, self.hcap = D, 32
        self.set_taps(K)

    def set_taps(self, K):
        """-> True where the history is lost: it is replaced (zeroed) only when it has to grow"""
        self.K, self.Kp = K, _kp(K)
        lost = K > self.hcap
        if lost:
            self.hcap = _bit_ceil(K)
        return lost

    def rule(self, n, yoff):
        if n == 0:
            return NONE
        return MATRIX if self.D == 1 and self.K > 16 and n >= MIN_N and yoff % 2 == 0 else DIRECT

    def want(self, n, kernel):
        """the record of a call of n inputs that `kernel` serves: (kernel, R | KSC, Kp, grid, LDS bytes, hcap, who wrote the next history, 0)"""
        if kernel == NONE:
            return (0, 0, self.Kp, 0, 0, self.hcap, 0, 0)
        if kernel == MATRIX:
            lds = ((SEG + self.Kp) // 16 * 18 + self.Kp + 32) * 8
            return (MATRIX, (self.Kp + 16) // 4 if self.Kp <= 256 else 0, self.Kp, _cdiv(_cdiv(n, SEG), SEG_PER_WG), lds, self.hcap, 1, 0)
        R = _R(self.D)
        return (DIRECT, R, self.Kp, _cdiv(n // self.D, 256 * R), (2 * self.K + (256 * R - 1) * self.D) * 8, self.hcap, 0, 0)


# steps: ("x", n, kernel expected[, yoff]) one call of the next n samples | ("reset",) | ("taps", K) settings_changed on the live handle
def _fir_plan(pid, K, D, steps):
    return {"id": pid, "K": K, "D": D, "steps": steps}


def _fir_walk(plan):
    """the plan without a device: [(n, yoff, kernel stated, kernel by the rule, record wanted)] of its calls"""
    m, out = _FirModel(plan["K"], plan["D"]), []
    for st in plan["steps"]:
        if st[0] == "taps":
            m.set_taps(st[1])
        elif st[0] == "x":
            yoff = st[3] if len(st) > 3 else 0
            out.append((st[1], yoff, st[2], m.rule(st[1], yoff), m.want(st[1], st[2])))
    return out


def _fir_taps(K, seed):
    return np.random.default_rng(seed).standard_normal(K) / np.sqrt(K)


def _fir_record(G, f):
    fn = G.capi.lib().gr4hip_internal_fir64_last_path  # (test hook, not in include/gr4hip.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int)]
    rec = (C.c_int * 8)(*([-1] * 8))
    assert fn(f._h, rec) == 0
    return tuple(rec)


def _fir_run(G, plan):
    """execute a plan: every call framed, recorded and, per stretch of one tap set and one origin of the history, compared with np.convolve over the stream"""
    K, D = plan["K"], plan["D"]
    seed = 7919 * K + D
    x = np.random.default_rng(seed + 1).standard_normal(max(1, sum(st[1] for st in plan["steps"] if st[0] == "x")))
    m, b = _FirModel(K, D), _fir_taps(K, seed)
    f = G.fir_filter(b, torch.float64, decimate=D)
    pos, origin, first, ys, seen, errs, ntap = 0, 0, 0, [], [], [], 0

    def close():  # the stretch since `first`: one tap set, history zero at `origin`
        if pos > first:
            lo = max(origin, first - (len(b) - 1))
            truth = np.convolve(x[lo:pos], b)[first - lo:pos - lo:D]
            errs.append((first, pos, len(b), _rel(np.concatenate(ys), truth)))
        ys.clear()

    for st in plan["steps"]:
        if st[0] == "reset":
            close()
            f.reset()
            origin = first = pos
        elif st[0] == "taps":
            close()
            ntap += 1
            b = _fir_taps(st[1], seed + 100 * ntap)
            f.settings_changed(b)
            first = pos
            if m.set_taps(st[1]):
                origin = pos
        else:
            n, kernel, yoff = st[1], st[2], st[3] if len(st) > 3 else 0
            xin, out = _dev_at(x[pos:pos + n]), _Framed(n // D, yoff=yoff)
            f.process_bulk(xin, out.view)
            bad = ([] if out.intact() else ["wrote outside [0, n_out)"]) + ([] if xin.cpu().numpy().tobytes() == x[pos:pos + n].tobytes() else ["changed its input"])
            seen.append((pos, n, yoff, _fir_record(G, f), m.want(n, kernel), bad))
            ys.append(out.numpy())
            pos += n
    close()
    wrong = [s for s in seen if s[3] != s[4] or s[5]]
    over = [e for e in errs if not e[3] <= TOL64]
    print(plan["id"], "stretches (first, end, taps, error):", errs)
    assert not wrong and not over, (plan["id"], "calls (pos, n, yoff, record, wanted, faults):", wrong, "stretches (first, end, taps, error):", errs)


def _ids(plans):
    return [p["id"] for p in plans]


# ------------------------------------------------------------------ a. the direct kernel: every R, one full workgroup, one lane over, one short of two
_DIRECT_K, _DIRECT_D = (1, 16, 17, 2048), (1, 8, 9, 16, 17, 32)


def _direct_plans():
    out = []
    for K in _DIRECT_K:
        for D in _DIRECT_D:
            T = 256 * _R(D)
            steps = [("x", 5 if D == 1 else D, DIRECT)] if K == 2048 else []  # a first call far shorter than hcap
            steps += [("x", c * D, DIRECT) for c in (1, 1, 3)]                # one history made of several calls
            steps += [("x", n_out * D, DIRECT) for n_out in (T, T + 1, 2 * T - 1)]
            out.append(_fir_plan(f"direct_K{K}_D{D}", K, D, steps))
    return out


DIRECT_PLANS = _direct_plans()


@pytest.mark.parametrize("plan", DIRECT_PLANS, ids=_ids(DIRECT_PLANS))
def test_fir_direct_kernel(G, plan):
    recs = [w[4] for w in _fir_walk(plan)]
    assert all(r[0] == DIRECT and r[1] == {1: 4, 8: 4, 9: 2, 16: 2, 17: 1, 32: 1}[plan["D"]] for r in recs)
    assert [r[3] for r in recs[-3:]] == [1, 2, 2]
    if plan["K"] == 2048 and plan["D"] == 8:
        assert recs[0][4] == 98240 > 64 * 1024  # the opt-in for more than 64 KiB of dynamic LDS
    _fir_run(G, plan)


def test_fir_refusals(G):
    assert _status(G, lambda: G.fir_filter(np.ones(4), torch.float64, decimate=33)) == G.capi.UNSUPPORTED
    f = G.fir_filter(np.ones(40), torch.float64, decimate=3)
    x = torch.ones(10, dtype=torch.float64, device="cuda")
    assert _status(G, lambda: f.process_bulk(x)) == G.capi.INVALID_ARGUMENT
    assert _fir_record(G, f) == (0, 0, 64, 0, 0, 64, 0, 0)  # a refused call enqueued nothing
    y = f.process_bulk(x[:9]).cpu().numpy()
    assert np.array_equal(y, [1.0, 4.0, 7.0]) and _fir_record(G, f)[:2] == (DIRECT, 4)
    n_out = C.c_size_t(77)
    assert G.capi.lib().gr4hip_fir64_process(f._h, None, 0, None, C.byref(n_out), None) == 0 and n_out.value == 0 and _fir_record(G, f) == (0, 0, 64, 0, 0, 64, 0, 0)


# ------------------------------------------------------------------ b. the matrix pipe: every K-loop, every n mod 4, one segment in the last workgroup, a ragged last segment
_MATRIX_N = (32768, 32769, 32770, 32771, 3 * 16384 - 1, 3 * 16384 + 4095)
# K: (KSC, Kp)
_MATRIX_K = {17: (20, 64), 64: (20, 64), 65: (36, 128), 128: (36, 128), 129: (68, 256), 256: (68, 256), 257: (0, 320), 320: (0, 320), 321: (0, 384), 1985: (0, 2048),
             2048: (0, 2048)}
MATRIX_PLANS = [_fir_plan(f"matrix_K{K}", K, 1, [("x", n, MATRIX) for n in _MATRIX_N]) for K in _MATRIX_K]


@pytest.mark.parametrize("plan", MATRIX_PLANS, ids=_ids(MATRIX_PLANS))
def test_fir_matrix_pipe(G, plan):
    recs = [w[4] for w in _fir_walk(plan)]
    assert all(r[:3] == (MATRIX,) + _MATRIX_K[plan["K"]] and r[6] == 1 for r in recs)
    assert [r[3] for r in recs] == [2, 3, 3, 3, 3, 4] == [_cdiv(_cdiv(n, 4096), 4) for n in _MATRIX_N]
    _fir_run(G, plan)


# ------------------------------------------------------------------ c. what falls through to the direct kernel
FALLTHROUGH_PLANS = [
    _fir_plan("fall_K16_n32768", 16, 1, [("x", 32768, DIRECT), ("x", 300, DIRECT)]),
    _fir_plan("fall_K17_n32767", 17, 1, [("x", 32767, DIRECT), ("x", 32768, MATRIX)]),
    _fir_plan("fall_K64_out_at_8_mod_16", 64, 1, [("x", 32768, DIRECT, 1), ("x", 32768, MATRIX), ("x", 32768 + 4099, DIRECT, 1)]),
    _fir_plan("fall_K64_D2_n65536", 64, 2, [("x", 65536, DIRECT), ("x", 600, DIRECT)]),
]


@pytest.mark.parametrize("plan", FALLTHROUGH_PLANS, ids=_ids(FALLTHROUGH_PLANS))
def test_fir_fall_through(G, plan):
    assert _fir_walk(plan)[0][4][0] == DIRECT
    _fir_run(G, plan)


# ------------------------------------------------------------------ d. hand-offs on one handle
_L = MIN_N + 77
HANDOFF_PLANS = [
    _fir_plan("handoff_matrix_direct_matrix", 100, 1, [("x", _L, MATRIX), ("x", 5, DIRECT), ("x", _L + SEG + 3, MATRIX), ("x", 1000, DIRECT), ("x", 0, NONE), ("x", _L, MATRIX)]),
    _fir_plan("handoff_reset", 100, 1, [("x", _L, MATRIX), ("x", 700, DIRECT), ("reset",), ("x", _L, MATRIX), ("reset",), ("x", 500, DIRECT), ("x", 500, DIRECT)]),
    _fir_plan("taps_same_length", 100, 1, [("x", 3000, DIRECT), ("taps", 100), ("x", 3000, DIRECT), ("x", _L, MATRIX), ("taps", 100), ("x", _L, MATRIX)]),
    _fir_plan("taps_grow_20_100", 20, 1, [("x", 3000, DIRECT), ("taps", 100), ("x", 3000, DIRECT), ("x", _L, MATRIX)]),
    _fir_plan("taps_shrink_100_20", 100, 1, [("x", 3000, DIRECT), ("taps", 20), ("x", 3000, DIRECT), ("x", _L, MATRIX)]),
    _fir_plan("taps_shrink_and_back_100_20_100", 100, 1, [("x", 3000, DIRECT), ("taps", 20), ("x", 3000, DIRECT), ("taps", 100), ("x", 3000, DIRECT), ("x", _L, MATRIX)]),
    _fir_plan("taps_between_matrix_calls_64_300_64", 64, 1, [("x", _L, MATRIX), ("taps", 300), ("x", _L, MATRIX), ("taps", 64), ("x", _L, MATRIX)]),
    _fir_plan("taps_shrink_decimating_100_20", 100, 8, [("x", 2400, DIRECT), ("taps", 20), ("x", 2400, DIRECT)]),
]
# plan: hcap of its calls, and at which "taps" steps (in order) the history is lost
_HANDOFF_FACTS = {"taps_same_length": ([128] * 4, [False, False]), "taps_grow_20_100": ([32, 128, 128], [True]), "taps_shrink_100_20": ([128] * 3, [False]),
                  "taps_shrink_and_back_100_20_100": ([128] * 4, [False, False]), "taps_between_matrix_calls_64_300_64": ([64, 512, 512], [True, False]),
                  "taps_shrink_decimating_100_20": ([128] * 2, [False])}


@pytest.mark.parametrize("plan", HANDOFF_PLANS, ids=_ids(HANDOFF_PLANS))
def test_fir_handoffs(G, plan):
    """settingsChanged replaces the HistoryBuffer only when the taps outgrow its capacity (time_domain_filter.hpp:38-42): the capacity only grows, a shorter tap
    set keeps the stream's history"""
    if plan["id"] in _HANDOFF_FACTS:
        hcaps, lost = _HANDOFF_FACTS[plan["id"]]
        m, got = _FirModel(plan["K"], plan["D"]), []
        for st in plan["steps"]:
            if st[0] == "taps":
                got.append(m.set_taps(st[1]))
        assert got == lost and [w[4][5] for w in _fir_walk(plan)] == hcaps
    if plan["id"] == "taps_between_matrix_calls_64_300_64":
        assert [w[4][1:3] for w in _fir_walk(plan)] == [(20, 64), (0, 320), (20, 64)]
    _fir_run(G, plan)


FIR_PLANS = DIRECT_PLANS + MATRIX_PLANS + FALLTHROUGH_PLANS + HANDOFF_PLANS


# ================================================================== FFT
FPB = lambda N: 8192 // N  # frames per workgroup of the Stockham kernel: 4096 complex points


def _fft_rule(N, aligned):
    return STOCKHAM if N >= 16 and aligned else RADIX2


def _fft_want(N, frames, kernel):
    """(kernel, grid, frames per workgroup, dynamic LDS bytes)"""
    if frames == 0:
        return (0, 0, 0, 0)
    return (STOCKHAM, _cdiv(frames, FPB(N)), FPB(N), 65536) if kernel == STOCKHAM else (RADIX2, frames, 1, 16 * N)


def _fft_plan(pid, N, window, frames, flags=0, kind="rand"):
    """one handle, the same samples twice: from a 16-byte-aligned pointer, then from one at 8 mod 16"""
    return {"id": pid, "N": N, "window": window, "frames": frames, "flags": flags, "kind": kind,
            "calls": [(0, _fft_rule(N, True)), (1, RADIX2)]}  # (input offset in doubles, kernel expected)


def _fft_walk(plan):
    return [(plan["frames"] * plan["N"], off, k, _fft_rule(plan["N"], off % 2 == 0), _fft_want(plan["N"], plan["frames"], k)) for off, k in plan["calls"]]


def _fft_record(G, f):
    fn = G.capi.lib().gr4hip_internal_fft64_last_path  # (test hook, not in include/gr4hip.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int)]
    rec = (C.c_int * 4)(*([-1] * 4))
    assert fn(f._h, rec) == 0
    return tuple(rec)


def _delta_ds(N):
    return [1] if N == 4 else [d for d in sorted({1, 3, N // 4 + 1}) if 2 * d < N - 2]


def _fft_input(plan):
    N, frames = plan["N"], plan["frames"]
    if plan["kind"] == "delta":  # x = delta[n - d] + 0.125 delta[n - d - 2], one frame per d
        x = np.zeros((frames, N))
        for i, d in enumerate(_delta_ds(N)):
            x[i, d], x[i, d + 2] = 1.0, 0.125
        return x.ravel()
    return np.random.default_rng(N + frames).standard_normal(frames * N) + np.cos(0.3 * np.arange(frames * N))


def _window(name, N):
    return np.ones(N) if name == "None" else O.window(O.WINDOWS.index(name), N, np.float64)


def _unwrap(ph):
    """unwrapPhase (fft_common.hpp:73-89), restated: each value is moved by whole turns until it is within pi of the unwrapped value before it"""
    out, pi = np.array(ph, np.float64), np.pi
    prev = out[0]
    for i in range(1, len(out)):
        cur = out[i]
        while cur - prev > pi:
            cur -= 2 * pi
        while cur - prev < -pi:
            cur += 2 * pi
        out[i] = prev = cur
    return out


def _fft_truth(x, N, window, flags):
    """FFT<double>::processBulk for real input (fft.hpp:147-171, 221-227) from numpy's float64 transform -> magnitude, phase, re, im of every frame, and X"""
    X = np.fft.fft(x.reshape(-1, N) * _window(window, N), axis=1)
    h = N // 2
    mag = np.abs(X[:, :h]) * 2 / N
    if flags & 1:
        with np.errstate(divide="ignore"):
            mag = np.where(mag > 0, 20 * np.log10(np.where(mag > 0, mag, 1.0)), -np.finfo(np.float64).max)
    ph = np.angle(X[:, :h])
    if flags & 4:
        ph = np.array([_unwrap(p) for p in ph])
    if flags & 2:
        ph = ph * 180.0 / np.pi
    return mag, ph, X[:, h:].real.copy(), X[:, h:].imag.copy(), X


def _fft_call(G, f, xin, frames, N, want=(True, True, True, True)):
    """gr4hip_fft64_process into four framed outputs (a null pointer where `want` says so) -> the outputs (None where not asked for), what is wrong around them"""
    outs = [_Framed(frames * (N // 2)) if w else None for w in want]
    before = xin.clone()
    rc = G.capi.lib().gr4hip_fft64_process(f._h, xin.data_ptr(), frames, *[o.view.data_ptr() if o else None for o in outs], torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    bad = [f"wrote outside output {i}" for i, o in enumerate(outs) if o and not o.intact()] + ([] if torch.equal(before, xin) else ["changed its input"])
    return [o.numpy().reshape(frames, N // 2) if o else None for o in outs], bad


def _fft_run(G, plan):
    """both calls of the plan -> [(kernel, magnitude, phase, re, im)]; asserts records, sentinels, and magnitude / re / im against the truth"""
    N, frames, flags = plan["N"], plan["frames"], plan["flags"]
    x = _fft_input(plan)
    mag, ph, re, im, X = _fft_truth(x, N, plan["window"], flags)
    f = G.FFT(N, plan["window"], outputInDb=bool(flags & 1), outputInDeg=bool(flags & 2), unwrapPhase=bool(flags & 4), dtype=torch.float64)
    res = []
    for off, kernel in plan["calls"]:
        xin = _dev_at(x, off)
        assert xin.data_ptr() % 16 == 8 * off
        o, bad = _fft_call(G, f, xin, frames, N)
        rec = _fft_record(G, f)
        assert rec == _fft_want(N, frames, kernel) and not bad, (plan["id"], off, rec, _fft_want(N, frames, kernel), bad)
        e = (_rel(o[2], re), _rel(o[3], im)) + ((_rel(o[0], mag),) if not flags & 1 else ())
        print(plan["id"], "kernel", kernel, "errors (re, im[, magnitude]):", e)
        assert max(e) <= TOL64, (plan["id"], kernel, e)
        res.append((kernel, o[0], o[1], o[2], o[3]))
    return res, (mag, ph, re, im, X)


def _circ(a, b):
    d = np.abs(a - b) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)  # +-pi is one point


# ------------------------------------------------------------------ e. sizes, frames per workgroup, windows
def _size_plans():
    out = []
    for window in ("None", "Hann", "BlackmanHarris"):
        for N in (2, 4, 8):
            out.append(_fft_plan(f"fft_N{N}_{window}", N, window, 5))
        for N in (64, 128, 256, 1024):
            out.append(_fft_plan(f"fft_N{N}_{window}", N, window, FPB(N) + 1))
        for N, fr in ((16, (511, 512, 513)), (4096, (1, 2, 3)), (8192, (1, 2, 3))):
            out += [_fft_plan(f"fft_N{N}_{window}_frames{k}", N, window, k) for k in fr]
    return out


SIZE_PLANS = _size_plans()


@pytest.mark.parametrize("plan", SIZE_PLANS, ids=_ids(SIZE_PLANS))
def test_fft_sizes_frames_windows(G, plan):
    """both kernels at every size: magnitude, Re and Im at TOL64; the phase within 1e-9 rad (+-pi one point) wherever the bin carries more than 1e-6 of the
    spectrum's peak (below that the phase of a rounding error is compared with the phase of another)"""
    res, (mag, ph, re, im, X) = _fft_run(G, plan)
    h = plan["N"] // 2
    big = np.abs(X[:, :h]) > 1e-6 * np.abs(X).max()
    for kernel, _, p, _, _ in res:
        assert not big.any() or _circ(p, ph)[big].max() <= 1e-9, (plan["id"], kernel)
    if plan["N"] == 8192:
        assert _fft_walk(plan)[1][4] == (RADIX2, plan["frames"], 1, 128 * 1024)  # the opt-in for 128 KiB of dynamic LDS


# ------------------------------------------------------------------ f. dB, degrees, unwrap: all eight combinations, every bin
FLAG_PLANS = [_fft_plan(f"flags{fl}_N{N}_{w}", N, w, len(_delta_ds(N)), fl, "delta") for N in (8, 64) for w in ("None", "Hann") for fl in range(8)]


def _delta_conditioning(N, window):
    """-> (margin of every raw phase step of the float64 DFT from +-pi, smallest bin / peak) over the delta frames of size N"""
    p = _fft_plan("", N, window, len(_delta_ds(N)), 0, "delta")
    X = _fft_truth(_fft_input(p), N, window, 0)[4][:, :N // 2]
    step = np.diff(np.angle(X), axis=1)
    return float(np.min(np.abs(np.abs(step) - np.pi))) if step.size else np.pi, float(np.min(np.abs(X) / np.abs(X).max(axis=1, keepdims=True)))


def test_delta_frames_are_well_conditioned():
    """x = delta[n - d] + 0.125 delta[n - d - 2]: for N = 4 .. 8192, with and without a Hann window, every raw phase step stays more than 1 rad from +-pi (no
    unwrap decision hangs on a rounding error).  Without a window every bin is at least 0.7 of the peak (7/9).  Under Hann the second delta can outweigh the first
    (d = 1: w[3] / w[1] -> 9, so 1 + 1.125 z^2 comes within 0.125 of zero): there a bin still carries more than 4e-4 of the peak, which puts the rounding of its
    phase and dB value at 1.1e-16 / 4e-4 = 3e-13, a factor 3000 inside the 1e-9 bars."""
    for N in (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192):
        for window in ("None", "Hann"):
            margin, floor = _delta_conditioning(N, window)
            assert margin > 1.0 and floor >= (0.7 if window == "None" else 4e-4), (N, window, margin, floor)


@pytest.mark.parametrize("plan", FLAG_PLANS, ids=_ids(FLAG_PLANS))
def test_fft_flags_one_at_a_time(G, plan):
    """every bin of every frame, none left out: phase within 1e-9 rad (x 180 / pi in degrees; without unwrap +-pi is one point), dB within 1e-9 dB, from both kernels"""
    margin, _ = _delta_conditioning(plan["N"], plan["window"])
    assert margin > 1.0
    res, (mag, ph, re, im, X) = _fft_run(G, plan)
    fl = plan["flags"]
    scale = 180.0 / np.pi if fl & 2 else 1.0
    for kernel, m, p, _, _ in res:
        if fl & 1:
            assert np.abs(m - mag).max() <= 1e-9, (plan["id"], kernel, np.abs(m - mag).max())
        err = np.abs(p - ph) if fl & 4 else _circ(p / scale, ph / scale) * scale
        assert err.max() <= 1e-9 * scale, (plan["id"], kernel, err.max())


@pytest.mark.parametrize("N", [8, 64])
@pytest.mark.parametrize("flags", [1, 7])
def test_fft_all_zero_frame(G, N, flags):
    """std::numeric_limits<double>::lowest() stands for -infinity dB (fft_common.hpp:40-44); atan2(0, 0) = 0"""
    x = np.random.default_rng(N).standard_normal(3 * N)
    x[N:2 * N] = 0.0
    f = G.FFT(N, "None", outputInDb=True, outputInDeg=bool(flags & 2), unwrapPhase=bool(flags & 4), dtype=torch.float64)
    for off in (0, 1):
        o, bad = _fft_call(G, f, _dev_at(x, off), 3, N)
        assert not bad and _fft_record(G, f)[0] == _fft_rule(N, off == 0)
        assert np.all(o[0][1] == -np.finfo(np.float64).max) and np.all(o[1][1] == 0.0) and np.all(o[2][1] == 0.0) and np.all(o[3][1] == 0.0)
        assert np.all(np.isfinite(o[0][[0, 2]])) and np.all(o[0][[0, 2]] > -400.0)


@pytest.mark.parametrize("N", [8, 64])
def test_fft_null_outputs_one_at_a_time(G, N):
    plan = _fft_plan("", N, "Hann", 3)
    x = _fft_input(plan)
    truth = _fft_truth(x, N, "Hann", 0)[:4]
    f = G.FFT(N, "Hann", dtype=torch.float64)
    for off in (0, 1):
        for skip in range(4):
            o, bad = _fft_call(G, f, _dev_at(x, off), 3, N, tuple(i != skip for i in range(4)))
            assert not bad and o[skip] is None and _fft_record(G, f) == _fft_want(N, 3, _fft_rule(N, off == 0))
            for i in range(4):
                if i != skip:
                    assert (_circ(o[i], truth[i]).max() <= 1e-9) if i == 1 else (_rel(o[i], truth[i]) <= TOL64), (N, off, skip, i)


@pytest.mark.parametrize("N", [8, 64])
def test_fft_ranges_frequency_and_refusals(G, N):
    x = _fft_input(_fft_plan("", N, "None", 4))
    blk = G.FFT(N, "None", outputInDb=True, dtype=torch.float64, sample_rate=48000.0)
    out = blk.process_bulk(_dev_at(x))
    rg = out["ranges"].cpu().numpy()
    assert rg.shape == (4, 4, 2)
    for i, k in enumerate(("magnitude", "phase", "re", "im")):
        v = out[k].cpu().numpy()
        assert np.array_equal(rg[:, i, 0], v.min(axis=1)) and np.array_equal(rg[:, i, 1], v.max(axis=1))
    assert np.array_equal(out["frequency"], np.arange(N // 2) * 48000.0 / N)
    assert "ranges" not in blk.process_bulk(_dev_at(x), ranges=False)
    for bad in (16384, 1000):
        assert _status(G, lambda: G.FFT(bad, "None", dtype=torch.float64)) == G.capi.UNSUPPORTED
    f = G.FFT(N, "None", dtype=torch.float64)
    assert G.capi.lib().gr4hip_fft64_process(f._h, None, 0, None, None, None, None, None) == 0 and _fft_record(G, f) == (0, 0, 0, 0)


FFT_PLANS = SIZE_PLANS + FLAG_PLANS


# ================================================================== IIR
IIR_SHAPES = [(4, 2), (1, 8), (8, 1)]
_IIR_N = (1, 31, 32, 33, 8191, 8192, 8193, 16 * 8192, 16 * 8192 + 1)  # a chunk is 32 samples, a tile 8192, a lane of the tile-level scan 16 tiles


def _draw_sections(nsec, order, seed):
    """stable random sections as in test_iir_filter_float64_every_instantiation (tests/test_gpu_parity.py): a draw with kappa = ||1 / A||_1 ||a||_1 > 100 is drawn again"""
    import scipy.signal as sps
    if (nsec, order, seed) in _SECTIONS:
        return tuple(v.copy() for v in _SECTIONS[(nsec, order, seed)])
    rng = np.random.default_rng(seed)
    b, a = [], []
    impulse = np.zeros(4000)
    impulse[0] = 1.0
    for _ in range(nsec):
        while True:
            poles = []
            while len(poles) < order:
                if order - len(poles) >= 2:
                    r, th = rng.uniform(0.3, 0.95), rng.uniform(0.1, 3.0)
                    poles += [r * np.exp(1j * th), r * np.exp(-1j * th)]
                else:
                    poles += [rng.uniform(-0.95, 0.95)]
            aa, bb = np.real(np.poly(poles)), rng.uniform(-1, 1, order + 1) * 0.5
            if np.sum(np.abs(sps.lfilter([1.0], aa, impulse))) * np.sum(np.abs(aa)) <= 100.0:
                break
        a.append(aa)
        b.append(bb)
    _SECTIONS[(nsec, order, seed)] = (np.array(b), np.array(a))
    return np.array(b), np.array(a)


_SECTIONS = {}


def _iir_truth(b, a, x):
    import scipy.signal as sps
    y = np.asarray(x, np.float64)
    for bb, aa in zip(b, a):
        y = sps.lfilter(bb, np.concatenate([[1.0], aa[1:]]), y)  # a[0] is taken as 1
    return y


# steps: ("x", n) | ("reset",); coef: "full" | "b_short" (b has one coefficient less than a) | "a_short" (a has one less than b)
def _iir_plan(pid, shape, steps, coef="full"):
    return {"id": pid, "shape": shape, "steps": steps, "coef": coef}


def _iir_coefficients(plan):
    nsec, order = plan["shape"]
    if plan["coef"] == "a_short":  # poles of order - 1, numerator of order
        b, _ = _draw_sections(nsec, order, 100 * nsec + order)
        _, a = _draw_sections(nsec, order - 1, 100 * nsec + order + 1)
        return b, a
    b, a = _draw_sections(nsec, order, 100 * nsec + order)
    return (b[:, :-1].copy(), a) if plan["coef"] == "b_short" else (b, a)


def _iir_run(G, plan, form=1):
    """execute a plan: every call framed and, per stretch since the state became zero, compared with scipy's lfilter section by section -> the whole output"""
    b, a = _iir_coefficients(plan)
    total = sum(st[1] for st in plan["steps"] if st[0] == "x")
    x = np.random.default_rng(total + plan["shape"][0]).standard_normal(total)
    f = G.iir_filter(b, a, form=form, dtype=torch.float64)
    pos, origin, ys, outs, errs, bad = 0, 0, [], [], [], []

    def close():
        if pos > origin:
            errs.append((origin, pos, _rel(np.concatenate(ys), _iir_truth(b, a, x[origin:pos]))))
        ys.clear()

    for st in plan["steps"]:
        if st[0] == "reset":
            close()
            f.reset()
            origin = pos
        else:
            n = st[1]
            xin, out = _dev_at(x[pos:pos + n]), _Framed(n)
            f.process_bulk(xin, out.view)
            if not out.intact():
                bad.append((pos, n, "wrote outside [0, n)"))
            if xin.cpu().numpy().tobytes() != x[pos:pos + n].tobytes():
                bad.append((pos, n, "changed its input"))
            ys.append(out.numpy())
            outs.append(ys[-1])
            pos += n
    close()
    print(plan["id"], "stretches (first, end, error):", errs)
    assert not bad and all(e[2] <= TOL64 for e in errs), (plan["id"], bad, errs)
    return np.concatenate(outs)


def _sid(shape):
    return f"{shape[0]}x{shape[1]}"


IIR_EDGE_PLANS = [_iir_plan(f"iir_{_sid(s)}_n{n}_{'one' if c == 1 else 'two'}", s, [("x", n)] * c) for s in IIR_SHAPES for n in _IIR_N for c in (1, 2)]
IIR_STREAM_PLANS = [p for s in IIR_SHAPES for p in (
    _iir_plan(f"iir_{_sid(s)}_forty_single_samples", s, [("x", 1)] * 40),
    _iir_plan(f"iir_{_sid(s)}_reset", s, [("x", 8192 + 5), ("x", 33), ("reset",), ("x", 31), ("x", 8193), ("reset",), ("x", 1), ("x", 64)]))]
IIR_COEF_PLANS = [_iir_plan(f"iir_{_sid(s)}_{c}", s, [("x", 8192 + 33), ("x", 31), ("x", 8192)], c) for s in ((4, 2), (1, 8), (2, 3)) for c in ("b_short", "a_short")]
IIR_PLANS = IIR_EDGE_PLANS + IIR_STREAM_PLANS + IIR_COEF_PLANS


@pytest.mark.parametrize("plan", IIR_EDGE_PLANS, ids=_ids(IIR_EDGE_PLANS))
def test_iir_span_edges(G, plan):
    """spans that end one sample before, on and after a chunk edge, a tile edge and the edge of a scan lane's 16 tiles; as one call, and as two calls of that
    length (the second one starts from a state that was written on the edge)"""
    _iir_run(G, plan)


@pytest.mark.parametrize("plan", IIR_STREAM_PLANS + IIR_COEF_PLANS, ids=_ids(IIR_STREAM_PLANS + IIR_COEF_PLANS))
def test_iir_streams_and_coefficient_padding(G, plan):
    b, a = _iir_coefficients(plan)
    assert (b.shape[1] - a.shape[1]) == {"full": 0, "b_short": -1, "a_short": 1}[plan["coef"]]
    _iir_run(G, plan)


@pytest.mark.parametrize("shape", IIR_SHAPES, ids=[_sid(s) for s in IIR_SHAPES])
def test_iir_forms_are_one_evaluation(G, shape):
    plan = _iir_plan(f"iir_{_sid(shape)}_forms", shape, [("x", 8192 + 33), ("x", 77)])
    ys = [_iir_run(G, plan, form) for form in range(4)]
    assert all(y.tobytes() == ys[0].tobytes() for y in ys[1:])
    b, a = _iir_coefficients(plan)
    assert _status(G, lambda: G.iir_filter(b, a, form=4, dtype=torch.float64)) == G.capi.INVALID_ARGUMENT


def test_iir_refusals(G):
    assert _status(G, lambda: G.iir_filter([[0.5]], [[1.0]], dtype=torch.float64)) == G.capi.UNSUPPORTED        # order 0
    assert _status(G, lambda: G.iir_filter(np.ones((3, 4)), np.ones((3, 4)), dtype=torch.float64)) == G.capi.UNSUPPORTED  # 9 state values
    assert _status(G, lambda: G.iir_filter(np.ones((1, 10)), np.ones((1, 10)), dtype=torch.float64)) == G.capi.UNSUPPORTED  # order 9


@pytest.mark.parametrize("shape", IIR_SHAPES, ids=[_sid(s) for s in IIR_SHAPES])
def test_iir_in_place_is_refused_and_the_stream_goes_on(G, shape):
    """the passes read the input through __restrict__ pointers while other workgroups write the output: out = x, and ranges that share one element, are
    refused; the refused call moved nothing, so the next valid call continues the stream"""
    plan = _iir_plan("", shape, [("x", 8192 + 100)])
    b, a = _iir_coefficients(plan)
    n1, m = 5000, 3292
    x = np.random.default_rng(9).standard_normal(n1 + m)
    truth = _iir_truth(b, a, x)
    f = G.iir_filter(b, a, dtype=torch.float64)
    y1 = f.process_bulk(_dev_at(x[:n1])).cpu().numpy()
    buf = torch.zeros(2 * m - 1, dtype=torch.float64, device="cuda")
    buf[:m].copy_(torch.from_numpy(x[n1:]))
    xin = buf[:m]
    assert _status(G, lambda: f.process_bulk(xin, xin)) == G.capi.INVALID_ARGUMENT
    assert _status(G, lambda: f.process_bulk(xin, buf[m - 1:])) == G.capi.INVALID_ARGUMENT   # the last input is the first output
    buf[m - 1:].copy_(torch.from_numpy(x[n1:]))
    assert _status(G, lambda: f.process_bulk(buf[m - 1:], buf[:m])) == G.capi.INVALID_ARGUMENT  # the last output is the first input
    assert np.array_equal(buf[m - 1:].cpu().numpy(), x[n1:])  # nothing ran
    out = _Framed(m)
    f.process_bulk(buf[m - 1:], out.view)
    assert out.intact() and _rel(np.concatenate([y1, out.numpy()]), truth) <= TOL64


# ================================================================== Rotator
LD = np.longdouble
ROT_INCS = (1e-3, 0.37, -2.5)
ROT_LONG = (1 << 24) + (1 << 20) + 333


def _two_pi_ld():
    return 8 * np.arctan(LD(1))


def _rot_phase(phase0, inc, k):
    """phase0 + k inc in long double, reduced to [0, 2 pi) there, rounded once to double"""
    ph = LD(phase0) + np.asarray(k).astype(LD) * LD(inc)
    two_pi = _two_pi_ld()
    return (ph - two_pi * np.floor(ph / two_pi)).astype(np.float64)


def _rot_truth(x, phase0, inc, k0):
    """y[i] = x[i] e^{i (phase0 + (k0 + i + 1) inc)} (Rotator.hpp:51-61 with the accumulated phase in closed form)"""
    ph = _rot_phase(phase0, inc, np.arange(k0 + 1, k0 + 1 + len(x), dtype=np.int64))
    return x * (np.cos(ph) + 1j * np.sin(ph))


def _rot_bar(phase0, inc, n_total):
    """The bar on |y - truth| / |x|, derived from the kernel's three rounding points, not measured.  With P = |phase0| + |inc| n_total, the largest phase the
    handle forms: (1) fma(hi, inc, phase0) rounds a value of at most P: 2^-53 P; (2) the product two_pi * floor(ph / two_pi) rounds a value of at most P:
    2^-53 P, and the double two_pi it is formed with is 2.45e-16 off 2 pi, floor(..) <= P / 2 pi times: 0.35 x 2^-53 P; (3) fma(lo, inc, ph) rounds a value of
    at most P + 2 pi: 2^-53 (P + 2 pi).  Together less than 4 x 2^-53 (P + 2 pi).  The 1e-12 on top holds sincos, the complex multiply-add and the rounding of
    the truth's own phase (1e-15 together), and the carried phase of a handle that is called many times: the host forms it with the same fma and product, at
    most two roundings per call of values below 2 pi + |inc| n_call (one where floor(..) <= 1: the product is exact), 2 x 2^-53 (2 pi c + |inc| n_total) over c
    calls.  For the 1000 calls of 97 samples of this file that is 5.5e-11, 9.4e-12 and 7e-13 at inc = -2.5, 0.37 and 1e-3, inside the bar's 1.08e-10, 1.7e-11
    and 1.05e-12."""
    return 4 * 2.0 ** -53 * (abs(phase0) + abs(inc) * n_total + 2 * np.pi) + 1e-12


needs_ld = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="the truth needs a long double of 64 bits of mantissa")


def _rot_x(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


# steps: ("x", n) | ("phase", p) settings_changed(initial_phase)
def _rot_plan(pid, inc, phase0, steps):
    return {"id": pid, "inc": inc, "phase0": phase0, "steps": steps}


def _rot_run(G, plan):
    """every call into its slice of ONE framed output; per stretch since the phase was last set, |y - truth| / |x| against the derived bar"""
    inc, phase0 = plan["inc"], plan["phase0"]
    total = sum(st[1] for st in plan["steps"] if st[0] == "x")
    x = _rot_x(total, total)
    xin, out = _dev_at(x), _Framed(total, torch.complex128)
    r = G.Rotator(phase_increment=inc, initial_phase=phase0, dtype=torch.complex128)
    pos, start, stretches = 0, 0, []
    for st in plan["steps"]:
        if st[0] == "phase":
            stretches.append((start, pos, phase0))
            phase0, start = st[1], pos
            r.settings_changed(phase0)
        else:
            r.process_bulk(xin[pos:pos + st[1]], out.view[pos:pos + st[1]])
            pos += st[1]
            assert 0.0 <= r.accumulated_phase < 2 * np.pi
    stretches.append((start, pos, phase0))
    assert out.intact() and xin.cpu().numpy().tobytes() == x.tobytes()
    y = out.numpy()
    errs = []
    for lo, hi, p0 in stretches:
        if hi > lo:
            e = float(np.max(np.abs(y[lo:hi] - _rot_truth(x[lo:hi], p0, inc, 0)) / np.abs(x[lo:hi])))
            errs.append((lo, hi, e, _rot_bar(p0, inc, hi - lo)))
    lo, hi, p0 = stretches[-1]
    want = float(_rot_phase(p0, inc, hi - lo))
    d = abs(r.accumulated_phase - want)
    print(plan["id"], "stretches (first, end, error, bar):", errs, "carried phase off by", min(d, 2 * np.pi - d))
    assert all(e[2] <= e[3] for e in errs), (plan["id"], errs)
    assert min(d, 2 * np.pi - d) <= _rot_bar(p0, inc, hi - lo)
    return y


ROT_PLANS = [_rot_plan(f"rot_inc{inc}_n{n}", inc, 0.25, [("x", n), ("x", n)]) for inc in ROT_INCS for n in (1, 255, 256, 257)]
ROT_PLANS += [_rot_plan(f"rot_inc{inc}_phase_set_in_mid_stream", inc, 0.25, [("x", 700), ("x", 300), ("phase", 1.75), ("x", 513), ("phase", -3.0), ("x", 257)]) for inc in ROT_INCS]
ROT_MANY = [(_rot_plan(f"rot_inc{inc}_1000_calls_of_97", inc, 0.25, [("x", 97)] * 1000), _rot_plan(f"rot_inc{inc}_one_call_of_97000", inc, 0.25, [("x", 97000)])) for inc in ROT_INCS]


@needs_ld
@pytest.mark.parametrize("plan", ROT_PLANS, ids=_ids(ROT_PLANS))
def test_rotator_short_spans_and_phase_changes(G, plan):
    _rot_run(G, plan)


@needs_ld
@pytest.mark.parametrize("many,one", ROT_MANY, ids=[m["id"] for m, _ in ROT_MANY])
def test_rotator_many_calls_against_one(G, many, one):
    """(see _rot_bar) both meet the bar against the truth, so they are within two bars of each other"""
    ya, yb = _rot_run(G, many), _rot_run(G, one)
    x = _rot_x(97000, 97000)
    assert float(np.max(np.abs(ya - yb) / np.abs(x))) <= 2 * _rot_bar(0.25, many["inc"], 97000)


def test_rotator_identity_bit_for_bit(G):
    x = _rot_x(70_001, 3)
    out = _Framed(len(x), torch.complex128)
    r = G.Rotator(phase_increment=0.0, initial_phase=0.0, dtype=torch.complex128)
    r.process_bulk(_dev_at(x), out.view)
    assert out.intact() and out.numpy().tobytes() == x.tobytes() and r.accumulated_phase == 0.0


@needs_ld
@pytest.mark.parametrize("inc", ROT_INCS)
def test_rotator_grid_stride_second_trip(G, inc):
    """the grid is capped at 65536 workgroups of 256 lanes: sample 2^24 is the first that a lane reaches on its second trip.  One span of 2^24 + 2^20 + 333
    samples, made on the device; three slices come back: the head with the index split at k = 2^20, 2^24 +- 4096, and the tail.  Bar: _rot_bar."""
    n, phase0 = ROT_LONG, 0.25
    assert _cdiv(n, 256) > 1 << 16
    g = torch.Generator(device="cuda").manual_seed(17)
    xin = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float64, device="cuda", generator=g))
    before = xin.clone()
    out = _Framed(n, torch.complex128)
    r = G.Rotator(phase_increment=inc, initial_phase=phase0, dtype=torch.complex128)
    r.process_bulk(xin, out.view)
    assert out.intact() and torch.equal(before, xin)
    bar, errs = _rot_bar(phase0, inc, n), []
    for lo, hi in ((0, (1 << 20) + 4096), ((1 << 24) - 4096, (1 << 24) + 4096), (n - 4096, n)):
        x, y = xin[lo:hi].cpu().numpy(), out.view[lo:hi].cpu().numpy()
        errs.append(float(np.max(np.abs(y - _rot_truth(x, phase0, inc, lo)) / np.abs(x))))
    print("rotator long span, inc", inc, "errors of the three slices:", errs, "bar", bar)
    assert max(errs) <= bar, (errs, bar)
    d = abs(r.accumulated_phase - float(_rot_phase(phase0, inc, n)))
    assert 0.0 <= r.accumulated_phase < 2 * np.pi and min(d, 2 * np.pi - d) <= bar


# ================================================================== the truths of this file against the oracle's
@pytest.mark.parametrize("shape,n", [((4, 2), 3000), ((1, 8), 2000), ((8, 1), 1000)])
def test_iir_truth_is_the_oracle(shape, n):
    b, a = _draw_sections(*shape, 100 * shape[0] + shape[1])
    x = O.signal_f32(shape[0], n)  # (the oracle takes float32 samples)
    want = O.iir_cascade(O.make_sections(list(zip(b, a))), x, O.DF_II, f64=True)
    # two float64 evaluations (direct form II here, transposed in lfilter) of up to 8 sections, each eps x kappa <= 1.1e-14 off: 16 x 1.1e-14
    assert _rel(_iir_truth(b, a, x.astype(np.float64)), want) <= 2e-13


@needs_ld
@pytest.mark.parametrize("inc,phase0,n", [(1e-3, 0.25, 4096), (0.37, 0.0, 1000), (-2.5, 1.5, 2000)])
def test_rotator_truth_is_the_oracle(inc, phase0, n):
    x = _rot_x(n, n)
    # the float64 recurrence: per step the sum and the wrap each round a value below 16 (2^-53 x 8 each), and the wrap's double 2 pi is 2.45e-16 off
    want, _ = O.rotator(x, inc, phase0)
    assert float(np.max(np.abs(_rot_truth(x, phase0, inc, 0) - want) / np.abs(x))) <= n * 2.0 ** -53 * 20 + 1e-14


@pytest.mark.parametrize("N,window", [(8, "None"), (64, "Hann"), (256, "BlackmanHarris")])
def test_fft_truth_is_the_oracle(N, window):
    x = _fft_input(_fft_plan("", N, window, 1))
    mag, ph, re, im, X = _fft_truth(x, N, window, 0)
    want = O.dft64(x * _window(window, N))  # the O(N^2) float64 DFT
    assert _rel(X[0], want) <= 1e-13
    assert _rel(mag[0], O.magnitude(want, half=True)) <= 1e-13 and _rel(re[0], want[N // 2:].real) <= 1e-13
    p = _fft_plan("", N, "None", len(_delta_ds(N)), 6, "delta")  # unwrapped degrees, on frames whose unwrap is well conditioned
    xd = _fft_input(p)
    got = _fft_truth(xd, N, "None", 6)[1]
    for i in range(p["frames"]):
        assert np.abs(got[i] - O.phase(O.dft64(xd[i * N:(i + 1) * N]), half=True, in_deg=True, unwrap=True)).max() <= 1e-9


# ================================================================== what the plans above cover
def test_plans_reach_every_path_and_state_the_dispatch_rule():
    """both FIR kernels with every R and every K-loop, both ways of writing the next history, both FFT kernels, the 98 KiB and 128 KiB LDS opt-ins -- each in a
    record that a test above asserts; and the kernel a plan states for a call is the one the dispatch rule, restated in _FirModel.rule / _fft_rule, picks"""
    seen = set()
    for plan in FIR_PLANS:
        for n, yoff, stated, ruled, rec in _fir_walk(plan):
            assert stated == ruled == rec[0], (plan["id"], n, yoff, stated, ruled)
            seen.add(("fir", rec[0], rec[1], rec[6]))
    assert {(k, r) for t, k, r, _ in seen if k == DIRECT} == {(DIRECT, 1), (DIRECT, 2), (DIRECT, 4)}
    assert {r for t, k, r, _ in seen if k == MATRIX} == {20, 36, 68, 0}
    assert {(k, w) for t, k, _, w in seen} == {(NONE, 0), (DIRECT, 0), (MATRIX, 1)}
    assert any(w[4][0] == DIRECT and w[4][4] > 64 * 1024 for p in FIR_PLANS for w in _fir_walk(p))
    kernels, lds = set(), set()
    for plan in FFT_PLANS:
        for n, off, stated, ruled, rec in _fft_walk(plan):
            assert stated == ruled == rec[0], (plan["id"], off, stated, ruled)
            kernels.add((rec[0], plan["N"]))
            lds.add(rec[3])
    assert {k for k, _ in kernels} == {RADIX2, STOCKHAM} and 128 * 1024 in lds
    assert {N for k, N in kernels if k == RADIX2} >= {2, 4, 8, 16, 64, 128, 256, 1024, 4096, 8192}
    assert {N for k, N in kernels if k == STOCKHAM} == {16, 64, 128, 256, 1024, 4096, 8192}


def plan_sizes():
    """[(plan id, samples)] of every plan of this file (the rotator's long span apart)"""
    out = [(p["id"], sum(w[0] for w in _fir_walk(p))) for p in FIR_PLANS]
    out += [(p["id"], p["frames"] * p["N"]) for p in FFT_PLANS]
    out += [(p["id"], sum(st[1] for st in p["steps"] if st[0] == "x")) for p in IIR_PLANS + ROT_PLANS + [q for pair in ROT_MANY for q in pair]]
    return out
