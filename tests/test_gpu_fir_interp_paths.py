"""gr4hip_fir_interp_process's dispatch (csrc/fir_interp.hip): which of its three kernels serves a call -- the register-window kernel fir_interp_kernel<L, R, S>,
the generic kernel, or the matrix-pipe kernel fir_interp_mfma_kernel<G, S> --, in which instantiation, grid and segments per workgroup, and whether the carried
history survives the tile edges inside a call and the hand-offs between calls.  Every call asserts the exact record of what it enqueued, read from the library's
test hook gr4hip_internal_fir_interp_last_path: a routing table here cannot go stale when a threshold moves.  Every call writes into a fresh allocation framed
by sentinels, which must stay as they were, like the input.

Truth is a float64 polyphase evaluation in numpy over the whole stream since the history last became zero (exact: the handle always holds at least Kp - 1
samples), pinned against the zero-stuffing oracle O.fir_interp at three small shapes.  The bar is the parity contract's 1e-5 (include/gr4hip.h) everywhere: the
longest sum of this file has 18200 terms per output, where a float32 evaluation in the kernel's order is 1.3e-6 from float64.

Every test is a PLAN (a list of steps on one handle); test_plans_reach_every_path_and_state_the_dispatch_rule walks all of them without running anything and
lists what the asserted records cover."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
MIN_OUT = 32768   # kIpMfmaMinOut: shorter spans stay off the matrix pipe
MAX_KS = 68       # kIpMaxKS: K-steps of the matrix-pipe form
ROW_MAX = 16384   # floats of its tap row in LDS: 4 KS L
LDS_MAX = 150 * 1024  # bytes of the register-window kernel's staged window
_R = {2: 4, 3: 4, 4: 2, 5: 2, 6: 2, 8: 2}  # the register-window kernel's instantiations: input positions per lane
NONE, WINDOW, GENERIC, MATRIX = 0, 1, 2, 3  # the record's kernel number
SENT, PAD = 0x4B1D5EED, 64  # sentinel word, and elements of it on either side of every output
NO_MFMA, SPW = "GR4HIP_INTERP_NO_MFMA", "GR4HIP_INTERP_SPW"


def SI(S):
    """inputs per segment of the matrix-pipe kernel"""
    return 4096 // S


def RIN(S, G):
    """inputs per round of a segment"""
    return 64 * (4 // S) * G


def _rel(got, truth):
    """THE parity metric (include/gr4hip.h, "PARITY CONTRACT"): max_k |got_k - truth_k| / max(|truth_k|, rms(truth))"""
    got = np.asarray(got).astype(np.complex128 if np.iscomplexobj(got) else np.float64).ravel()
    truth = np.asarray(truth).ravel()
    rms = np.sqrt(np.mean(np.abs(truth) ** 2))
    return float(np.max(np.abs(got - truth) / np.maximum(np.abs(truth), rms if rms > 0 else 1.0)))


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


# ------------------------------------------------------------------ the handle's decisions, restated (ip_upload, gr4hip_fir_interp_process)
def _cdiv(a, b):
    return -(-a // b)


def _form(L, K):
    """(KS, G) of ip_upload: KS = 0 where (L, K) has no matrix-pipe form"""
    Kp = _cdiv(K, L)
    pow2 = L in (2, 4, 8, 16)
    G_ = 16 // L if pow2 else 1
    if not (pow2 or L == 7 or L > 8):
        return 0, 1
    KS = _cdiv(Kp - 1 + G_, 4)
    if G_ == 8:
        KS += KS & 1
    return (KS, G_) if KS <= MAX_KS and 4 * KS * L <= ROW_MAX else (0, G_)


class _Model:
    """what the handle keeps between calls: taps, history capacity, and the process-wide switches the plan has set"""

    def __init__(self, L, S, K):
        self.L, self.S, self.hcap, self.sw = L, S, 32, {}
        self.set_taps(K)

    def set_taps(self, K):
        """-> True where the history is lost: it is replaced (zeroed) only when it has to grow"""
        self.K, self.Kp = K, _cdiv(K, self.L)
        self.KS, self.G = _form(self.L, K)
        lost = self.Kp > self.hcap
        if lost:
            self.hcap = 1 << (self.Kp - 1).bit_length()
        return lost

    def rule(self, n, yoff):
        """the kernel gr4hip_fir_interp_process picks"""
        if n == 0:
            return NONE
        if self.KS > 0 and n * self.L >= MIN_OUT and yoff == 0 and not self.sw.get(NO_MFMA):
            return MATRIX
        if self.L in _R and (self.Kp - 1 + 256 * _R[self.L]) * 4 * self.S <= LDS_MAX:
            return WINDOW
        return GENERIC

    def want(self, n, kernel):
        """the record of a call of n inputs that `kernel` serves"""
        if kernel == NONE:
            return (0, 0, self.KS, 0, 0, 0, 0, self.hcap)
        if kernel == MATRIX:
            nseg = _cdiv(n, SI(self.S))
            forced = self.sw.get(SPW, 0)
            spw = forced if 1 <= forced <= 4 else min(max(nseg // 2048, 1), 4)
            return (MATRIX, self.G, self.KS, spw, _cdiv(nseg, spw), _cdiv(self.L, 16) if self.G == 1 else 1, 1, self.hcap)
        if kernel == WINDOW:
            return (WINDOW, _R[self.L], self.KS, 0, _cdiv(n, 256 * _R[self.L]), 1, 0, self.hcap)
        return (GENERIC, 0, self.KS, 0, min(_cdiv(n * self.L, 256), 1 << 16), 1, 0, self.hcap)


# ------------------------------------------------------------------ plans: {id, L, K, cplx, taps, steps}
# steps: ("x", n, kernel expected[, yoff]) one call of the next n samples | ("reset",) | ("taps", K) set_taps on the live handle | ("sw", name, value)
def _plan(pid, L, K, cplx, steps, taps="rand"):
    return {"id": f"{pid}_{'c32' if cplx else 'f32'}", "L": L, "K": K, "cplx": cplx, "steps": steps, "taps": taps}


def _long(L, extra=0):
    """the shortest span the matrix pipe takes, plus `extra` inputs"""
    return _cdiv(MIN_OUT, L) + extra


def _walk(plan):
    """the plan without a device: [(n, yoff, kernel stated, kernel by the rule, record wanted)] of its calls"""
    m = _Model(plan["L"], 2 if plan["cplx"] else 1, plan["K"])
    out = []
    for st in plan["steps"]:
        if st[0] == "sw":
            m.sw[st[1]] = st[2]
        elif st[0] == "taps":
            m.set_taps(st[1])
        elif st[0] == "x":
            yoff = st[3] if len(st) > 3 else 0
            out.append((st[1], yoff, st[2], m.rule(st[1], yoff), m.want(st[1], st[2])))
    return out


def _taps(K, L, kind, seed):
    if kind == "lp" and K >= 8:
        return O.design_taps_hamming_lowpass(K, 0.4 / L)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(K) / np.sqrt(_cdiv(K, L))).astype(np.float32)  # every lag of the history weighs as much as any other


def _signal(cplx, n, seed):
    return (O.signal_c32 if cplx else O.signal_f32)(seed, n, tone_frel=0.03)


def _truth(b, x, L):
    """float64 polyphase evaluation from a zero history: y[p::L] = L convolve(x, b[p::L])"""
    n, Kp = len(x), _cdiv(len(b), L)
    b64 = np.zeros(Kp * L)
    b64[:len(b)] = np.asarray(b, np.float64)
    x64 = np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    y = np.empty(n * L, x64.dtype)
    for p in range(L):
        y[p::L] = L * np.convolve(x64, b64[p::L])[:n] if n else 0
    return y


def _record(G, f):
    fn = G.capi.lib().gr4hip_internal_fir_interp_last_path  # (test hook, not in include/gr4hip.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int)]
    rec = (C.c_int * 8)(*([-1] * 8))
    assert fn(f._h, rec) == 0
    return tuple(rec)


def _framed_call(f, xs, n_out, yoff):
    """one call whose output lies `yoff` elements past a 16-byte boundary of a fresh allocation of sentinels -> (output, what is wrong around it)"""
    w = 2 if np.iscomplexobj(xs) else 1  # 32-bit words per element
    host = np.full((n_out + 2 * PAD + 4) * w, SENT, np.uint32)
    buf = torch.from_numpy(host.view(np.int32)).cuda().view(f.dtype)
    out = buf[PAD + yoff:PAD + yoff + n_out]
    xin = torch.from_numpy(xs.copy()).cuda()
    assert (out.data_ptr() % 16 == 0) == (yoff == 0) and xin.data_ptr() % 16 == 0
    f.process_bulk(xin, out)
    words = buf.view(torch.int32).cpu().numpy().view(np.uint32)
    bad = []
    if not (np.all(words[:(PAD + yoff) * w] == SENT) and np.all(words[(PAD + yoff + n_out) * w:] == SENT)):
        bad.append("wrote outside [0, n_out)")
    if xin.cpu().numpy().tobytes() != xs.tobytes():
        bad.append("changed its input")
    return words[(PAD + yoff) * w:(PAD + yoff + n_out) * w].view(np.float32).view(xs.dtype).copy(), bad


def _run(G, devsw, plan):
    """execute a plan: every call framed, recorded and, per stretch of one tap set and one origin of the history, compared with the truth -> the whole output"""
    L, cplx = plan["L"], plan["cplx"]
    seed = 1000 * L + plan["K"] % 997 + cplx
    x = _signal(cplx, max(1, sum(st[1] for st in plan["steps"] if st[0] == "x")), seed)
    m = _Model(L, 2 if cplx else 1, plan["K"])
    b = _taps(plan["K"], L, plan["taps"], seed)
    f = G.fir_interpolator(b, L, torch.complex64 if cplx else torch.float32)
    pos, origin, first, ys, outs, seen, errs = 0, 0, 0, [], [], [], []

    def close():  # the stretch since `first`: one tap set, history zero at `origin`
        if pos > first:
            lo = max(origin, first - (_cdiv(len(b), L) - 1))
            truth = _truth(b, x[lo:pos], L)[(first - lo) * L:]
            y = np.concatenate(ys)
            errs.append((first, pos, len(b), _rel(y, truth) if y.shape == truth.shape else "shape"))
        ys.clear()

    for st in plan["steps"]:
        if st[0] == "sw":
            devsw(st[1], st[2])
            m.sw[st[1]] = st[2]
        elif st[0] == "reset":
            close()
            f.reset()
            origin = first = pos
        elif st[0] == "taps":
            close()
            b = _taps(st[1], L, plan["taps"], seed + st[1])
            f.settings_changed(b)
            first = pos
            if m.set_taps(st[1]):
                origin = pos
        else:
            n, kernel, yoff = st[1], st[2], st[3] if len(st) > 3 else 0
            y, bad = _framed_call(f, x[pos:pos + n], n * L, yoff)
            seen.append((pos, n, yoff, _record(G, f), m.want(n, kernel), bad))
            ys.append(y)
            outs.append(y)
            pos += n
    close()
    wrong = [s for s in seen if s[3] != s[4] or s[5]]
    over = [e for e in errs if e[3] == "shape" or e[3] > TOL]
    print(plan["id"], "stretches (first, end, taps, error):", errs)
    assert not wrong and not over, (plan["id"], "calls (pos, n, yoff, record, wanted, faults):", wrong, "stretches (first, end, taps, error):", errs)
    return np.concatenate(outs)


def _ids(plans):
    return [p["id"] for p in plans]


def _both(fn):
    """the plans of fn(cplx) for real and for complex data"""
    return [p for cplx in (False, True) for p in fn(cplx)]


# ------------------------------------------------------------------ the truth of this file against the zero-stuffing oracle
@pytest.mark.parametrize("L,K,n,cplx", [(2, 33, 3000, False), (7, 50, 2000, True), (16, 5, 1000, False)])
def test_polyphase_truth_is_the_zero_stuffing_oracle(L, K, n, cplx):
    b = _taps(K, L, "rand", L)
    x = _signal(cplx, n, K)
    want, _ = O.fir_interp(b, x, L)
    assert _rel(_truth(b, x, L), want) <= 1e-14  # two float64 sums of at most 17 terms in different orders


# ------------------------------------------------------------------ a. routing table: one case per kernel variant, the second call from a carried history
def _routes(cplx):
    S = 2 if cplx else 1
    out = []
    for L, R in _R.items():  # register-window: the tile edges TM = 256 R
        TM = 256 * R
        out.append(_plan(f"window_L{L}_tile_edges", L, 8 * L + 3, cplx, [("x", n, WINDOW) for n in (TM - 1, TM, TM + 1, 2 * TM + 5)], "lp"))
    for L in (3, 5, 6):  # no matrix-pipe form: long spans stay
        out.append(_plan(f"window_L{L}_long", L, 12 * L + 1, cplx, [("x", _long(L, 7), WINDOW), ("x", _long(L, 3000), WINDOW)], "lp"))
    for L in (1, 7, 9, 33):
        out.append(_plan(f"generic_L{L}_short", L, 6 * L + 1, cplx, [("x", 700, GENERIC), ("x", 291, GENERIC)], "lp"))
    for L in (2, 4, 8, 16, 7, 12, 17, 20, 48, 100):  # G = 8, 4, 2 and G = 1 with grid.y = 1, 1, 1, 2 (a last row block of one row), 2, 3, 7
        out.append(_plan(f"matrix_L{L}", L, 5 * L + 3, cplx, [("x", _long(L, 37), MATRIX), ("x", _long(L, SI(S) + 5), MATRIX)], "lp"))
    for L, lo in ((2, WINDOW), (16, GENERIC), (7, GENERIC)):  # n L >= 32768 exactly, and one input less
        out.append(_plan(f"threshold_L{L}", L, 6 * L, cplx, [("x", _long(L), MATRIX), ("x", _long(L) - 1, lo), ("x", _long(L), MATRIX)], "lp"))
    for L, lo in ((4, WINDOW), (16, GENERIC)):  # the matrix-pipe kernel ends on 16-byte stores
        out.append(_plan(f"misaligned_L{L}", L, 9 * L, cplx, [("x", _long(L, 100), lo, 1), ("x", _long(L, 100), MATRIX), ("x", _long(L, 9), lo, 1)], "lp"))
    for L, lo in ((8, WINDOW), (12, GENERIC)):
        out.append(_plan(f"no_mfma_L{L}", L, 9 * L, cplx, [("sw", NO_MFMA, 1), ("x", _long(L, 100), lo), ("x", _long(L, SI(S) + 3), lo),
                                                       ("sw", NO_MFMA, 0), ("x", _long(L, 1), MATRIX)], "lp"))
    return out


ROUTES = _both(_routes)


@pytest.mark.parametrize("plan", ROUTES, ids=_ids(ROUTES))
def test_routing_table(G, devsw, plan):
    _run(G, devsw, plan)


# ------------------------------------------------------------------ b. limits of the matrix-pipe form: K = Kp L taps on spans of 32768 outputs and a little more
# (L, Kp, kernel of a long span, KS, G)
_LIMITS = [
    (2, 265, MATRIX, 68, 8), (2, 266, WINDOW, 0, 8), (4, 269, MATRIX, 68, 4), (4, 270, WINDOW, 0, 4),          # KS <= 68
    (8, 271, MATRIX, 68, 2), (8, 272, WINDOW, 0, 2), (16, 272, MATRIX, 68, 1), (16, 273, GENERIC, 0, 1),
    (2, 1, MATRIX, 2, 8), (2, 2, MATRIX, 4, 8), (2, 5, MATRIX, 4, 8), (2, 6, MATRIX, 4, 8),                    # G = 8: KS is even
    (64, 256, MATRIX, 64, 1), (64, 257, GENERIC, 0, 1), (100, 160, MATRIX, 40, 1), (100, 161, GENERIC, 0, 1),  # 4 KS L <= 16384
    (4096, 4, MATRIX, 1, 1),                                                                                   # exactly 16384
]


def _limits(cplx):
    return [_plan(f"limit_L{L}_Kp{Kp}", L, Kp * L, cplx, [("x", _long(L), k), ("x", _long(L, 5), k)]) for L, Kp, k, _, _ in _LIMITS]


LIMITS = _both(_limits)


def test_limits_table_states_the_form():
    assert [_form(L, Kp * L) for L, Kp, _, _, _ in _LIMITS] == [(KS, G_) for _, _, _, KS, G_ in _LIMITS]
    assert 4 * 64 * 64 == ROW_MAX and 4 * 1 * 4096 == ROW_MAX and 4 * 40 * 100 <= ROW_MAX < 4 * 41 * 100


@pytest.mark.parametrize("plan", LIMITS, ids=_ids(LIMITS))
def test_limits_of_the_matrix_pipe_form(G, devsw, plan):
    _run(G, devsw, plan)


def _no_history(cplx):
    """Hq = 4 KS - G = 0: no sample in front of a block"""
    return [_plan(f"hq0_L{L}_K{K}", L, K, cplx, [("x", _long(L, 3), MATRIX), ("x", _long(L, SI(2 if cplx else 1) + 1), MATRIX)]) for L, K in ((2, 1), (2, 2), (4, 3), (4, 4))]


NO_HISTORY = _both(_no_history)


@pytest.mark.parametrize("plan", NO_HISTORY, ids=_ids(NO_HISTORY))
def test_matrix_pipe_without_history_in_front_of_a_block(G, devsw, plan):
    KS, G_ = _form(plan["L"], plan["K"])
    assert 4 * KS - G_ == 0
    _run(G, devsw, plan)


# ------------------------------------------------------------------ c. tile edges of the matrix-pipe kernel: segments, rounds, the G = 8 scalar tail store
def _edges(cplx):
    S = 2 if cplx else 1
    out = []
    for L, K in ((2, 64), (4, 37), (8, 256), (16, 256), (7, 128)):
        G_ = _form(L, K)[1]
        base = _cdiv(_long(L), SI(S)) * SI(S) + SI(S)
        ds = [-1, 0, 1, RIN(S, G_) - 1, RIN(S, G_), RIN(S, G_) + 1] + (list(range(2, 8)) if L == 2 else [])  # L = 2: every n_in % 8
        out.append(_plan(f"edges_L{L}_K{K}", L, K, cplx, [("x", base + d, MATRIX) for d in ds]))
    return out


EDGES = _both(_edges)


@pytest.mark.parametrize("plan", EDGES, ids=_ids(EDGES))
def test_matrix_pipe_tile_edges(G, devsw, plan):
    _run(G, devsw, plan)


# ------------------------------------------------------------------ d. segments per workgroup: the in-loop prefetch, at ten segments
_SPW_CASES = [(2, 64, False), (8, 256, True), (4, 37, True), (7, 128, False), (16, 256, True)]


def _spw_plans(L, K, cplx):
    n = 9 * SI(2 if cplx else 1) + 77
    return [_plan(f"spw{v}_L{L}", L, K, cplx, [("sw", SPW, v), ("x", n, MATRIX), ("x", n, MATRIX)]) for v in (0, 1, 2, 3, 4)]


@pytest.mark.parametrize("L,K,cplx", _SPW_CASES, ids=[f"L{c[0]}_{'c32' if c[2] else 'f32'}" for c in _SPW_CASES])
def test_segments_per_workgroup(G, devsw, L, K, cplx):
    """an output's MFMA chain does not depend on which workgroup staged its segment, nor on whether the segment came from the prefetch registers: the outputs
    under 1 .. 4 segments per workgroup are the same bits (and each meets the bar, second call included: the history is written under spw > 1 too)"""
    plans = _spw_plans(L, K, cplx)
    for p, v in zip(plans, (0, 1, 2, 3, 4)):
        recs = [w[4] for w in _walk(p)]
        assert all(r[0] == MATRIX and r[3] == max(v, 1) and r[4] == _cdiv(10, max(v, 1)) for r in recs), recs
    ys = [_run(G, devsw, p) for p in plans]
    assert all(y.tobytes() == ys[0].tobytes() for y in ys[1:])


# ------------------------------------------------------------------ e. history hand-offs on one handle
def _handoffs(_=None):
    out = []
    for L, K, cplx, lo in ((2, 530, True, WINDOW), (4, 1076, False, WINDOW), (8, 2168, False, WINDOW), (16, 256, True, GENERIC), (7, 128, False, GENERIC), (12, 100, True, GENERIC)):
        S, Kp, a = 2 if cplx else 1, _cdiv(K, L), _long(L)
        out.append(_plan(f"handoff_L{L}_K{K}", L, K, cplx, [
            ("x", a + SI(S) + 13, MATRIX),     # writes the next history itself
            ("x", 1, lo),                      # the carry launch: all but one sample of the history is old
            ("x", 0, NONE),
            ("x", Kp - 2, lo),                 # shorter than the history
            ("x", a + 7, MATRIX),              # its first segment stages a history mixed from three calls
            ("x", 300, lo),
            ("x", a + SI(S) + 1, lo, 1),       # a long span off the matrix pipe: the output is not on a 16-byte boundary
            ("x", a + 2 * SI(S) + 5, MATRIX),
            ("reset",),
            ("x", a + 11, MATRIX)]))
    # fewer inputs than history slots ON the matrix pipe (n L >= 32768 at n < hcap = 32): its new_hist mixes the old history and the span.  No later call at
    # these factors reads that far back (Kp - 1 <= 3 where 4 KS L <= 16384 holds), so the taps then grow within hcap -- off the matrix pipe -- and the next call
    # reads 29 samples of history, 13 of which an earlier matrix-pipe call carried over from the call before it.
    out.append(_plan("short_of_hcap_L2048", 2048, 5000, False, [("x", 16, MATRIX), ("x", 17, MATRIX), ("x", 3, GENERIC), ("x", 16, MATRIX), ("x", 31, MATRIX), ("x", 16, MATRIX),
                                                               ("taps", 30 * 2048), ("x", 4, GENERIC)]))
    out.append(_plan("short_of_hcap_L4096", 4096, 9000, True, [("x", 8, MATRIX), ("x", 9, MATRIX), ("x", 2, GENERIC), ("x", 12, MATRIX), ("x", 8, MATRIX),
                                                              ("taps", 30 * 4096), ("x", 3, GENERIC)]))
    return out


HANDOFFS = _handoffs()


@pytest.mark.parametrize("plan", HANDOFFS, ids=_ids(HANDOFFS))
def test_history_handoffs(G, devsw, plan):
    recs = [w[4] for w in _walk(plan)]
    assert all(r[6] == (r[0] == MATRIX) for r in recs) and {0, 1} <= {r[6] for r in recs}  # the matrix pipe writes the next history, the carry launch does otherwise
    if plan["L"] >= 2048:
        assert all(r[7] == 32 for r in recs) and all(w[0] < 32 for w in _walk(plan))
    _run(G, devsw, plan)


# ------------------------------------------------------------------ f. the register-window kernel's window past 150 KB of LDS
LDS_FALLBACK = _plan("window_over_150KB", 2, 36400, True, [("x", 350, GENERIC), ("x", 350, GENERIC)])


def test_lds_fallback_of_the_register_window_kernel(G, devsw):
    assert (18200 - 1 + 256 * _R[2]) * 8 == 153_784 > LDS_MAX  # H + TM complex samples: 184 B over
    assert all(w[4][0] == GENERIC and w[4][2] == 0 and w[4][7] == 32768 for w in _walk(LDS_FALLBACK))
    _run(G, devsw, LDS_FALLBACK)


# ------------------------------------------------------------------ g. set_taps on a live handle
_G_LONG, _G_SHORT = _long(4, SI(1) + 21), 500
# (K, kernel of the long call, KS, hcap): shrink (kept) | grow within hcap (kept: older samples in use) | beyond hcap (zeroed) | beyond it again, off the matrix pipe | back
_G_STEPS = [(64, MATRIX, 5, 32), (20, MATRIX, 2, 32), (120, MATRIX, 9, 32), (400, MATRIX, 26, 128), (1080, WINDOW, 0, 512), (64, MATRIX, 5, 512)]
SET_TAPS = _plan("set_taps_L4", 4, 64, False, [s for i, (K, k, _, _) in enumerate(_G_STEPS)
                                                for s in ([("taps", K)] if i else []) + [("x", _G_LONG, k), ("x", _G_SHORT, WINDOW)]])


def test_set_taps_on_a_live_handle(G, devsw):
    """the capacity only grows, to bit_ceil(Kp): 1080 taps (Kp = 270) take it from 128 to 512, where it stays"""
    recs = [w[4] for w in _walk(SET_TAPS)]
    assert [(r[2], r[7]) for r in recs] == [(KS, hcap) for _, _, KS, hcap in _G_STEPS for _ in range(2)]
    _run(G, devsw, SET_TAPS)


# ------------------------------------------------------------------ h. the C entry point
def test_c_entry_point_counts_and_null_pointers(G):
    L_, fn = 3, G.capi.lib().gr4hip_fir_interp_process
    f = G.fir_interpolator(_taps(10, L_, "rand", 1), L_)
    x, y, n_out = torch.ones(5, device="cuda"), torch.zeros(15, device="cuda"), C.c_size_t(77)
    assert fn(f._h, x.data_ptr(), 5, y.data_ptr(), C.byref(n_out), None) == 0 and n_out.value == 15 and _record(G, f)[0] == WINDOW
    assert fn(f._h, None, 0, None, C.byref(n_out), None) == 0 and n_out.value == 0 and _record(G, f) == (0, 0, 0, 0, 0, 0, 0, 32)
    n_out.value = 77
    bad = G.capi.INVALID_ARGUMENT
    assert fn(f._h, None, 5, y.data_ptr(), C.byref(n_out), None) == bad and n_out.value == 15
    assert fn(f._h, x.data_ptr(), 5, None, None, None) == bad and fn(f._h, None, 5, None, None, None) == bad
    torch.cuda.synchronize()
    assert float(y.sum()) != 0.0  # (the first call ran)


# ------------------------------------------------------------------ what the plans above cover
def _all_plans():
    return ROUTES + LIMITS + NO_HISTORY + EDGES + [p for c in _SPW_CASES for p in _spw_plans(*c)] + HANDOFFS + [LDS_FALLBACK, SET_TAPS]


def test_plans_reach_every_path_and_state_the_dispatch_rule():
    """every kernel 0 .. 3, every G in 8, 4, 2, 1 and every R for both element sizes, 1 .. 4 segments per workgroup, both ways of writing the next history -- each
    in a record that a test above asserts; and the kernel a plan states for a call is the one the dispatch rule, restated in _Model.rule, picks"""
    seen = set()
    for plan in _all_plans():
        S = 2 if plan["cplx"] else 1
        for n, yoff, stated, ruled, rec in _walk(plan):
            assert stated == ruled, (plan["id"], n, yoff, stated, ruled)
            seen.add((S, rec[0], rec[1], rec[3], rec[6]))
    for S in (1, 2):
        assert {k for s, k, _, _, _ in seen if s == S} == {NONE, WINDOW, GENERIC, MATRIX}
        assert {g for s, k, g, _, _ in seen if s == S and k == MATRIX} == {8, 4, 2, 1}
        assert {r for s, k, r, _, _ in seen if s == S and k == WINDOW} == {2, 4}
        assert {fl for s, _, _, _, fl in seen if s == S} == {0, 1}
    assert {(g, v) for _, k, g, v, _ in seen if k == MATRIX} >= {(g, v) for g in (8, 4, 2, 1) for v in (1, 2, 3, 4)}
    assert {v for s, k, _, v, _ in seen if k == MATRIX and s == 1} == {v for s, k, _, v, _ in seen if k == MATRIX and s == 2} == {1, 2, 3, 4}
