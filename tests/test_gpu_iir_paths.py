"""gr4hip_iir_process's dispatch (csrc/iir.hip, iir_run; the float64 cascade of csrc/f64.hip is in test_gpu_parity.py): which kernel serves a call -- the
segment-sequential runs (iir_seq_kernel), the look-back single pass (iir_onepass_kernel), the three passes (iir_pass_z / b / y) or the sequential float32 form --,
in which instantiation, with which warm-up and run length, and whether the carried state survives the tile edges inside a call and the hand-offs between calls.
Every call asserts the exact record of what it enqueued, read from the library's test hook gr4hip_internal_iir_last_path: a routing table here cannot go stale
when a threshold moves.  Every result is compared with the float64 oracle under the parity contract's bar (include/gr4hip.h): 1e-5 where the reference's own
float32 cascade stays within 3e-6 of float64 on the test signal (test_table_filters_are_what_the_table_says checks that without a GPU), and
max(1e-5, 3 x that float32 error) for the cascades with a pole close to the unit circle (the bar of test_iir_random_cascades).  Two parallel kernels on the same
stream agree within 2e-5 of the output rms."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5
REF32_OK = 3e-6  # a table filter that is not marked slow: the reference's float32 cascade is this close to float64
PAIR = 2e-5      # two parallel kernels on one stream, relative to the output rms
TILE = 8192      # kIirBS chunks of kIirL samples
CHUNK, CHUNKS = 32, 256
SEQ, LOOKBACK, THREE, SEQ_F32 = 1, 2, 3, 4  # the record's kernel number


def _rel(got, truth):
    """THE parity metric (include/gr4hip.h, "PARITY CONTRACT"): max_k |got_k - truth_k| / max(|truth_k|, rms(truth))"""
    got = np.asarray(got).astype(np.float64).ravel()
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


# ------------------------------------------------------------------ the cascades of this file
def _f32(secs):
    """sections as the handle sees them: float32 coefficients, (b[nsec][nb], a[nsec][na])"""
    return np.array([s[0] for s in secs], np.float32), np.array([s[1] for s in secs], np.float32)


def _bq(r, th, b=(0.2, 0.3, 0.2)):
    return np.array(b, np.float64), np.array([1.0, -2 * r * np.cos(th), r * r])


def _o4(r1, th1, r2, th2, b=(0.1, 0.2, 0.3, 0.2, 0.1)):
    return np.array(b, np.float64), np.convolve(_bq(r1, th1)[1], _bq(r2, th2)[1])


def _pole(p):
    """a real pole and a mild biquad behind it (the cascade of test_iir_segment_sequential_runs_...): the pole sets how fast the memory fades"""
    return _f32([((1.0 - p, 0.0, 0.0), (1.0, -p, 0.0)), ((0.2, 0.3, 0.2), (1.0, -0.4, 0.2))])


_BQ8 = [_bq(0.80, 0.6), _bq(0.70, 1.4), _bq(0.85, 0.3, (0.3, -0.1, 0.2)), _bq(0.60, 2.2), _bq(0.75, 1.0), _bq(0.65, 1.8, (0.4, 0.1, -0.2)), _bq(0.82, 2.6), _bq(0.5, 0.9)]
_O44 = [_o4(0.80, 0.6, 0.70, 1.4), _o4(0.85, 0.3, 0.60, 2.2), _o4(0.75, 1.0, 0.65, 1.8, (0.3, -0.1, 0.2, 0.1, 0.05)), _o4(0.82, 2.6, 0.5, 0.9)]
_NEAR = _bq(0.9997, 0.3, (3e-4, 0.0, 0.0))  # a pole pair 3e-4 inside the unit circle: no warm-up of 4 tiles forgets it
_NEAR4 = (np.array([3e-4, 1e-4, 2e-4, 0.0, 0.0]), np.convolve(_NEAR[1], _bq(0.7, 1.4)[1]))
FILTERS = {
    "bq2": _f32(_BQ8[:2]), "bq4": _f32(_BQ8[:4]), "bq5": _f32(_BQ8[:5]), "bq8": _f32(_BQ8),
    "o4x1": _f32([((0.1, 0.2, 0.3, 0.2, 0.1), (1.0, -0.9, 0.5, -0.1, 0.02))]), "o4x2": _f32(_O44[:2]), "o4x3": _f32(_O44[:3]), "o4x4": _f32(_O44),
    "near_bq2": _f32([_NEAR, _BQ8[1]]), "near_bq4": _f32([_NEAR] + _BQ8[1:4]), "near_o4x1": _f32([_NEAR4]), "near_o4x2": _f32([_NEAR4, _O44[1]]),
    "p0.7": _pole(0.7), "p0.985": _pole(0.985), "p0.993": _pole(0.993), "p0.9965": _pole(0.9965), "p0.998": _pole(0.998), "p0.999": _pole(0.999), "p0.99999": _pole(0.99999),
    "order1": (np.array([[0.3, 0.2]], np.float32), np.array([[1.0, -0.7]], np.float32)),
    "order3": (np.array([[0.1, 0.2, 0.2, 0.1]], np.float32), np.array([[1.0, -0.9, 0.5, -0.1]], np.float32)),
    "nb1_na3": (np.array([[0.4]], np.float32), np.array([[1.0, -1.1, 0.5]], np.float32)),          # all-pole
    "nb3_na1": (np.array([[0.3, -0.5, 0.2]], np.float32), np.array([[1.0]], np.float32)),          # feed-forward only
    "nb5_na3": (np.array([[0.1, 0.2, 0.3, 0.2, 0.1]], np.float32), np.array([[1.0, -1.1, 0.5]], np.float32)),
    "one_pole": (np.array([[0.1, 0.0]], np.float32), np.array([[1.0, -0.9]], np.float32)),
}
SLOW = {"near_bq2", "near_bq4", "near_o4x1", "near_o4x2", "p0.9965", "p0.998", "p0.999", "p0.99999"}  # bar: max(1e-5, 3 x the float32 cascade's own error)
NMAX = 40 * TILE  # no span of the table and no stream of the hand-off tests is longer


# ------------------------------------------------------------------ the create-time decisions, restated (iir_create_impl)
def _layout(b, a, no_split=False):
    """the handle's parts as iir_create_impl lays them out: [(ORD, padded NSEC, B[nsec][ord + 1], A[nsec][ord + 1])]; more than 8 state values: two parts"""
    b, a = np.atleast_2d(b).astype(np.float64), np.atleast_2d(a).astype(np.float64)
    ns, order = b.shape[0], max(b.shape[1], a.shape[1]) - 1
    ord_ = 2 if order <= 2 else 4
    if ns * ord_ > 8 and not no_split:
        k = 8 // ord_
        return _layout(b[:k], a[:k]) + _layout(b[k:], a[k:])
    mp = 4 if ns * ord_ <= 4 else 8 if ns * ord_ <= 8 else 16
    nsec = mp // ord_
    B, A = np.zeros((nsec, ord_ + 1)), np.zeros((nsec, ord_ + 1))
    B[ns:, 0] = 1.0  # identity padding sections
    B[:ns, :b.shape[1]], A[:ns, :a.shape[1]] = b, a
    A[:, 0] = 1.0    # a[0] is taken as 1
    return [(ord_, nsec, B, A)]


def _warm(part):
    """(warm_tiles, warm_chunks) of one part: the smallest w in {1, 2, 4} tiles with ||Phi_tile^w||_inf <= 1e-8 in float64, and for w = 1 the smallest of 32, 64, 128
    chunks of the warm-up tile that already do; (0, 0): the memory does not fade within 4 tiles (look-back), or the part has 16 state values (three-pass)"""
    ord_, nsec, B, A = part
    M = ord_ * nsec
    if M > 8:
        return 0, 0
    step = np.zeros((M, M))
    for j in range(M):  # one zero-input step of the direct-form-II cascade from the unit state e_j (host_step)
        st = np.zeros((nsec, ord_))
        st.ravel()[j] = 1.0
        x = 0.0
        for s in range(nsec):
            w = x - A[s, 1:] @ st[s]
            x = B[s, 0] * w + B[s, 1:] @ st[s]
            st[s] = np.concatenate(([w], st[s][:-1]))
        step[:, j] = st.ravel()
    nrm = lambda P: float(np.max(np.sum(np.abs(P), axis=1)))
    PL = np.linalg.matrix_power(step, CHUNK)
    Pw = np.linalg.matrix_power(PL, CHUNKS)
    for w in (1, 2, 4):
        if nrm(Pw) <= 1e-8:
            if w == 1:
                Pc = np.linalg.matrix_power(PL, 32)
                for wc in (32, 64, 128):
                    if nrm(Pc) <= 1e-8:
                        return 1, wc
                    Pc = Pc @ Pc
            return w, CHUNKS
        Pw = Pw @ Pw
    return 0, 0


def _parts(name, no_split=False):
    """[(ORD, padded NSEC, warm_tiles, warm_chunks)] of a table filter"""
    return [(p[0], p[1]) + _warm(p) for p in _layout(*FILTERS[name], no_split=no_split)]


def _want(kernel, part, n, slots):
    """the record of one part for a call of n samples: {kernel, ORD, NSEC, warm_tiles, warm_chunks, tiles_per_wg, grid, nt} (iir_run)"""
    ord_, nsec, wt, wc = part
    nb = -(-n // TILE)
    if kernel == SEQ:
        per = max(wt, -(-nb // slots))
        return (SEQ, ord_, nsec, wt, wc, per, -(-nb // per), 0)
    return (kernel, ord_, nsec, 0, 0, 1, nb, 0)


def _by_nature(part):
    return THREE if part[0] * part[1] > 8 else SEQ if part[2] > 0 else LOOKBACK


def _record(G, f):
    """the last call's record: one tuple per part of the handle"""
    fn = G.capi.lib().gr4hip_internal_iir_last_path  # (test hook, not in include/gr4hip.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    rec = (C.c_int * 8)()
    assert fn(f._h, -1, rec) == 0
    split = rec[0] == 1
    assert fn(f._h, 0, rec) == 0
    first = tuple(rec)
    if not split or first[0] == SEQ_F32:
        return (first,)
    assert fn(f._h, 1, rec) == 0
    return (first, tuple(rec))


def _signal(n, seed):
    return O.signal_f32(seed, n, tone_frel=0.03)


def _sections(name):
    b, a = FILTERS[name]
    return O.make_sections([(bb, aa) for bb, aa in zip(np.atleast_2d(b), np.atleast_2d(a))])


_ORACLE = {}


def _oracle(name, seed, n=NMAX):
    """(x, float64 truth, error of the reference's float32 cascade) of a table filter on the file's test signal, computed once"""
    key = (name, seed, n)
    if key not in _ORACLE:
        x = _signal(n, seed)
        truth = O.iir_cascade(_sections(name), x, O.DF_II, f64=True)
        truth.setflags(write=False)
        _ORACLE[key] = (x, truth, _rel(O.iir_cascade(_sections(name), x, O.DF_II, f64=False), truth))
    return _ORACLE[key]


def _bar(name, e32):
    return max(TOL, 3 * e32) if name in SLOW else TOL


class _Stream:
    """one handle fed the consecutive spans of `x`: each call places its input `xoff` and its output `yoff` floats past a 16-byte boundary of a fresh allocation,
    and records what the hook says it enqueued next to what the dispatcher's rules say it should have"""

    def __init__(self, G, f, x, parts, slots=None):
        self.G, self.f, self.x, self.parts = G, f, x, parts
        self.slots = slots or 4 * torch.cuda.get_device_properties(0).multi_processor_count  # four resident workgroups per compute unit
        self.pos, self.ys, self.seen = 0, [], []

    def __call__(self, n, kernel=None, xoff=0, yoff=0):
        """kernel None: each part by nature; LOOKBACK / THREE: every part by switch; SEQ_F32: the one launch of the whole cascade"""
        xin = torch.empty(n + 4, dtype=torch.float32, device="cuda")[xoff:xoff + n]
        xin.copy_(torch.from_numpy(np.ascontiguousarray(self.x[self.pos:self.pos + n])))
        out = torch.empty(n + 4, dtype=torch.float32, device="cuda")[yoff:yoff + n]
        assert (xin.data_ptr() % 16 == 0) == (xoff == 0) and (out.data_ptr() % 16 == 0) == (yoff == 0)
        self.f.process_bulk(xin, out)
        self.ys.append(out.cpu().numpy())
        if kernel == SEQ_F32:
            b, a = self.f.b, self.f.a
            want = ((SEQ_F32, max(b.shape[1], a.shape[1]) - 1, b.shape[0], 0, 0, 1, 1, 0),)
        else:
            want = tuple(_want(kernel or _by_nature(p), p, n, self.slots) for p in self.parts)
        self.seen.append((self.pos, n, xoff, yoff, _record(self.G, self.f), want))
        self.pos += n
        return self.ys[-1]

    def y(self):
        return np.concatenate(self.ys)

    def wrong(self):
        return [s for s in self.seen if s[4] != s[5]]


# ------------------------------------------------------------------ a. routing table: one case per reachable (kernel, instantiation)
# (id, filter, switch, algo, kernel expected, [(ORD, padded NSEC, warm_tiles, warm_chunks) per part]); kernel None: by nature, which the parts' warm_tiles decide
# (warm_tiles 0 and <= 8 state values: look-back).  The template instantiations of iir_process_parallel: <2,2> <2,4> <2,8> <4,1> <4,2> <4,4>.
_S32, _NO = (1, 32), (0, 0)
_ROUTES = [
    # segment-sequential runs by nature: iir_seq_kernel<2,2> <2,4> <4,1> <4,2>
    ("seq_2_2", "bq2", None, None, SEQ, [(2, 2) + _S32]),
    ("seq_2_4", "bq4", None, None, SEQ, [(2, 4) + _S32]),
    ("seq_4_1", "o4x1", None, None, SEQ, [(4, 1) + _S32]),
    ("seq_4_2", "o4x2", None, None, SEQ, [(4, 2) + _S32]),
    # look-back by nature (a pole pair 3e-4 inside the circle): iir_onepass_kernel<2,2> <2,4> <4,1> <4,2>
    ("lookback_nature_2_2", "near_bq2", None, "IIR_PARALLEL", LOOKBACK, [(2, 2) + _NO]),
    ("lookback_nature_2_4", "near_bq4", None, "IIR_PARALLEL", LOOKBACK, [(2, 4) + _NO]),
    ("lookback_nature_4_1", "near_o4x1", None, "IIR_PARALLEL", LOOKBACK, [(4, 1) + _NO]),
    ("lookback_nature_4_2", "near_o4x2", None, "IIR_PARALLEL", LOOKBACK, [(4, 2) + _NO]),
    # look-back by switch
    ("lookback_switch_2_2", "bq2", "GR4HIP_IIR_LOOKBACK", None, LOOKBACK, [(2, 2) + _S32]),
    ("lookback_switch_2_4", "bq4", "GR4HIP_IIR_LOOKBACK", None, LOOKBACK, [(2, 4) + _S32]),
    ("lookback_switch_4_1", "o4x1", "GR4HIP_IIR_LOOKBACK", None, LOOKBACK, [(4, 1) + _S32]),
    ("lookback_switch_4_2", "o4x2", "GR4HIP_IIR_LOOKBACK", None, LOOKBACK, [(4, 2) + _S32]),
    # three-pass by switch: iir_pass_z / iir_pass_y <2,2> <2,4> <4,1> <4,2>, iir_pass_b<4> <8>
    ("three_2_2", "bq2", "GR4HIP_IIR_THREE_PASS", None, THREE, [(2, 2) + _S32]),
    ("three_2_4", "bq4", "GR4HIP_IIR_THREE_PASS", None, THREE, [(2, 4) + _S32]),
    ("three_4_1", "o4x1", "GR4HIP_IIR_THREE_PASS", None, THREE, [(4, 1) + _S32]),
    ("three_4_2", "o4x2", "GR4HIP_IIR_THREE_PASS", None, THREE, [(4, 2) + _S32]),
    # three-pass by GR4HIP_IIR_NO_SPLIT, the only kernels of 16 state values: iir_pass_z / iir_pass_y <2,8> <4,4>, iir_pass_b<16>
    ("nosplit_2_8_five", "bq5", "GR4HIP_IIR_NO_SPLIT", None, THREE, [(2, 8) + _NO]),
    ("nosplit_2_8_eight", "bq8", "GR4HIP_IIR_NO_SPLIT", None, THREE, [(2, 8) + _NO]),
    ("nosplit_4_4_three", "o4x3", "GR4HIP_IIR_NO_SPLIT", None, THREE, [(4, 4) + _NO]),
    ("nosplit_4_4_four", "o4x4", "GR4HIP_IIR_NO_SPLIT", None, THREE, [(4, 4) + _NO]),
    # split handles: two cascades one behind the other, each on its own kernel
    ("split_5_biquads", "bq5", None, None, SEQ, [(2, 4) + _S32, (2, 2) + _S32]),
    ("split_8_biquads", "bq8", None, None, SEQ, [(2, 4) + _S32, (2, 4) + _S32]),
    ("split_3_order4", "o4x3", None, None, SEQ, [(4, 2) + _S32, (4, 1) + _S32]),
    ("split_4_order4", "o4x4", None, None, SEQ, [(4, 2) + _S32, (4, 2) + _S32]),
    # the sequential float32 form, whole and split
    ("seq_f32_bq4", "bq4", None, "IIR_SEQUENTIAL_F32", SEQ_F32, [(2, 4) + _S32]),
    ("seq_f32_o4x3", "o4x3", None, "IIR_SEQUENTIAL_F32", SEQ_F32, [(4, 2) + _S32, (4, 1) + _S32]),
    # section shapes: order 1 and 2 on the biquad kernels, order 3 padded to 4, and rows of different lengths
    ("shape_order1", "order1", None, None, SEQ, [(2, 2) + _S32]),
    ("shape_order3", "order3", None, None, SEQ, [(4, 1) + _S32]),
    ("shape_nb1_na3", "nb1_na3", None, None, SEQ, [(2, 2) + _S32]),
    ("shape_nb3_na1", "nb3_na1", None, None, SEQ, [(2, 2) + _S32]),
    ("shape_nb5_na3", "nb5_na3", None, None, SEQ, [(4, 1) + _S32]),
    ("shape_order3_three_pass", "order3", "GR4HIP_IIR_THREE_PASS", None, THREE, [(4, 1) + _S32]),
    ("shape_nb5_na3_lookback", "nb5_na3", "GR4HIP_IIR_LOOKBACK", None, LOOKBACK, [(4, 1) + _S32]),
    # every (warm_tiles, warm_chunks) the host can choose
    ("warm_1_32", "p0.7", None, None, SEQ, [(2, 2, 1, 32)]),
    ("warm_1_64", "p0.985", None, None, SEQ, [(2, 2, 1, 64)]),
    ("warm_1_128", "p0.993", None, None, SEQ, [(2, 2, 1, 128)]),
    ("warm_1_256", "p0.9965", None, "IIR_PARALLEL", SEQ, [(2, 2, 1, 256)]),
    ("warm_2_256", "p0.998", None, "IIR_PARALLEL", SEQ, [(2, 2, 2, 256)]),
    ("warm_4_256", "p0.999", None, "IIR_PARALLEL", SEQ, [(2, 2, 4, 256)]),
    ("warm_0_lookback", "p0.99999", None, "IIR_PARALLEL", LOOKBACK, [(2, 2) + _NO]),
]
# (n, xoff, yoff): later calls start from carried state; a misaligned input, a misaligned output, a call shorter than a tile, an exact multiple of a tile, and
# a span of several runs (40 tiles in all)
_CALLS = [(2 * TILE + 3616, 0, 0), (5_000, 1, 0), (3 * TILE, 0, 1), (24 * TILE + 4097, 3, 2), (9 * TILE + 3671, 0, 0)]
assert sum(c[0] for c in _CALLS) == NMAX


def check_table():
    """no GPU: the filters are what the table says they are -- the warm-up of every part by the restated create-time criterion, every instantiation and every
    warm-up choice reached, and the reference's float32 cascade within 3e-6 of float64 on the test signal for every filter that is held to 1e-5"""
    for cid, name, switch, algo, kernel, parts in _ROUTES:
        got = _parts(name, no_split=switch == "GR4HIP_IIR_NO_SPLIT")
        assert got == [tuple(p) for p in parts], (cid, got, parts)
        if kernel in (SEQ, LOOKBACK) and switch is None:
            assert all(_by_nature(p) == kernel for p in got), cid
    reached = {(k, p[0], p[1]) for _, _, _, _, k, parts in _ROUTES for p in parts}
    for k in (SEQ, LOOKBACK, THREE):
        assert {(k, 2, 2), (k, 2, 4), (k, 4, 1), (k, 4, 2)} <= reached, k
    assert {(THREE, 2, 8), (THREE, 4, 4)} <= reached and any(k == SEQ_F32 for k, _, _ in reached)
    warm = {(p[2], p[3]) for _, _, sw, _, k, parts in _ROUTES for p in parts if k in (SEQ, LOOKBACK) and sw is None}
    assert warm == {(1, 32), (1, 64), (1, 128), (1, 256), (2, 256), (4, 256), (0, 0)}
    for name in sorted({r[1] for r in _ROUTES} | set(_EDGE_FILTERS) | {"one_pole"}):
        e32 = _oracle(name, 11)[2]
        assert name in SLOW or e32 <= REF32_OK, (name, e32)


def test_table_filters_are_what_the_table_says():
    check_table()


@pytest.mark.parametrize("cid,name,switch,algo,kernel,parts", _ROUTES, ids=[r[0] for r in _ROUTES])
def test_iir_routing_table(G, devsw, cid, name, switch, algo, kernel, parts):
    x, truth, e32 = _oracle(name, 11)
    if switch:
        devsw(switch)  # (GR4HIP_IIR_NO_SPLIT is read at create)
    f = G.iir_filter(*FILTERS[name])
    if algo:
        f.set_algo(getattr(G.capi, algo))
    s = _Stream(G, f, x, parts)
    forced = {"GR4HIP_IIR_LOOKBACK": LOOKBACK, "GR4HIP_IIR_THREE_PASS": THREE}.get(switch, SEQ_F32 if kernel == SEQ_F32 else None)
    for n, xoff, yoff in _CALLS:
        s(n, forced, xoff, yoff)
    f.status()
    e = _rel(s.y(), truth)
    print(cid, "error", e, "float32 cascade", e32, "bar", _bar(name, e32))
    assert all(r[0] == kernel for call in s.seen for r in call[4]), (cid, s.seen)
    assert not s.wrong() and e <= _bar(name, e32), (cid, e, e32, s.wrong())


@pytest.mark.parametrize("name", ["bq5", "bq8", "o4x3", "o4x4"])
def test_unsplit_and_split_handles_agree(G, devsw, name):
    """the same cascade as one scan of 16 state values (GR4HIP_IIR_NO_SPLIT) and as two cascades one behind the other"""
    x, truth, e32 = _oracle(name, 11)
    out = {}
    for mode in ("split", "whole"):
        if mode == "whole":
            devsw("GR4HIP_IIR_NO_SPLIT")
        s = _Stream(G, G.iir_filter(*FILTERS[name]), x, _parts(name, no_split=mode == "whole"))
        for n in (3 * TILE + 5, 12 * TILE, 7 * TILE - 1):
            s(n)
        assert not s.wrong() and len(s.seen[0][4]) == (2 if mode == "split" else 1), s.seen
        out[mode] = s.y().astype(np.float64)
        assert _rel(out[mode], truth[:s.pos]) <= _bar(name, e32), mode
    assert np.abs(out["split"] - out["whole"]).max() <= PAIR * np.sqrt(np.mean(truth ** 2))


# ------------------------------------------------------------------ b. tile edges of the segment-sequential kernel: run boundaries at a few dozen tiles
# GR4HIP_IIR_SEQ_SLOTS = 3: tiles_per_wg = max(warm_tiles, ceil(tiles / 3)).  The poles are slow for their warm-up: a run that starts from a wrong state stays
# wrong for thousands of samples.
_EDGE_FILTERS = {"p0.9965": (1, 256), "p0.985": (1, 64), "p0.998": (2, 256), "p0.999": (4, 256)}
_FIRST = 12_345


def _edge_spans(w):
    return [5, TILE - 1, TILE, TILE + 1, w * TILE, w * TILE + 1, (w + 1) * TILE - 1, (w + 1) * TILE, (2 * w + 1) * TILE + 77, 19 * TILE + 4096 + 13]


@pytest.mark.parametrize("name", list(_EDGE_FILTERS))
def test_iir_segment_sequential_tile_edges(G, devsw, name):
    w, wc = _EDGE_FILTERS[name]
    parts = _parts(name)
    assert parts == [(2, 2, w, wc)]
    x, truth, e32 = _oracle(name, 11)
    bar, rms = _bar(name, e32), np.sqrt(np.mean(truth ** 2))
    devsw("GR4HIP_IIR_SEQ_SLOTS", 3)
    records, worst = [], 0.0
    for n in _edge_spans(w):
        for behind in (0, _FIRST):  # as a first call, and from the state a first call of 12 345 samples left
            ys = {}
            for kernel in (SEQ, LOOKBACK):
                devsw("GR4HIP_IIR_LOOKBACK", int(kernel == LOOKBACK))
                f = G.iir_filter(*FILTERS[name])
                f.set_algo(G.capi.IIR_PARALLEL)
                s = _Stream(G, f, x, parts, slots=3)
                if behind:
                    s(behind, kernel if kernel == LOOKBACK else None)
                ys[kernel] = s(n, kernel if kernel == LOOKBACK else None, xoff=(n % 3), yoff=(n % 2)).astype(np.float64)
                f.status()
                assert not s.wrong(), (n, behind, s.seen)
                e = _rel(s.y(), truth[:s.pos])
                worst = max(worst, e)
                assert e <= bar, (n, behind, kernel, e, bar)
                if kernel == SEQ:
                    records.append((n, s.seen[-1][4][0]))
            assert np.abs(ys[SEQ] - ys[LOOKBACK]).max() <= PAIR * rms, (n, behind)
    print(name, "worst error", worst, "bar", bar)
    tiles = lambda n: -(-n // TILE)
    assert any(r[6] >= 2 and r[5] > r[3] for _, r in records)                       # several workgroups, runs longer than their warm-up
    assert any(tiles(n) % r[5] != 0 and r[6] >= 2 for n, r in records)              # a last run shorter than the others
    assert any(tiles(n) == r[3] + 1 and r[6] == 2 and r[5] == r[3] for n, r in records)  # the second run's warm-up starts at tile 0: it takes the carried state


# ------------------------------------------------------------------ c. block edges of the other two kernels
@pytest.mark.parametrize("name", ["near_bq4", "o4x1"])
def test_iir_lookback_window_edges(G, devsw, name):
    """the look-back kernel, by switch: a block looks back over windows of 64 predecessors -- spans of 1, 2, 3, 64, 65, 66 and 129 blocks plus 5 samples, each twice
    on one handle (from zero state and from carried state)"""
    devsw("GR4HIP_IIR_LOOKBACK")
    parts = _parts(name)
    for blocks in (1, 2, 3, 64, 65, 66, 129):
        n = blocks * TILE + 5
        x, truth, e32 = _oracle(name, 12, 2 * (129 * TILE + 5))
        f = G.iir_filter(*FILTERS[name])
        f.set_algo(G.capi.IIR_PARALLEL)
        s = _Stream(G, f, x, parts)
        s(n, LOOKBACK)
        s(n, LOOKBACK, xoff=1, yoff=3)
        f.status()
        e = _rel(s.y(), truth[:s.pos])
        assert not s.wrong() and s.seen[0][4][0][6] == blocks + 1 and e <= _bar(name, e32), (blocks, e, e32, s.seen)


@pytest.mark.parametrize("name", ["near_bq4", "o4x1"])
def test_iir_three_pass_lane_chains(G, devsw, name):
    """the three-pass kernels, by switch: iir_pass_b walks the blocks in chains of four per lane -- spans of 1, 3, 4, 5 and 9 blocks, each twice on one handle"""
    devsw("GR4HIP_IIR_THREE_PASS")
    parts = _parts(name)
    x, truth, e32 = _oracle(name, 12, 2 * (129 * TILE + 5))
    for blocks in (1, 3, 4, 5, 9):
        f = G.iir_filter(*FILTERS[name])
        f.set_algo(G.capi.IIR_PARALLEL)
        s = _Stream(G, f, x, parts)
        s(blocks * TILE, THREE)
        s(blocks * TILE, THREE, xoff=2, yoff=1)
        e = _rel(s.y(), truth[:s.pos])
        assert not s.wrong() and s.seen[0][4][0][6] == blocks and e <= _bar(name, e32), (blocks, e, e32, s.seen)


def test_iir_three_pass_crosses_a_block_scan_group(G, devsw):
    """2049 blocks plus 5 samples: the smallest span for which iir_pass_b's loop over groups of 2048 blocks runs twice and hands its T across; a second call takes
    the state from there.  One pole, so that the oracle stays cheap"""
    devsw("GR4HIP_IIR_THREE_PASS")
    n1, n2 = 2049 * TILE + 5, 3 * TILE + 7
    x, truth, e32 = _oracle("one_pole", 13, n1 + n2)
    s = _Stream(G, G.iir_filter(*FILTERS["one_pole"]), x, _parts("one_pole"))
    s(n1, THREE)
    s(n2, THREE)
    e = _rel(s.y(), truth)
    assert not s.wrong() and s.seen[0][4][0][6] == 2050 and e <= TOL, (e, s.seen)


# ------------------------------------------------------------------ d. hand-offs: one handle, one stream
def _restarted(name, x, cuts):
    """the oracle started from zero state at every cut"""
    return np.concatenate([O.iir_cascade(_sections(name), x[lo:hi], O.DF_II, f64=True) for lo, hi in zip(cuts[:-1], cuts[1:])])


def test_handoff_between_the_three_parallel_kernels(G, devsw):
    """the three parallel kernels share one direct-form-II state pair: no switch, look-back, three-pass, no switch on one stream is the oracle's one stream"""
    name = "p0.999"
    x, truth, e32 = _oracle(name, 11)
    f = G.iir_filter(*FILTERS[name])
    f.set_algo(G.capi.IIR_PARALLEL)
    s = _Stream(G, f, x, _parts(name))
    s(5 * TILE + 1234)
    devsw("GR4HIP_IIR_LOOKBACK", 1)
    s(3 * TILE + 77, LOOKBACK, xoff=1)
    devsw("GR4HIP_IIR_LOOKBACK", 0)
    devsw("GR4HIP_IIR_THREE_PASS", 1)
    s(4_000, THREE)
    s(6 * TILE, THREE, yoff=1)
    devsw("GR4HIP_IIR_THREE_PASS", 0)
    s(9 * TILE + 5)
    f.status()
    e = _rel(s.y(), truth[:s.pos])
    assert not s.wrong() and e <= _bar(name, e32), (e, e32, s.seen)


def test_handoff_set_algo_restarts_from_zero_state(G):
    """PARALLEL -> SEQUENTIAL_F32 -> AUTO in mid-stream: the two evaluations keep different state, every change restarts the filter"""
    name = "bq4"
    x, _, e32 = _oracle(name, 11)
    cuts = [0, 3 * TILE + 100, 5 * TILE + 300, 9 * TILE + 1]
    f = G.iir_filter(*FILTERS[name])
    s = _Stream(G, f, x, _parts(name))
    f.set_algo(G.capi.IIR_PARALLEL)
    s(cuts[1] - cuts[0])
    f.set_algo(G.capi.IIR_SEQUENTIAL_F32)
    s(cuts[2] - cuts[1], SEQ_F32)
    f.set_algo(G.capi.IIR_AUTO)
    assert f.algo_in_use[0] == G.capi.IIR_PARALLEL
    s(cuts[3] - cuts[2])
    e = _rel(s.y(), _restarted(name, x, cuts))
    assert not s.wrong() and e <= _bar(name, e32), (e, s.seen)


@pytest.mark.parametrize("name,switch,algo,kernel", [("p0.999", None, "IIR_PARALLEL", None), ("p0.999", "GR4HIP_IIR_LOOKBACK", "IIR_PARALLEL", LOOKBACK),
                                                    ("p0.999", "GR4HIP_IIR_THREE_PASS", "IIR_PARALLEL", THREE), ("bq8", None, None, None),
                                                    ("bq8", None, "IIR_SEQUENTIAL_F32", SEQ_F32), ("bq4", None, "IIR_SEQUENTIAL_F32", SEQ_F32)],
                         ids=["runs", "lookback", "three_pass", "split", "split_seq_f32", "seq_f32"])
def test_handoff_reset_in_mid_stream(G, devsw, name, switch, algo, kernel):
    """reset() between two calls: the next call is the oracle from zero state -- for a split handle in both parts, for the sequential form in its own histories"""
    x, _, e32 = _oracle(name, 11)
    cuts = [0, 2 * TILE + 4000, 7 * TILE + 4001]
    if switch:
        devsw(switch)
    f = G.iir_filter(*FILTERS[name])
    if algo:
        f.set_algo(getattr(G.capi, algo))
    s = _Stream(G, f, x, _parts(name))
    s(cuts[1], kernel)
    f.reset()
    s(cuts[2] - cuts[1], kernel, xoff=1)
    e = _rel(s.y(), _restarted(name, x, cuts))
    assert not s.wrong() and e <= _bar(name, e32), (e, s.seen)


@pytest.mark.parametrize("name", ["p0.999", "bq8"])
def test_handoff_reset_behind_an_unsynchronised_call(G, name):
    """reset() is a host-side note: the state is zeroed on the stream of the NEXT call, behind the launches still in flight -- the earlier call's output is intact"""
    x, _, e32 = _oracle(name, 11)
    n1, n2 = 30 * TILE + 11, 4 * TILE + 5
    f = G.iir_filter(*FILTERS[name])
    x1, x2 = torch.from_numpy(x[:n1]).cuda(), torch.from_numpy(x[n1:n1 + n2]).cuda()
    torch.cuda.synchronize()
    y1 = f.process_bulk(x1)  # (nothing waits for it)
    f.reset()
    y2 = f.process_bulk(x2)
    parts = _parts(name)
    assert _record(G, f) == tuple(_want(SEQ, p, n2, 4 * torch.cuda.get_device_properties(0).multi_processor_count) for p in parts)
    y = np.concatenate([y1.cpu().numpy(), y2.cpu().numpy()])
    e = _rel(y, _restarted(name, x, [0, n1, n1 + n2]))
    assert e <= _bar(name, e32), e


# ------------------------------------------------------------------ overlapping input and output
def test_iir_refuses_overlapping_input_and_output(G):
    """the kernels read through __restrict__ pointers, and a run of the segment-sequential kernel warms up on input tiles that the run before it overwrites when the
    output is the input: gr4hip_iir_process and gr4hip_iir64_process refuse overlapping ranges before anything is enqueued (include/gr4hip.h)"""
    for dt in (torch.float32, torch.float64):
        f = G.iir_filter(*FILTERS["bq2"], dtype=dt)
        buf = torch.zeros(3 * TILE, dtype=dt, device="cuda")
        for xin, out in ((buf[:TILE], buf[:TILE]), (buf[:TILE], buf[TILE - 1:2 * TILE - 1]), (buf[5:TILE + 5], buf[:TILE])):
            with pytest.raises(G.capi.Gr4HipError) as e:
                f.process_bulk(xin, out)
            assert e.value.status == G.capi.INVALID_ARGUMENT
        if dt == torch.float32:
            assert _record(G, f)[0][0] == 0  # (the handle has enqueued nothing)
