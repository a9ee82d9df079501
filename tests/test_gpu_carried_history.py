"""The carry launch every streaming filter shares (csrc/history.hpp, CarriedHistory::advance; csrc/history.hip): new[h] = (old ++ x)[n_in + h], h < len, as a copy of
4-byte or 8-byte elements.  Driven through the library's test hook gr4hip_internal_carry_history (exported, not in include/gr4hip.h) on buffers of seeded random BIT
PATTERNS -- NaN payloads, -0 and subnormals included -- and compared byte for byte with concatenate(old, x)[-len:].  The three buffers are views into larger
allocations of a sentinel: nothing around `new` may change, and `old` and `x` stay as they were."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENT = 0x4B1D5EED
PAD = 64  # uint32 words of sentinel on either side of every buffer (a multiple of 2: the 8-byte views stay aligned)


@pytest.fixture(scope="module")
def carry():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gnuradio4_amd as G
    fn = G.capi.lib().gr4hip_internal_carry_history
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return G, fn


def _framed(words):
    """a device allocation of sentinels with `words` (uint32, as int32 bits) in its middle -> (allocation, the expected host image of it)"""
    host = np.full(words.size + 2 * PAD, SENT, np.uint32)
    host[PAD:PAD + words.size] = words
    return torch.from_numpy(host.view(np.int32)).cuda(), host


@pytest.mark.parametrize("elem_bytes", [4, 8])
@pytest.mark.parametrize("length", [1, 255, 256, 257])
def test_carry_is_the_tail_of_old_and_input_bit_for_bit(carry, elem_bytes, length):
    G, fn = carry
    w = elem_bytes // 4  # uint32 words per element
    rng = np.random.default_rng(1000 * elem_bytes + length)
    for n_in in sorted({0, 1, length - 1, length, length + 1, 2 * length + 3}):
        old = rng.integers(0, 2 ** 32, length * w, dtype=np.uint32)
        x = rng.integers(0, 2 ** 32, max(n_in, 1) * w, dtype=np.uint32)  # (n_in = 0: one element nobody may read, so that the pointer is not null)
        d_old, h_old = _framed(old)
        d_x, h_x = _framed(x)
        d_new, h_new = _framed(np.full(length * w, SENT, np.uint32))
        off = 4 * PAD
        G.capi.check(fn(elem_bytes, d_x.data_ptr() + off, n_in, d_old.data_ptr() + off, d_new.data_ptr() + off, length, None), "carry_history")
        want = np.concatenate([old, x[:n_in * w]])[-length * w:]
        got = d_new.cpu().numpy().view(np.uint32)
        assert got[PAD:PAD + length * w].tobytes() == want.tobytes(), (elem_bytes, length, n_in)
        assert np.all(got[:PAD] == SENT) and np.all(got[PAD + length * w:] == SENT), (elem_bytes, length, n_in)
        assert d_old.cpu().numpy().view(np.uint32).tobytes() == h_old.tobytes() and d_x.cpu().numpy().view(np.uint32).tobytes() == h_x.tobytes()


def test_carry_hook_refuses_what_the_kernel_cannot_take(carry):
    G, fn = carry
    a, b, x = (torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(3))
    pa, pb, px = a.data_ptr(), b.data_ptr(), x.data_ptr()
    assert fn(8, px, 4, pa, pb, 4, None) == 0
    bad = G.capi.INVALID_ARGUMENT
    for width in (0, 1, 2, 3, 5, 16):
        assert fn(width, px, 4, pa, pb, 4, None) == bad and b"4 or 8" in G.capi.lib().gr4hip_last_error()
    assert fn(4, None, 4, pa, pb, 4, None) == bad and fn(4, px, 4, None, pb, 4, None) == bad and fn(4, px, 4, pa, None, 4, None) == bad
    assert fn(4, px + 2, 4, pa, pb, 4, None) == bad and fn(8, px, 4, pa + 4, pb, 4, None) == bad and fn(8, px, 4, pa, pb + 4, 4, None) == bad
    assert fn(4, px, 4, pa + 4, pb, 4, None) == 0  # (4-byte elements need 4-byte alignment only)
    assert fn(4, px, 4, pa, pa, 4, None) == bad and b"one buffer" in G.capi.lib().gr4hip_last_error()
    assert fn(4, px, 4, pa, pb, 0, None) == bad
    torch.cuda.synchronize()
