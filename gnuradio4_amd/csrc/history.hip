// history.hip -- the carry launch of CarriedHistory (history.hpp): the one kernel that moves a streaming filter's history past a call
#include "history.hpp"

namespace gr4 {

// new_hist[h] = (old_hist ++ x)[n + h]: element s = n - len + h of the call, or -- below 0, a call shorter than the history -- element len + s of the old
// history (s >= -len, so that index is never negative).  W is the element as the lane moves it: one 4-byte or one 8-byte load and store, whatever it means
// (a float, one float of an interleaved complex, a float2, a double).  Old and new are two buffers: nothing is read that this launch writes.
template <typename W>
__global__ __launch_bounds__(256) void carry_history_kernel(const W* __restrict__ x, long n, const W* __restrict__ old_hist, W* __restrict__ new_hist, long len) {
    const long h = (long)blockIdx.x * 256 + threadIdx.x;
    if (h >= len) return;
    const long s = n - len + h;
    new_hist[h]  = s >= 0 ? x[s] : old_hist[len + s];
}

int carry_history_launch(int elem_bytes, const void* x, size_t n_in, const void* old_hist, void* new_hist, size_t len, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(len, (size_t)256));
    if (elem_bytes == 4)
        hipLaunchKernelGGL(carry_history_kernel<unsigned>, grid, dim3(256), 0, st, static_cast<const unsigned*>(x), (long)n_in, static_cast<const unsigned*>(old_hist), static_cast<unsigned*>(new_hist), (long)len);
    else
        hipLaunchKernelGGL(carry_history_kernel<unsigned long long>, grid, dim3(256), 0, st, static_cast<const unsigned long long*>(x), (long)n_in, static_cast<const unsigned long long*>(old_hist), static_cast<unsigned long long*>(new_hist), (long)len);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

} // namespace gr4

using namespace gr4;

// test hook (exported, not declared in include/gr4hip.h): the carry launch on caller-owned buffers
extern "C" int gr4hip_internal_carry_history(int elem_bytes, const void* d_x, size_t n_in, const void* d_old, void* d_new, size_t len, gr4hip_stream_t stream) {
    GR4_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "carry_history: elements of %d bytes (4 or 8)", elem_bytes);
    GR4_REQUIRE(d_x && d_old && d_new, "carry_history: null device pointer");
    GR4_REQUIRE(((uintptr_t)d_x | (uintptr_t)d_old | (uintptr_t)d_new) % (uintptr_t)elem_bytes == 0, "carry_history: buffers must be aligned to %d bytes", elem_bytes);
    GR4_REQUIRE(d_new != d_old, "carry_history: old and new history are one buffer");
    GR4_REQUIRE(len >= 1 && len <= (size_t(1) << 38) && n_in <= (size_t(1) << 40), "carry_history: len=%zu n_in=%zu", len, n_in);
    return carry_history_launch(elem_bytes, d_x, n_in, d_old, d_new, len, as_stream(stream));
}
