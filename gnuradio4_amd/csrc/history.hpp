// history.hpp -- the tail of its input that a streaming filter carries from one process call to the next: one implementation of the stream rule (common.hpp)
// for it.  Two device buffers: a call reads current() in front of its span and the half after it is written into next() -- by advance()'s carry launch, or by
// the filter's own kernel followed by flip() -- so nothing is read that the same launch writes.
#pragma once
#include "common.hpp"

namespace gr4 {

// new_hist[h] = (old_hist ++ x)[n_in + h], h < len, in elements of elem_bytes (4 or 8) bytes; old_hist and new_hist are two buffers of len elements (history.hip)
int carry_history_launch(int elem_bytes, const void* x, size_t n_in, const void* old_hist, void* new_hist, size_t len, hipStream_t st);

struct CarriedHistory {
    DeviceBuffer d_half[2];
    int          cur   = 0;
    size_t       bytes = 0;    // in use of each half (the buffers only grow)
    bool         zero  = true; // current() is to be zeroed: noted by create / reset / a resize, applied by on() on the stream of the next call
    // host and hipMalloc only.  What the history held is lost: a launch still in flight may be writing either half, so the zeroing waits for the next call's stream
    int resize(size_t nbytes) {
        for (auto& h : d_half)
            if (const int rc = h.ensure(nbytes)) return rc;
        bytes = nbytes;
        zero  = true;
        return GR4HIP_OK;
    }
    void reset() { zero = true; }
    void keep() { zero = false; } // a caller has just written current() on its stream: what was pending is superseded
    // the history as the call about to be enqueued on `st` must see it: behind the handle's earlier launches on that stream, in front of the next
    int on(hipStream_t st) {
        if (zero && bytes) GR4_HIP_TRY(hipMemsetAsync(d_half[cur].ptr, 0, bytes, st));
        zero = false;
        return GR4HIP_OK;
    }
    void* current() const { return d_half[cur].ptr; } // (not const void*: a pending rescale and the chain's hand-over write it on the call's stream)
    void* next() const { return d_half[cur ^ 1].ptr; }
    void  flip() { cur ^= 1; } // (for launches that wrote next() themselves)
    // the handle moves past a span of n_in elements at x: the next history is the last len elements of (current ++ x)
    int advance(const void* x, size_t n_in, size_t len, int elem_bytes, hipStream_t st) {
        if (!len) return GR4HIP_OK;
        if (const int rc = carry_history_launch(elem_bytes, x, n_in, current(), next(), len, st)) return rc;
        flip();
        return GR4HIP_OK;
    }
};

} // namespace gr4
