// leaf_integrator.hpp -- the leaf-and-fold integration scheme of the spectrum integrator (SPECTRUM_INTEGRATOR.md), the cross-spectrum correlator
// (CROSS_SPECTRUM.md) and the integrating beamformer (BEAMFORMER.md): the geometry of one call, the emit step and the carried state, once.
//
//   leaf_l[e] = the float32 sum, frames ascending from +0, of row element e over integration q's leaf l = q A + [LEAF l, min(LEAF (l + 1), A))
//   acc[e]    = ((0 + (double)leaf_0[e]) + ...)           float64, leaves ascending;  y_q[e] = (float)acc[e]  or  (float)(acc[e] / (double)A)
//
// A call of n frames that starts `pos` frames into an integration touches the leaves K = k0 .. k0 + nl - 1, counted from that integration's first leaf.  One
// launch of the block's own (its leaf kernel, a transform's sink) writes the float32 sum of call-leaf k = K - k0 to leaves[k][M], the call's first continuing
// the carried running leaf; the emit kernel, a second small launch on the same stream, folds them into the float64 accumulator, writes the finished rows and
// stores the carry of the next call into the other of two carry buffers.
#pragma once
#include "common.hpp"

#include <algorithm>

namespace gr4 {

template <int LEAF>
struct LeafGeom {
    long pos; // frames of the integration in progress that earlier calls took (< A)
    long n;   // frames of this call
    long A;   // frames per integration
    long lpi; // leaves per integration: ceil(A / LEAF)
    long k0;  // pos / LEAF: the call's first leaf
    long nl;  // leaves the call touches
    long nq;  // integrations the call touches: ceil((pos + n) / A)
};

template <int LEAF>
__host__ __device__ __forceinline__ LeafGeom<LEAF> leaf_geom(long pos, long n, long A) {
    LeafGeom<LEAF> g{pos, n, A, (A + LEAF - 1) / LEAF, pos / LEAF, 0, (pos + n + A - 1) / A};
    const long     last = pos + n - 1; // n >= 1
    g.nl                = (last / A) * g.lpi + (last % A) / LEAF - g.k0 + 1;
    return g;
}

// call-leaf k: its first frame in the call, the frames of it the call holds, and whether the call holds its end
template <int LEAF>
__host__ __device__ __forceinline__ void leaf_range(const LeafGeom<LEAF>& g, long k, long* first, int* count, bool* complete) {
    const long K = g.k0 + k, q = K / g.lpi, l = K - q * g.lpi;
    const long s = q * g.A + l * LEAF;
    const long e = s + LEAF < (q + 1) * g.A ? s + LEAF : (q + 1) * g.A;
    const long a = s > g.pos ? s : g.pos, b = e < g.pos + g.n ? e : g.pos + g.n;
    *first    = a - g.pos;
    *count    = (int)(b - a);
    *complete = e <= g.pos + g.n;
}

// ---- emit.  Element i of [nq][M]: element e of the row of the j-th integration the call touches.  Its leaves in ascending order into a float64 sum that starts
// from the carried one (j = 0) or from 0; a complete integration is written to out[j], the last one leaves the carry of the next call: its sum, and the call's
// last leaf where the call does not hold that leaf's end.  HERMITIAN: the row is a packed lower triangle of interleaved complex values, baseline p = e / (2 N),
// and the imaginary part of the diagonal p = i (i + 3) / 2, where 8 p + 9 = (2 i + 3)^2, is +0 by definition.
template <int LEAF, bool HERMITIAN>
__host__ __device__ __forceinline__ void leaf_emit_element(long i, const float* __restrict__ leaves, const LeafGeom<LEAF>& g, const double* __restrict__ acc_in,
                                                           double* __restrict__ acc_out, float* __restrict__ leaf_out, float* __restrict__ out, long M, int N, int mean) {
    const long j = i / M;
    const long e = i - j * M;
    const long end = g.pos + g.n, k_last = g.nl - 1;
    long       first;
    int        count;
    bool       last_complete;
    leaf_range(g, k_last, &first, &count, &last_complete);
    const long ka = j * g.lpi > g.k0 ? j * g.lpi - g.k0 : 0, kb = (j + 1) * g.lpi - g.k0 < g.nl ? (j + 1) * g.lpi - g.k0 : g.nl; // [ka, kb): the call-leaves of integration j
    const long ke = (kb == g.nl && !last_complete) ? kb - 1 : kb;                                                                 // [ka, ke): the complete ones
    double       a = j == 0 ? acc_in[e] : 0.0;
    const float* p = leaves + e;
    long         k = ka;
    for (; k + 8 <= ke; k += 8) { // eight loads in flight, the adds in leaf order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(k + u) * M];
#pragma unroll
        for (int u = 0; u < 8; ++u) a = a + (double)v[u];
    }
    for (; k < ke; ++k) a = a + (double)p[k * M];
    const bool done = (j + 1) * g.A <= end;
    if (done) {
        float v = mean ? (float)(a / (double)g.A) : (float)a;
        if constexpr (HERMITIAN) {
            if (e & 1) {
                const int r = 8 * (int)(e / (2L * N)) + 9, s = (int)__builtin_sqrtf((float)r);
                if (s * s == r) v = 0.f;
            }
        }
        out[i] = v;
    }
    if (j == g.nq - 1) {
        acc_out[e]  = done ? 0.0 : a;
        leaf_out[e] = ke < kb ? p[ke * M] : 0.f;
    }
}

template <int LEAF, bool HERMITIAN>
__global__ __launch_bounds__(256) void leaf_emit_kernel(const float* __restrict__ leaves, LeafGeom<LEAF> g, const double* __restrict__ acc_in, double* __restrict__ acc_out,
                                                        float* __restrict__ leaf_out, float* __restrict__ out, long M, int N, int mean, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) leaf_emit_element<LEAF, HERMITIAN>(i, leaves, g, acc_in, acc_out, leaf_out, out, M, N, mean);
}

constexpr size_t kLeafMaxFrames = size_t(1) << 40; // of one integration, and of one call

// ---- the carried state of one integrator: host position, two (float64 sum, float32 running leaf) carry pairs that the emit kernel ping-pongs between, and the
// leaf scratch.  The stream rule (common.hpp): reset / set_length only note that the carry is to be zero, the next call zeroes it on its own stream.
template <int LEAF, bool HERMITIAN>
struct LeafIntegrator {
    size_t       M = 0;   // floats per row
    size_t       N = 0;   // HERMITIAN: bins per baseline (M = 2 P N)
    size_t       A = 0;   // frames per integration
    size_t       pos = 0; // frames of the integration in progress (host side: n_out needs no device sync)
    bool         mean = false;
    DeviceBuffer d_acc[2], d_leaf[2], d_leaves;
    int          cur = 0;
    bool         zero_state = true;

    void   reset() { pos = 0; zero_state = true; } // zeroed on the stream of the next call
    void   set_length(size_t n_integrate) { A = n_integrate; reset(); }
    size_t pending(size_t n_frames) const { return (pos + n_frames) / A; } // rows that n_frames more frames complete

    // device check and allocation on first use (create is host code), the pending zeroing, the call's geometry, the leaf scratch
    int begin(size_t n_frames, hipStream_t st, const char* who, LeafGeom<LEAF>* g, const float** carry, float** leaves) {
        if (!d_acc[0].ptr) {
            if (const int rc = have_device(who)) return rc;
            for (int k = 0; k < 2; ++k) {
                if (const int rc = d_acc[k].ensure(M * sizeof(double))) return rc;
                // rounded up to four floats here, for every user, not through a capacity argument: the spectrum integrator's carry has always been (its
                // vector leaf kernel reads it as float4), the correlator pays at most 12 bytes for it, and no caller has the rounding to remember.  M floats
                // of it are in use, and zeroed.
                if (const int rc = d_leaf[k].ensure((M + 3) / 4 * 4 * sizeof(float))) return rc;
            }
            zero_state = true;
        }
        if (zero_state) {
            GR4_HIP_TRY(hipMemsetAsync(d_acc[cur].ptr, 0, M * sizeof(double), st));
            GR4_HIP_TRY(hipMemsetAsync(d_leaf[cur].ptr, 0, M * sizeof(float), st));
            zero_state = false;
        }
        *g = leaf_geom<LEAF>((long)pos, (long)n_frames, (long)A);
        if (const int rc = d_leaves.ensure((size_t)g->nl * M * sizeof(float))) return rc;
        *carry  = static_cast<const float*>(d_leaf[cur].ptr);
        *leaves = static_cast<float*>(d_leaves.ptr);
        return GR4HIP_OK;
    }

    // the emit kernel behind the launch that wrote the leaves; the handle moves past the call
    int finish(const LeafGeom<LEAF>& g, float* d_out, hipStream_t st) {
        const long total = g.nq * (long)M;
        hipLaunchKernelGGL((leaf_emit_kernel<LEAF, HERMITIAN>), dim3((unsigned)ceil_div(total, 256L)), dim3(256), 0, st, static_cast<const float*>(d_leaves.ptr), g,
                           static_cast<const double*>(d_acc[cur].ptr), static_cast<double*>(d_acc[cur ^ 1].ptr), static_cast<float*>(d_leaf[cur ^ 1].ptr), d_out, (long)M, (int)N,
                           mean ? 1 : 0, total);
        GR4_LAUNCH_CHECK();
        cur ^= 1;
        pos = (size_t)((g.pos + g.n) % g.A);
        return GR4HIP_OK;
    }

    // a long call in pieces of at most `piece` frames (a cut like any other: the values do not depend on it): body(first frame, frames, where its rows go)
    template <typename Body>
    int for_each_piece(size_t n_frames, size_t piece, float* d_out, Body body) {
        for (size_t f = 0; f < n_frames; f += piece) {
            const size_t n = std::min(piece, n_frames - f), done = pending(n);
            if (const int rc = body(f, n, d_out)) return rc;
            if (d_out) d_out += done * M;
        }
        return GR4HIP_OK;
    }
};

} // namespace gr4
