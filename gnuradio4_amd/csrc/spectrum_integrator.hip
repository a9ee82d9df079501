// spectrum_integrator.hip -- the spectrum integrator on gfx950 (SPECTRUM_INTEGRATOR.md): C-ABI gr4hip_specint_*, the stand-alone leaf and emit kernels, the
// handle's begin / finish steps for the entries fused into a transform's launch (gr4hip_fft_mag2_integrate in fft.hip, gr4hip_pfb_power_integrate in pfb.hip)
// and those entries' sink kernels for N = 512 .. 4096 (256 and 8192 are compiled in fft_fast_pk.hip, like the kernels they have to equal).
//
//   leaf_l[c] = (((0 + m[f0][c]) + m[f0 + 1][c]) + ...)   float32        acc[c] = ((0 + (double)leaf_0[c]) + (double)leaf_1[c]) + ...   float64
//
// The reference has no such block: the definition is this project's, tests/spectrum_integrator_oracle.py pins it.  One launch sums the call's leaves (each from
// +0, the call's first from the carried running leaf), a second small one on the same stream folds them into the float64 accumulator, writes the finished
// spectra and stores the carry of the next call into the other of two carry buffers.
#ifndef GR4_BUF_STORE_AUX
#define GR4_BUF_STORE_AUX 2
#endif
#ifndef GR4_BUF_LOAD_AUX
#define GR4_BUF_LOAD_AUX 2
#endif
#include "specint_kernels.hpp"

#include <algorithm>

namespace gr4 {

// Element i of [nl][NQ] groups of four bins: a workgroup's 256 lanes take 1024 consecutive values of the leaf scratch -- with 1024 bins or more one (bin tile,
// leaf) pair, below that several leaves, so that small spectra fill their workgroups too.  VEC: 16-byte loads (n_bins a multiple of 4, the frames aligned to 16).
template <bool VEC>
__global__ __launch_bounds__(256) void specint_leaf_kernel(const float* __restrict__ m, SpecintGeom g, const float* __restrict__ carry, float* __restrict__ leaves, int N, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int  NQ = (N + 3) / 4;
    const long k  = i / NQ;
    const int  c  = (int)(i - k * NQ) * 4;
    long       first;
    int        count;
    bool       complete;
    specint_leaf_range(g, k, &first, &count, &complete);
    const float* p = m + first * N + c;
    if constexpr (VEC) {
        float4 a = k == 0 ? *reinterpret_cast<const float4*>(carry + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        int    j = 0;
        for (; j + 8 <= count; j += 8) { // eight loads in flight, the adds in frame order
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(p + (long)(j + u) * N);
#pragma unroll
            for (int u = 0; u < 8; ++u) a = make_float4(a.x + v[u].x, a.y + v[u].y, a.z + v[u].z, a.w + v[u].w);
        }
        for (; j < count; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(p + (long)j * N);
            a              = make_float4(a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w);
        }
        *reinterpret_cast<float4*>(leaves + k * N + c) = a;
    } else {
        const int w = N - c < 4 ? N - c : 4;
        for (int e = 0; e < w; ++e) {
            float a = k == 0 ? carry[c + e] : 0.f;
            for (int j = 0; j < count; ++j) a = a + p[(long)j * N + e];
            leaves[k * N + c + e] = a;
        }
    }
}

// Element i of [nq][N]: bin c of the j-th integration the call touches.  Its leaves in ascending order into a float64 sum that starts from the carried one
// (j = 0) or from 0; a complete integration is written to out[j], the last one leaves the carry of the next call: its sum, and the call's last leaf where the
// call does not hold that leaf's end.
__global__ __launch_bounds__(256) void specint_emit_kernel(const float* __restrict__ leaves, SpecintGeom g, const double* __restrict__ acc_in, double* __restrict__ acc_out,
                                                           float* __restrict__ leaf_out, float* __restrict__ out, int N, int mean, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long j = i / N;
    const int  c = (int)(i - j * N);
    const long end = g.pos + g.n, k_last = g.nl - 1;
    long       first;
    int        count;
    bool       last_complete;
    specint_leaf_range(g, k_last, &first, &count, &last_complete);
    // call-leaves of integration j: K = j lpi .. (j + 1) lpi - 1, cut to the call's
    const long ka = j * g.lpi > g.k0 ? j * g.lpi - g.k0 : 0, kb = (j + 1) * g.lpi - g.k0 < g.nl ? (j + 1) * g.lpi - g.k0 : g.nl; // [ka, kb)
    const long ke = (kb == g.nl && !last_complete) ? kb - 1 : kb;                                  // [ka, ke): the complete ones
    double     a  = j == 0 ? acc_in[c] : 0.0;
    const float* p = leaves + c;
    long         k = ka;
    for (; k + 8 <= ke; k += 8) { // eight loads in flight, the adds in leaf order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(k + u) * N];
#pragma unroll
        for (int u = 0; u < 8; ++u) a = a + (double)v[u];
    }
    for (; k < ke; ++k) a = a + (double)p[k * N];
    const bool done = (j + 1) * g.A <= end;
    if (done) out[i] = mean ? (float)(a / (double)g.A) : (float)a;
    if (j == g.nq - 1) {
        acc_out[c]  = done ? 0.0 : a;
        leaf_out[c] = ke < kb ? p[ke * N] : 0.f;
    }
}

} // namespace gr4

using namespace gr4;

constexpr size_t kSpecintMaxBins     = size_t(1) << 20;
constexpr size_t kSpecintPieceFloats = size_t(1) << 24; // the composition's |X|^2 scratch: 64 MiB (at least one frame); at 32 MiB a 2^27-sample call measured
                                                        // 0.6 .. 0.7 of the two-call composition: 48 launches in 0.4 ms

struct gr4hip_specint {
    size_t       N = 0, A = 0;
    int          flags = 0;
    size_t       pos = 0; // frames of the integration in progress (host side: n_out needs no device sync)
    DeviceBuffer d_acc[2], d_leaf[2], d_leaves, d_mag2;
    int          cur = 0, last_path = 0;
    int          force_path = 0; // test hook: 1 = the sink wherever a kernel exists, 2 = the composition, 0 = the measured default
    bool         zero_state = true;
};

namespace gr4 {

// The sink kernels exist for 256 .. 8192 points.  A size takes its sink by default only where the entry measured faster than the composition by more than both
// spreads (SPECTRUM_INTEGRATOR.md, profiles/spectrum_integrator_rates.txt); elsewhere the kernel stays behind gr4hip_internal_specint_set_path.
// Measured at 2^27 samples per call, A = 32 / 1024 / 65536, every size (profiles/spectrum_integrator_rates_sizes.txt), sink against the two-call composition:
//   FFT block  256 .. 2048: 1.38 .. 1.65,  4096: 1.13 .. 1.15,  8192 (256 registers, one workgroup per CU): 0.97 .. 0.98
//   bank P = 1 256 .. 8192: 1.10 .. 1.33;  P = 2: 1.02 at 256, 0.59 .. 0.93 elsewhere;  P = 4: 0.50 .. 0.88 -- the slots of a workgroup are a leaf apart, so no
//   two of them share a frame any more: every frame is fetched P times where pfb_fast_kernel's neighbouring slots fetch it once
bool specint_takes_sink(const gr4hip_specint* si, size_t n_bins, size_t bank_taps) {
    if (!(is_pow2(n_bins) && n_bins >= 256 && n_bins <= 8192) || si->force_path == 2) return false;
    if (si->force_path == 1) return true;
    return bank_taps == 0 ? n_bins <= 4096 : bank_taps == 1;
}

int specint_check(const gr4hip_specint* si, const char* who, size_t n_bins, const void* d_in, size_t in_frame_bytes, size_t in_align, size_t n_frames, const float* d_out, size_t* n_out) {
    GR4_REQUIRE(si, "%s: null integrator handle", who);
    GR4_REQUIRE(n_out, "%s: null n_out", who);
    GR4_REQUIRE(si->N == n_bins, "%s: the integrator has %zu bins, the transform writes %zu values per frame", who, si->N, n_bins);
    if (n_frames == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in, "%s: null input", who);
    GR4_REQUIRE(n_frames <= (size_t(1) << 40) / si->N, "%s: %zu frames of %zu bins in one call", who, n_frames, si->N);
    const size_t n = (si->pos + n_frames) / si->A;
    GR4_REQUIRE(d_out || n == 0, "%s: null output in a call that completes %zu integrations", who, n);
    GR4_REQUIRE((uintptr_t)d_in % in_align == 0 && (uintptr_t)d_out % 4 == 0, "%s: the input must be aligned to %zu bytes, the output to 4", who, in_align);
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + n_frames * in_frame_bytes, o0 = (uintptr_t)d_out, o1 = o0 + n * si->N * sizeof(float);
    GR4_REQUIRE(n == 0 || a1 <= o0 || o1 <= a0, "%s: d_out overlaps the input", who);
    return GR4HIP_OK;
}

int specint_begin(gr4hip_specint* si, size_t n_frames, hipStream_t st, SpecintLaunch* L) {
    const size_t N = si->N;
    if (!si->d_acc[0].ptr) { // the carry buffers, on first use: create is host code
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
            (void)hipGetLastError();
            set_error("spectrum integrator: no HIP device visible");
            return GR4HIP_NO_DEVICE;
        }
        for (int k = 0; k < 2; ++k) {
            if (const int rc = si->d_acc[k].ensure(N * sizeof(double))) return rc;
            if (const int rc = si->d_leaf[k].ensure((N + 3) / 4 * 4 * sizeof(float))) return rc;
        }
        si->zero_state = true;
    }
    if (si->zero_state) {
        GR4_HIP_TRY(hipMemsetAsync(si->d_acc[si->cur].ptr, 0, N * sizeof(double), st));
        GR4_HIP_TRY(hipMemsetAsync(si->d_leaf[si->cur].ptr, 0, N * sizeof(float), st));
        si->zero_state = false;
    }
    L->geom = specint_geom((long)si->pos, (long)n_frames, (long)si->A);
    if (const int rc = si->d_leaves.ensure((size_t)L->geom.nl * N * sizeof(float))) return rc;
    L->carry  = static_cast<const float*>(si->d_leaf[si->cur].ptr);
    L->leaves = static_cast<float*>(si->d_leaves.ptr);
    return GR4HIP_OK;
}

int specint_finish(gr4hip_specint* si, const SpecintLaunch& L, float* d_out, int path, hipStream_t st) {
    const long total = L.geom.nq * (long)si->N;
    hipLaunchKernelGGL(specint_emit_kernel, dim3((unsigned)ceil_div(total, 256L)), dim3(256), 0, st, (const float*)L.leaves, L.geom, static_cast<const double*>(si->d_acc[si->cur].ptr),
                       static_cast<double*>(si->d_acc[si->cur ^ 1].ptr), static_cast<float*>(si->d_leaf[si->cur ^ 1].ptr), d_out, (int)si->N, (si->flags & GR4HIP_SPECINT_MEAN) ? 1 : 0, total);
    GR4_LAUNCH_CHECK();
    si->cur ^= 1;
    si->pos       = (size_t)((L.geom.pos + L.geom.n) % L.geom.A);
    si->last_path = path;
    return GR4HIP_OK;
}

// frames already in HBM: the stand-alone fold
static int specint_fold(gr4hip_specint* si, const float* d_frames, size_t n_frames, float* d_out, int path, hipStream_t st) {
    SpecintLaunch L;
    if (const int rc = specint_begin(si, n_frames, st, &L)) return rc;
    const int  N     = (int)si->N;
    const long total = L.geom.nl * (long)((N + 3) / 4);
    const dim3 grid((unsigned)ceil_div(total, 256L));
    if (N % 4 == 0 && (uintptr_t)d_frames % 16 == 0) hipLaunchKernelGGL(specint_leaf_kernel<true>, grid, dim3(256), 0, st, d_frames, L.geom, L.carry, L.leaves, N, total);
    else hipLaunchKernelGGL(specint_leaf_kernel<false>, grid, dim3(256), 0, st, d_frames, L.geom, L.carry, L.leaves, N, total);
    GR4_LAUNCH_CHECK();
    return specint_finish(si, L, d_out, path, st);
}

int specint_compose(gr4hip_specint* si, size_t n_frames, float* d_out, hipStream_t st, int (*produce)(void* ctx, size_t first, size_t n, float* d_mag2, hipStream_t st), void* ctx) {
    const size_t piece = std::max<size_t>(1, kSpecintPieceFloats / si->N);
    if (const int rc = si->d_mag2.ensure(std::min(piece, n_frames) * si->N * sizeof(float))) return rc;
    float* m = static_cast<float*>(si->d_mag2.ptr);
    for (size_t f = 0; f < n_frames; f += piece) { // (a cut like any other: the values do not depend on it)
        const size_t n = std::min(piece, n_frames - f), done = (si->pos + n) / si->A;
        if (const int rc = produce(ctx, f, n, m, st)) return rc;
        if (const int rc = specint_fold(si, m, n, d_out, 2, st)) return rc;
        if (d_out) d_out += done * si->N;
    }
    return GR4HIP_OK;
}

int specint_sink_fft(size_t N, const float* x, const float* window, const float2* tw, const SpecintLaunch& L, hipStream_t st) {
    switch (N) {
    case 256: return fft_sink_launch_256(x, window, tw, L, st);
    case 512: return fft_sink_launch<9, 4>(x, window, tw, L, st);
    case 1024: return fft_sink_launch<10, 4>(x, window, tw, L, st);
    case 2048: return fft_sink_launch<11, 4>(x, window, tw, L, st);
    case 4096: return fft_sink_launch<12, 2>(x, window, tw, L, st);
    case 8192: return fft_sink_launch_8192(x, window, tw, L, st);
    default: set_error("spectrum integrator: internal: no sink kernel for %zu points", N); return GR4HIP_RUNTIME_ERROR;
    }
}

int specint_sink_pfb(size_t N, const PfbFront& bank, const float2* tw, const SpecintLaunch& L, hipStream_t st) {
    switch (N) {
    case 256: return pfb_sink_launch_256(bank, tw, L, st);
    case 512: return pfb_sink_launch<9, 4>(bank, tw, L, st);
    case 1024: return pfb_sink_launch<10, 4>(bank, tw, L, st);
    case 2048: return pfb_sink_launch<11, 2>(bank, tw, L, st);
    case 4096: return pfb_sink_launch<12, 2>(bank, tw, L, st);
    case 8192: return pfb_sink_launch_8192(bank, tw, L, st);
    default: set_error("spectrum integrator: internal: no sink kernel for %zu points", N); return GR4HIP_RUNTIME_ERROR;
    }
}

} // namespace gr4

extern "C" {

size_t gr4hip_specint_leaf(void) { return (size_t)kSpecintLeaf; }

int gr4hip_specint_create(gr4hip_specint_t** out, size_t n_bins, size_t n_integrate, int flags) {
    GR4_REQUIRE(out, "specint: null output handle");
    GR4_REQUIRE(n_bins >= 2, "specint: n_bins must be >= 2 (got %zu)", n_bins);
    GR4_REQUIRE(n_integrate >= 1, "specint: n_integrate must be >= 1");
    GR4_REQUIRE((flags & ~GR4HIP_SPECINT_MEAN) == 0, "specint: unknown flags %d", flags);
    GR4_REQUIRE(n_integrate <= (size_t(1) << 40), "specint: n_integrate %zu", n_integrate);
    if (n_bins > kSpecintMaxBins) { set_error("specint: %zu bins (supported: up to %zu)", n_bins, kSpecintMaxBins); return GR4HIP_UNSUPPORTED; }
    auto* s = new (std::nothrow) gr4hip_specint();
    GR4_REQUIRE(s, "out of host memory");
    s->N     = n_bins;
    s->A     = n_integrate;
    s->flags = flags;
    *out     = s; // the device buffers come with the first process call: everything up to there is host code
    return GR4HIP_OK;
}

int gr4hip_specint_reset(gr4hip_specint_t* s) {
    GR4_REQUIRE(s, "specint_reset: null handle");
    s->pos        = 0;
    s->zero_state = true; // zeroed on the stream of the next call
    return GR4HIP_OK;
}

int gr4hip_specint_set_length(gr4hip_specint_t* s, size_t n_integrate) {
    GR4_REQUIRE(s, "specint_set_length: null handle");
    GR4_REQUIRE(n_integrate >= 1 && n_integrate <= (size_t(1) << 40), "specint_set_length: n_integrate must be >= 1 (got %zu)", n_integrate);
    s->A = n_integrate;
    return gr4hip_specint_reset(s);
}

int gr4hip_specint_pending(const gr4hip_specint_t* s, size_t n_frames, size_t* n_out) {
    GR4_REQUIRE(s && n_out, "specint_pending: null argument");
    GR4_REQUIRE(n_frames <= (size_t(1) << 40), "specint_pending: %zu frames", n_frames);
    *n_out = (s->pos + n_frames) / s->A;
    return GR4HIP_OK;
}

int gr4hip_specint_process(gr4hip_specint_t* s, const float* d_frames, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(s, "specint_process: null handle");
    if (const int rc = specint_check(s, "specint_process", s->N, d_frames, s->N * sizeof(float), 4, n_frames, d_out, n_out)) return rc;
    const size_t n = (s->pos + n_frames) / s->A;
    if (n_frames > 0)
        if (const int rc = specint_fold(s, d_frames, n_frames, d_out, 0, as_stream(stream))) return rc;
    *n_out = n;
    return GR4HIP_OK;
}

int gr4hip_specint_destroy(gr4hip_specint_t* s) {
    delete s;
    return GR4HIP_OK;
}

// test hook (exported, not declared in include/gr4hip.h): how the last fused entry ran -- 1 = the sink in the transform's launch, 2 = the composition
// (0: the handle's last call was gr4hip_specint_process, or none)
int gr4hip_internal_specint_last_path(gr4hip_specint_t* s, int* path) {
    GR4_REQUIRE(s && path, "specint_last_path: bad arguments");
    *path = s->last_path;
    return GR4HIP_OK;
}

// test hook: 1 = the fused entries take the sink wherever a kernel exists, 2 = the composition, 0 = the default
int gr4hip_internal_specint_set_path(gr4hip_specint_t* s, int path) {
    GR4_REQUIRE(s && path >= 0 && path <= 2, "specint_set_path: bad arguments");
    s->force_path = path;
    return GR4HIP_OK;
}

} // extern "C"
