// spectrum_integrator.hip -- the spectrum integrator on gfx950 (SPECTRUM_INTEGRATOR.md): C-ABI gr4hip_specint_*, the stand-alone leaf kernel, the handle's
// begin / finish steps for the entries fused into another block's launch (gr4hip_fft_mag2_integrate in fft.hip, gr4hip_pfb_power_integrate in pfb.hip,
// gr4hip_beamform_power_integrate in beamformer.hip) and the sink kernels for N = 512 .. 4096 (256 and 8192 are compiled in fft_fast_pk.hip, like the kernels
// they have to equal).
//
//   leaf_l[c] = (((0 + m[f0][c]) + m[f0 + 1][c]) + ...)   float32        acc[c] = ((0 + (double)leaf_0[c]) + (double)leaf_1[c]) + ...   float64
//
// The reference has no such block: the definition is this project's, tests/spectrum_integrator_oracle.py pins it.  One launch sums the call's leaves, the emit
// kernel folds them and leaves the carry of the next call: the scheme and its carried state are leaf_integrator.hpp's, with leaves of 32 frames.
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
    leaf_range(g, k, &first, &count, &complete);
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

} // namespace gr4

using namespace gr4;

constexpr size_t kSpecintMaxBins     = size_t(1) << 20;
constexpr size_t kSpecintPieceFloats = size_t(1) << 24; // the composition's |X|^2 scratch: 64 MiB (at least one frame); at 32 MiB a 2^27-sample call measured
                                                        // 0.6 .. 0.7 of the two-call composition: 48 launches in 0.4 ms

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
    const size_t N = si->integ.M;
    GR4_REQUIRE(N == n_bins, "%s: the integrator has %zu bins, the transform writes %zu values per frame", who, N, n_bins);
    if (n_frames == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in, "%s: null input", who);
    GR4_REQUIRE(n_frames <= kLeafMaxFrames / N, "%s: %zu frames of %zu bins in one call", who, n_frames, N);
    const size_t n = si->integ.pending(n_frames);
    GR4_REQUIRE(d_out || n == 0, "%s: null output in a call that completes %zu integrations", who, n);
    GR4_REQUIRE((uintptr_t)d_in % in_align == 0 && (uintptr_t)d_out % 4 == 0, "%s: the input must be aligned to %zu bytes, the output to 4", who, in_align);
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + n_frames * in_frame_bytes, o0 = (uintptr_t)d_out, o1 = o0 + n * N * sizeof(float);
    GR4_REQUIRE(n == 0 || a1 <= o0 || o1 <= a0, "%s: d_out overlaps the input", who);
    return GR4HIP_OK;
}

int specint_begin(gr4hip_specint* si, size_t n_frames, hipStream_t st, SpecintLaunch* L) {
    return si->integ.begin(n_frames, st, "spectrum integrator", &L->geom, &L->carry, &L->leaves);
}

int specint_finish(gr4hip_specint* si, const SpecintLaunch& L, float* d_out, int path, hipStream_t st) {
    if (const int rc = si->integ.finish(L.geom, d_out, st)) return rc;
    si->last_path = path;
    return GR4HIP_OK;
}

// frames already in HBM: the stand-alone fold
static int specint_fold(gr4hip_specint* si, const float* d_frames, size_t n_frames, float* d_out, int path, hipStream_t st) {
    SpecintLaunch L;
    if (const int rc = specint_begin(si, n_frames, st, &L)) return rc;
    const int  N     = (int)si->integ.M;
    const long total = L.geom.nl * (long)((N + 3) / 4);
    const dim3 grid((unsigned)ceil_div(total, 256L));
    if (N % 4 == 0 && (uintptr_t)d_frames % 16 == 0) hipLaunchKernelGGL(specint_leaf_kernel<true>, grid, dim3(256), 0, st, d_frames, L.geom, L.carry, L.leaves, N, total);
    else hipLaunchKernelGGL(specint_leaf_kernel<false>, grid, dim3(256), 0, st, d_frames, L.geom, L.carry, L.leaves, N, total);
    GR4_LAUNCH_CHECK();
    return specint_finish(si, L, d_out, path, st);
}

int specint_compose(gr4hip_specint* si, size_t n_frames, float* d_out, hipStream_t st, int (*produce)(void* ctx, size_t first, size_t n, float* d_mag2, hipStream_t st), void* ctx) {
    const size_t N = si->integ.M, piece = std::max<size_t>(1, kSpecintPieceFloats / N);
    if (const int rc = si->d_mag2.ensure(std::min(piece, n_frames) * N * sizeof(float))) return rc;
    float* m = static_cast<float*>(si->d_mag2.ptr);
    return si->integ.for_each_piece(n_frames, piece, d_out, [&](size_t f, size_t n, float* out) {
        if (const int rc = produce(ctx, f, n, m, st)) return rc;
        return specint_fold(si, m, n, out, 2, st);
    });
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
    GR4_REQUIRE(n_integrate <= kLeafMaxFrames, "specint: n_integrate %zu", n_integrate);
    if (n_bins > kSpecintMaxBins) { set_error("specint: %zu bins (supported: up to %zu)", n_bins, kSpecintMaxBins); return GR4HIP_UNSUPPORTED; }
    auto* s = new (std::nothrow) gr4hip_specint();
    GR4_REQUIRE(s, "out of host memory");
    s->integ.M    = n_bins;
    s->integ.A    = n_integrate;
    s->integ.mean = (flags & GR4HIP_SPECINT_MEAN) != 0;
    *out          = s; // the device buffers come with the first process call: everything up to there is host code
    return GR4HIP_OK;
}

int gr4hip_specint_reset(gr4hip_specint_t* s) {
    GR4_REQUIRE(s, "specint_reset: null handle");
    s->integ.reset();
    return GR4HIP_OK;
}

int gr4hip_specint_set_length(gr4hip_specint_t* s, size_t n_integrate) {
    GR4_REQUIRE(s, "specint_set_length: null handle");
    GR4_REQUIRE(n_integrate >= 1 && n_integrate <= kLeafMaxFrames, "specint_set_length: n_integrate must be >= 1 (got %zu)", n_integrate);
    s->integ.set_length(n_integrate);
    return GR4HIP_OK;
}

int gr4hip_specint_pending(const gr4hip_specint_t* s, size_t n_frames, size_t* n_out) {
    GR4_REQUIRE(s && n_out, "specint_pending: null argument");
    GR4_REQUIRE(n_frames <= kLeafMaxFrames, "specint_pending: %zu frames", n_frames);
    *n_out = s->integ.pending(n_frames);
    return GR4HIP_OK;
}

int gr4hip_specint_process(gr4hip_specint_t* s, const float* d_frames, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(s, "specint_process: null handle");
    if (const int rc = specint_check(s, "specint_process", s->integ.M, d_frames, s->integ.M * sizeof(float), 4, n_frames, d_out, n_out)) return rc;
    const size_t n = s->integ.pending(n_frames);
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
