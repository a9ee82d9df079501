// ifft.hip -- the inverse transform and the polyphase synthesis bank on gfx950 (INVERSE_FFT.md): C-ABI gr4hip_ifft_* and gr4hip_pfb_synth_*, the kernel for
// N < 256 and the bank's streaming kernel.  The kernels for N = 256 .. 8192 are in ifft_kernels.hpp: the FFT block's frame loop between a conjugating load and
// a conjugating store.
//
//   C2C:  x[n] = sum_{k < N} X[k] e^{+2 pi i k n / N}          C2R: the same of the Hermitian expansion of bins 0 .. N/2, real parts only
//   bank: v_m = C2C of frame m;  y[m N + i] = sum_{k < P} g[k N + i] v_{m - k}[i]     float32, from 0, k ascending, one fma per term and component
//
// The transform reads its bins once and writes its samples once: streaming (nt) hints on both.  The bank's sums read every transformed frame P times: those
// loads carry no hint, the sums' stores do.
#ifndef GR4_BUF_STORE_AUX
#define GR4_BUF_STORE_AUX 2
#endif
#ifndef GR4_BUF_LOAD_AUX
#define GR4_BUF_LOAD_AUX 2
#endif
#include "ifft_kernels.hpp"
#include "history.hpp"

#include <algorithm>

namespace gr4 {

// N < 256: fft_block_kernel's layout (fpb frames per workgroup, tf = max(1, N / 8) lanes per frame, the run-time radix-8/4/2 passes in LDS)
__global__ void ifft_block_kernel(const float2* __restrict__ in, void* __restrict__ out, const float* __restrict__ window, float scale, int c2r, const float2* __restrict__ tw,
                                  FftPlanDev plan, long n_frames) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int  N     = plan.N;
    const int  tf    = plan.tf;
    const int  fl    = threadIdx.x / tf; // frame slot in block
    const int  t     = threadIdx.x - fl * tf;
    const long frame = (long)blockIdx.x * plan.fpb + fl;
    const bool live  = frame < n_frames;
    float2*    buf   = lds + (size_t)fl * N;
    if (live) {
        const float2* x = in + frame * N;
        for (int k = t; k < N; k += tf) {
            if (c2r) { // the Hermitian expansion: bin k > N/2 is the conjugate of bin N - k (conjugated twice), bins 0 and N/2 are real
                const float2 s = x[k <= N / 2 ? k : N - k];
                buf[k]         = make_float2(s.x, k == 0 || k == N / 2 ? -0.f : k < N / 2 ? -s.y : s.y);
            } else {
                const float2 s = x[k];
                buf[k]         = make_float2(s.x, -s.y);
            }
        }
    }
    __syncthreads();
    lds_passes(buf, t, tf, plan, tw);
    if (!live) return;
    for (int n = t; n < N; n += tf) {
        float2 y = make_float2(buf[n].x * scale, -buf[n].y * scale);
        if (window) { const float w = window[n]; y = make_float2(y.x * w, y.y * w); }
        if (c2r) __builtin_nontemporal_store(y.x, static_cast<float*>(out) + frame * N + n);
        else {
            __builtin_nontemporal_store(y.x, &static_cast<float2*>(out)[frame * N + n].x);
            __builtin_nontemporal_store(y.y, &static_cast<float2*>(out)[frame * N + n].y);
        }
    }
}

// The bank's P-term sums.  A lane owns C consecutive samples i of one output frame m (C = 2: 16-byte loads and stores; C = 1 where the caller's output is only
// 8-byte aligned) and walks k = 0 .. P - 1 over v[m - k] -- the call's transformed frames V, or the history ([P - 1][N], oldest first) where m - k < 0.
template <int C>
__global__ __launch_bounds__(256) void pfb_synth_combine_kernel(const float2* __restrict__ V, const float2* __restrict__ hist, const float* __restrict__ g, float2* __restrict__ y,
                                                                 int log2n, int P, long n_frames) {
    typedef float vec __attribute__((ext_vector_type(2 * C)));
    const long N = 1L << log2n, total = (n_frames << log2n) / C;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
        const long e = q * C, m = e >> log2n, i = e & (N - 1);
        vec        acc = 0.f;
#pragma unroll 4 // (the loads of four terms in flight; the fma chain keeps its order)
        for (int k = 0; k < P; ++k) {
            const long   f   = m - k; // >= -(P - 1); below 0: history frame P - 1 + f
            const float* src = reinterpret_cast<const float*>(f >= 0 ? V + f * N + i : hist + (P - 1 + f) * N + i);
            const vec    v   = *reinterpret_cast<const vec*>(src);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float h  = g[k * N + i + c];
                acc[2 * c]     = fmaf(h, v[2 * c], acc[2 * c]);
                acc[2 * c + 1] = fmaf(h, v[2 * c + 1], acc[2 * c + 1]);
            }
        }
        __builtin_nontemporal_store(acc, reinterpret_cast<vec*>(y + e));
    }
}

int fft_build_plan(size_t N, FftPlanDev* plan);                                                                             // fft.hip
int fft_upload_twiddles(size_t N, DeviceBuffer* buf);                                                                       // fft.hip

// one launch: n_frames frames of plan.N bins at d_in -> samples at d_out
static int ifft_launch(const FftPlanDev& plan, bool c2r, const float* d_in, void* d_out, const float* d_window, float scale, const float2* d_tw, long n_frames, hipStream_t st) {
    float* o = static_cast<float*>(d_out);
    switch (plan.N) {
    case 256: return ifft_fast_launch_256(c2r, d_in, o, d_window, scale, d_tw, n_frames, st);
    case 512: return ifft_fast_launch<9>(c2r, d_in, o, d_window, scale, d_tw, n_frames, st);
    case 1024: return ifft_fast_launch<10>(c2r, d_in, o, d_window, scale, d_tw, n_frames, st);
    case 2048: return ifft_fast_launch<11>(c2r, d_in, o, d_window, scale, d_tw, n_frames, st);
    case 4096: return ifft_fast_launch<12>(c2r, d_in, o, d_window, scale, d_tw, n_frames, st);
    case 8192: return ifft_fast_launch_8192(c2r, d_in, o, d_window, scale, d_tw, n_frames, st);
    default: break;
    }
    const size_t lds = (size_t)plan.fpb * plan.N * sizeof(float2); // <= 8 KiB below 256 points
    hipLaunchKernelGGL(ifft_block_kernel, dim3((unsigned)ceil_div(n_frames, (long)plan.fpb)), dim3(plan.tf * plan.fpb), lds, st, reinterpret_cast<const float2*>(d_in), d_out, d_window,
                       scale, c2r ? 1 : 0, d_tw, plan, n_frames);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

} // namespace gr4

using namespace gr4;

constexpr size_t kSynthMaxTapsPerChannel = 32;
constexpr size_t kSynthScratchBytes      = size_t(64) << 20; // the transformed frames of one piece of a call (like the integrator's scratch)

struct gr4hip_ifft {
    size_t       N = 0;
    bool         c2r = false;
    float        scale = 1.f;
    FftPlanDev   plan{};
    DeviceBuffer d_tw, d_window;
};

struct gr4hip_pfb_synth {
    size_t             N = 0, P = 0;
    float              scale = 1.f;
    std::vector<float> taps; // the host image the stream-ordered upload reads
    FftPlanDev         plan{};
    DeviceBuffer       d_taps, d_tw, d_scratch;
    CarriedHistory     hist; // the last P - 1 transformed frames: (P - 1) N complex samples (none for P = 1)
    bool               taps_dirty = false;
};

// the size rules of both handles: INVALID_ARGUMENT for what no transform has, UNSUPPORTED for what these kernels do not run
static int ifft_check_size(const char* who, size_t N) {
    GR4_REQUIRE(N >= 2, "%s: the transform needs >= 2 points (got %zu)", who, N);
    if (!is_pow2(N) || N > 8192) { set_error("%s: %zu points: the inverse runs the single-kernel transforms (powers of two <= 8192)", who, N); return GR4HIP_UNSUPPORTED; }
    return GR4HIP_OK;
}

static int synth_check_taps(const char* who, const float* h, size_t count) {
    for (size_t i = 0; i < count; ++i) GR4_REQUIRE(std::isfinite(h[i]), "%s: tap %zu is not finite", who, i);
    return GR4HIP_OK;
}

// the checks of a process call that both handles share
static int ifft_check_call(const char* who, size_t N, const void* d_in, size_t n_frames, const void* d_out, size_t out_elem, size_t fpb) {
    GR4_REQUIRE(d_in, "%s: null input", who);
    GR4_REQUIRE(d_out, "%s: null output", who);
    GR4_REQUIRE((uintptr_t)d_in % 8 == 0 && (uintptr_t)d_out % out_elem == 0, "%s: complex buffers must be aligned to 8 bytes, a real output to 4", who);
    GR4_REQUIRE(n_frames <= (size_t(1) << 40) / N, "%s: %zu frames", who, n_frames);
    // (below 256 points: one workgroup per fpb frames, no frame loop -- the grid must fit a launch)
    GR4_REQUIRE(N >= 256 || ceil_div(n_frames, fpb) <= 0x7fffffffu, "%s: %zu frames of %zu points in one call (at most %zu)", who, n_frames, N, (size_t)0x7fffffffu * fpb);
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + n_frames * N * sizeof(float2), o0 = (uintptr_t)d_out, o1 = o0 + n_frames * N * out_elem;
    GR4_REQUIRE(a1 <= o0 || o1 <= a0, "%s: the output overlaps the input", who);
    return GR4HIP_OK;
}

extern "C" {

int gr4hip_ifft_create(gr4hip_ifft_t** out, int out_dtype, size_t fft_size, int window, int flags) {
    GR4_REQUIRE(out, "ifft: null output handle");
    GR4_REQUIRE(out_dtype == GR4HIP_F32 || out_dtype == GR4HIP_C32, "ifft: output dtype must be C32 or F32 (got %d)", out_dtype);
    GR4_REQUIRE((flags & ~GR4HIP_IFFT_SCALE) == 0, "ifft: unknown flags %d", flags);
    GR4_REQUIRE(window >= GR4HIP_WIN_NONE && window <= GR4HIP_WIN_KAISER, "ifft: unknown window %d", window);
    if (const int rc = ifft_check_size("ifft", fft_size)) return rc;
    if (const int rc = have_device("ifft")) return rc;
    auto* f = new (std::nothrow) gr4hip_ifft();
    GR4_REQUIRE(f, "out of host memory");
    f->N     = fft_size;
    f->c2r   = out_dtype == GR4HIP_F32;
    f->scale = (flags & GR4HIP_IFFT_SCALE) ? 1.f / (float)fft_size : 1.f;
    int rc   = fft_build_plan(fft_size, &f->plan);
    if (!rc) rc = fft_upload_twiddles(fft_size, &f->d_tw);
    if (!rc && window != GR4HIP_WIN_NONE && window != GR4HIP_WIN_RECTANGULAR) {
        std::vector<float> w(fft_size);
        rc = make_window(window, w.data(), fft_size, 1.6f);
        if (!rc) rc = f->d_window.ensure(fft_size * sizeof(float));
        if (!rc && upload_fresh(f->d_window.ptr, w.data(), fft_size * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); set_error("ifft: window upload failed"); rc = GR4HIP_RUNTIME_ERROR; }
    }
    if (rc) { delete f; return rc; }
    *out = f;
    return GR4HIP_OK;
}

int gr4hip_ifft_process(gr4hip_ifft_t* f, const void* d_spectra, size_t n_frames, void* d_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(f, "ifft_process: null handle");
    if (n_frames == 0) return GR4HIP_OK;
    if (const int rc = ifft_check_call("ifft_process", f->N, d_spectra, n_frames, d_out, f->c2r ? sizeof(float) : sizeof(float2), (size_t)f->plan.fpb)) return rc;
    return ifft_launch(f->plan, f->c2r, static_cast<const float*>(d_spectra), d_out, static_cast<const float*>(f->d_window.ptr), f->scale, static_cast<const float2*>(f->d_tw.ptr),
                       (long)n_frames, as_stream(stream));
}

int gr4hip_ifft_destroy(gr4hip_ifft_t* f) {
    delete f;
    return GR4HIP_OK;
}

int gr4hip_pfb_synth_create(gr4hip_pfb_synth_t** out, size_t n_channels, size_t taps_per_channel, const float* h_taps, int flags) {
    GR4_REQUIRE(out, "pfb_synth: null output handle");
    GR4_REQUIRE((flags & ~GR4HIP_IFFT_SCALE) == 0, "pfb_synth: unknown flags %d", flags);
    GR4_REQUIRE(n_channels >= 2, "pfb_synth: n_channels must be >= 2 (got %zu)", n_channels);
    GR4_REQUIRE(taps_per_channel >= 1, "pfb_synth: taps_per_channel must be >= 1");
    if (const int rc = ifft_check_size("pfb_synth", n_channels)) return rc;
    if (taps_per_channel > kSynthMaxTapsPerChannel) { set_error("pfb_synth: %zu taps per channel (supported: 1 .. %zu)", taps_per_channel, kSynthMaxTapsPerChannel); return GR4HIP_UNSUPPORTED; }
    const size_t L = n_channels * taps_per_channel;
    if (h_taps)
        if (const int rc = synth_check_taps("pfb_synth", h_taps, L)) return rc;
    if (const int rc = have_device("pfb_synth")) return rc;
    auto* f = new (std::nothrow) gr4hip_pfb_synth();
    GR4_REQUIRE(f, "out of host memory");
    f->N     = n_channels;
    f->P     = taps_per_channel;
    f->scale = (flags & GR4HIP_IFFT_SCALE) ? 1.f / (float)n_channels : 1.f;
    f->taps.resize(L);
    int rc = GR4HIP_OK;
    if (h_taps) std::copy(h_taps, h_taps + L, f->taps.begin());
    else rc = gr4hip_pfb_design(f->taps.data(), f->N, f->P, GR4HIP_WIN_HAMMING, 0.f); // the analysis bank's own default
    if (!rc) rc = fft_build_plan(f->N, &f->plan);
    if (!rc) rc = fft_upload_twiddles(f->N, &f->d_tw);
    if (!rc) rc = f->d_taps.ensure(L * sizeof(float));
    if (!rc && upload_fresh(f->d_taps.ptr, f->taps.data(), L * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); set_error("pfb_synth: prototype upload failed"); rc = GR4HIP_RUNTIME_ERROR; }
    if (!rc) rc = f->hist.resize((f->P - 1) * f->N * sizeof(float2));
    if (rc) { delete f; return rc; }
    *out = f;
    return GR4HIP_OK;
}

int gr4hip_pfb_synth_set_taps(gr4hip_pfb_synth_t* f, const float* h_taps, size_t count) {
    GR4_REQUIRE(f, "pfb_synth_set_taps: null handle");
    GR4_REQUIRE(h_taps, "pfb_synth_set_taps: null taps");
    GR4_REQUIRE(count == f->N * f->P, "pfb_synth_set_taps: %zu taps, the bank has %zu x %zu", count, f->P, f->N);
    if (const int rc = synth_check_taps("pfb_synth_set_taps", h_taps, count)) return rc;
    std::copy(h_taps, h_taps + count, f->taps.begin());
    f->taps_dirty = true; // uploaded on the stream of the next call
    return GR4HIP_OK;
}

int gr4hip_pfb_synth_reset(gr4hip_pfb_synth_t* f) {
    GR4_REQUIRE(f, "pfb_synth_reset: null handle");
    f->hist.reset(); // zeroed on the stream of the next call
    return GR4HIP_OK;
}

int gr4hip_pfb_synth_process(gr4hip_pfb_synth_t* f, const void* d_spectra, size_t n_frames, void* d_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(f, "pfb_synth_process: null handle");
    if (n_frames == 0) return GR4HIP_OK;
    const size_t N = f->N, P = f->P;
    if (const int rc = ifft_check_call("pfb_synth_process", N, d_spectra, n_frames, d_out, sizeof(float2), (size_t)f->plan.fpb)) return rc;
    hipStream_t st = as_stream(stream);
    const auto  tw = static_cast<const float2*>(f->d_tw.ptr);
    if (f->taps_dirty) {
        GR4_HIP_TRY(hipMemcpyAsync(f->d_taps.ptr, f->taps.data(), f->taps.size() * sizeof(float), hipMemcpyHostToDevice, st));
        f->taps_dirty = false;
    }
    if (const int rc = f->hist.on(st)) return rc;
    if (P == 1) // one tap per channel is a synthesis window: the transform's own sink applies it, nothing is carried
        return ifft_launch(f->plan, false, static_cast<const float*>(d_spectra), d_out, static_cast<const float*>(f->d_taps.ptr), f->scale, tw, (long)n_frames, st);
    // the call in pieces through the bounded scratch: transform, sums, history of the next piece.  A piece is a cut like any other.
    const size_t piece = std::max<size_t>(1, kSynthScratchBytes / (N * sizeof(float2)));
    if (const int rc = f->d_scratch.ensure(std::min(piece, n_frames) * N * sizeof(float2))) return rc;
    auto*     V    = static_cast<float2*>(f->d_scratch.ptr);
    const int log2n = ilog2(N);
    for (size_t done = 0; done < n_frames; done += piece) {
        const size_t n  = std::min(piece, n_frames - done);
        const auto*  in = static_cast<const float*>(d_spectra) + done * N * 2;
        float2*      y  = static_cast<float2*>(d_out) + done * N;
        if (const int rc = ifft_launch(f->plan, false, in, V, nullptr, f->scale, tw, (long)n, st)) return rc;
        const auto* hist = static_cast<const float2*>(f->hist.current());
        const auto* g    = static_cast<const float*>(f->d_taps.ptr);
        if ((uintptr_t)y % 16 == 0) {
            const size_t lanes = n * N / 2;
            hipLaunchKernelGGL(pfb_synth_combine_kernel<2>, dim3((unsigned)std::min<size_t>(ceil_div(lanes, (size_t)256), 0x7fffffffu)), dim3(256), 0, st, V, hist, g, y, log2n, (int)P, (long)n);
        } else {
            const size_t lanes = n * N;
            hipLaunchKernelGGL(pfb_synth_combine_kernel<1>, dim3((unsigned)std::min<size_t>(ceil_div(lanes, (size_t)256), 0x7fffffffu)), dim3(256), 0, st, V, hist, g, y, log2n, (int)P, (long)n);
        }
        GR4_LAUNCH_CHECK();
        if (const int rc = f->hist.advance(V, n * N, (P - 1) * N, (int)sizeof(float2), st)) return rc;
    }
    return GR4HIP_OK;
}

int gr4hip_pfb_synth_destroy(gr4hip_pfb_synth_t* f) {
    delete f;
    return GR4HIP_OK;
}

} // extern "C"
