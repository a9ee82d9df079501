// pfb.hip -- the polyphase filter bank on gfx950 (critically sampled analysis bank: PFB spectrometer / channelizer, PFB.md): C-ABI gr4hip_pfb_*,
// the prototype design, the kernel for N < 256 and the history kernel.  The kernels for N = 256 .. 8192 (and the run form at 8192) are in pfb_kernels.hpp.
//
//   u_m[i] = sum_{k < P} h[k N + i] x[(m - P + 1 + k) N + i]   ->   X_m = the FFT block's forward transform of u_m   ->   spectrum / |X|^2
//
// The reference has no polyphase form: the definition is this project's, tests/pfb_oracle.py pins it.  One launch transforms a call's
// frames -- the FFT block's passes and epilogue behind another first-pass load --, a second small one on the same stream writes the history of the next call.
// The results' stores carry the FFT block's streaming hint; the front end's loads do not (every sample is read P times).
#ifndef GR4_BUF_STORE_AUX
#define GR4_BUF_STORE_AUX 2
#endif
#include "specint_kernels.hpp"
#include "history.hpp"

#include <algorithm>

namespace gr4 {

// N < 256: fft_block_kernel's layout (fpb frames per workgroup, tf = max(1, N / 8) lanes per frame, the run-time radix-8/4/2 passes in LDS)
__global__ void pfb_block_kernel(PfbFront fe, const float2* __restrict__ tw, FftPlanDev plan, FftOutputs out, long n_frames) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int  N     = plan.N;
    const int  tf    = plan.tf;
    const int  fl    = threadIdx.x / tf; // frame slot in block
    const int  t     = threadIdx.x - fl * tf;
    const long frame = (long)blockIdx.x * plan.fpb + fl;
    const bool live  = frame < n_frames;
    float2*    buf   = lds + (size_t)fl * N;
    if (live) {
        const float2* x = reinterpret_cast<const float2*>(fe.x);
        const float2* p = reinterpret_cast<const float2*>(fe.hist);
        for (int i = t; i < N; i += tf) {
            float2 u = make_float2(0.f, 0.f);
            for (int k = 0; k < fe.P; ++k) {
                const long   f = frame - (fe.P - 1) + k; // < n_frames; below 0: history frame P - 1 + f
                const float2 s = f < 0 ? p[(fe.P - 1 + f) * N + i] : x[f * N + i];
                const float  h = fe.taps[k * N + i];
                u = make_float2(fmaf(h, s.x, u.x), fmaf(h, s.y, u.y));
            }
            buf[i] = u;
        }
    }
    __syncthreads();
    lds_passes(buf, t, tf, plan, tw);
    if (!live) return;
    for (int k = t; k < N; k += tf) emit_bin(out, frame, N, k, buf[k]);
}

int fft_build_plan(size_t N, FftPlanDev* plan);       // fft.hip
int fft_upload_twiddles(size_t N, DeviceBuffer* buf); // fft.hip

} // namespace gr4

using namespace gr4;

constexpr size_t kPfbMaxTapsPerChannel = 32;

struct gr4hip_pfb {
    size_t             N = 0, P = 0;
    std::vector<float> taps; // the host image the stream-ordered upload reads
    FftPlanDev         plan{};
    DeviceBuffer       d_taps, d_tw;
    CarriedHistory     hist; // the last P - 1 frames: (P - 1) N complex samples (none for P = 1)
    long               run_length = 0; // N = 8192, P = 2 .. 4: frames per workgroup of the run form (test hook); 0: the simple form
    bool               taps_dirty = false, last_run_form = false;
};

static int pfb_design(float* h, size_t N, size_t P, int window, float beta) {
    const size_t        L = N * P;
    std::vector<double> w(L);
    if (const int rc = make_window64(window, w.data(), L, (double)beta)) return rc;
    const double mid = (double)(L - 1) * 0.5;
    for (size_t j = 0; j < L; ++j) {
        const double a = M_PI * (((double)j - mid) / (double)N);
        h[j]           = (float)(w[j] * (a == 0.0 ? 1.0 : std::sin(a) / a));
    }
    return GR4HIP_OK;
}

// the size rules shared by design and create: INVALID_ARGUMENT for what no bank has, UNSUPPORTED for what this one does not run
static int pfb_check_shape(const char* who, size_t N, size_t P) {
    GR4_REQUIRE(N >= 2, "%s: n_channels must be >= 2 (got %zu)", who, N);
    GR4_REQUIRE(P >= 1, "%s: taps_per_channel must be >= 1", who);
    if (!is_pow2(N) || N > 8192) { set_error("%s: %zu channels: the bank runs the single-kernel transforms (powers of two <= 8192)", who, N); return GR4HIP_UNSUPPORTED; }
    if (P > kPfbMaxTapsPerChannel) { set_error("%s: %zu taps per channel (supported: 1 .. %zu)", who, P, kPfbMaxTapsPerChannel); return GR4HIP_UNSUPPORTED; }
    return GR4HIP_OK;
}

static int pfb_check_taps(const char* who, const float* h, size_t count) {
    for (size_t i = 0; i < count; ++i) GR4_REQUIRE(std::isfinite(h[i]), "%s: tap %zu is not finite", who, i);
    return GR4HIP_OK;
}

// what set_taps / reset left for the next call, on that call's stream
static int pfb_apply_pending(gr4hip_pfb* f, hipStream_t st) {
    if (f->taps_dirty) {
        GR4_HIP_TRY(hipMemcpyAsync(f->d_taps.ptr, f->taps.data(), f->taps.size() * sizeof(float), hipMemcpyHostToDevice, st));
        f->taps_dirty = false;
    }
    return f->hist.on(st);
}

extern "C" {

int gr4hip_pfb_design(float* h_out, size_t n_channels, size_t taps_per_channel, int window, float beta) {
    GR4_REQUIRE(h_out, "pfb_design: null output");
    GR4_REQUIRE(n_channels >= 2 && taps_per_channel >= 1, "pfb_design: need >= 2 channels and >= 1 tap per channel");
    GR4_REQUIRE(taps_per_channel <= (size_t(1) << 30) / n_channels, "pfb_design: %zu x %zu taps", n_channels, taps_per_channel);
    return pfb_design(h_out, n_channels, taps_per_channel, window, beta);
}

int gr4hip_pfb_create(gr4hip_pfb_t** out, int in_dtype, size_t n_channels, size_t taps_per_channel, const float* h_taps, int flags) {
    GR4_REQUIRE(out, "pfb: null output handle");
    GR4_REQUIRE(in_dtype == GR4HIP_F32 || in_dtype == GR4HIP_C32, "pfb: input dtype must be C32 (got %d)", in_dtype);
    GR4_REQUIRE(flags == 0, "pfb: unknown flags %d", flags);
    if (const int rc = pfb_check_shape("pfb", n_channels, taps_per_channel)) return rc;
    if (in_dtype == GR4HIP_F32) { set_error("pfb: real input is not implemented (complex<float> streams only)"); return GR4HIP_UNSUPPORTED; }
    const size_t L = n_channels * taps_per_channel;
    if (h_taps)
        if (const int rc = pfb_check_taps("pfb", h_taps, L)) return rc;
    if (const int rc = have_device("pfb")) return rc;
    auto* f = new (std::nothrow) gr4hip_pfb();
    GR4_REQUIRE(f, "out of host memory");
    f->N = n_channels;
    f->P = taps_per_channel;
    f->taps.resize(L);
    int rc = GR4HIP_OK;
    if (h_taps) std::copy(h_taps, h_taps + L, f->taps.begin());
    else rc = pfb_design(f->taps.data(), f->N, f->P, GR4HIP_WIN_HAMMING, 0.f);
    if (!rc) rc = fft_build_plan(f->N, &f->plan);
    if (!rc) rc = fft_upload_twiddles(f->N, &f->d_tw);
    if (!rc) rc = f->d_taps.ensure(L * sizeof(float));
    if (!rc && upload_fresh(f->d_taps.ptr, f->taps.data(), L * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); set_error("pfb: prototype upload failed"); rc = GR4HIP_RUNTIME_ERROR; }
    if (!rc) rc = f->hist.resize((f->P - 1) * f->N * sizeof(float2));
    if (rc) { delete f; return rc; }
    *out = f;
    return GR4HIP_OK;
}

int gr4hip_pfb_set_taps(gr4hip_pfb_t* f, const float* h_taps, size_t count) {
    GR4_REQUIRE(f, "pfb_set_taps: null handle");
    GR4_REQUIRE(h_taps, "pfb_set_taps: null taps");
    GR4_REQUIRE(count == f->N * f->P, "pfb_set_taps: %zu taps, the bank has %zu x %zu", count, f->P, f->N);
    if (const int rc = pfb_check_taps("pfb_set_taps", h_taps, count)) return rc;
    std::copy(h_taps, h_taps + count, f->taps.begin());
    f->taps_dirty = true; // uploaded on the stream of the next call
    return GR4HIP_OK;
}

int gr4hip_pfb_reset(gr4hip_pfb_t* f) {
    GR4_REQUIRE(f, "pfb_reset: null handle");
    f->hist.reset(); // zeroed on the stream of the next call
    return GR4HIP_OK;
}

int gr4hip_pfb_process(gr4hip_pfb_t* f, const void* d_in, size_t n_frames, float* d_spectrum, float* d_mag2, gr4hip_stream_t stream) {
    GR4_REQUIRE(f, "pfb_process: null handle");
    if (n_frames == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in, "pfb_process: null input");
    GR4_REQUIRE(d_spectrum || d_mag2, "pfb_process: both outputs are null");
    GR4_REQUIRE((uintptr_t)d_in % 8 == 0 && (uintptr_t)d_spectrum % 8 == 0 && (uintptr_t)d_mag2 % 4 == 0, "pfb_process: complex buffers must be aligned to 8 bytes, |X|^2 to 4");
    const size_t N = f->N, P = f->P, n_in = n_frames * N;
    GR4_REQUIRE(n_frames <= (size_t(1) << 40) / N, "pfb_process: %zu frames", n_frames);
    // (below 256 points: one workgroup per fpb frames, no frame loop -- the grid must fit a launch)
    GR4_REQUIRE(N >= 256 || ceil_div(n_frames, (size_t)f->plan.fpb) <= 0x7fffffffu, "pfb_process: %zu frames of %zu points in one call (at most %zu)", n_frames, N, (size_t)0x7fffffffu * f->plan.fpb);
    {
        const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + n_in * sizeof(float2);
        const uintptr_t s0 = (uintptr_t)d_spectrum, s1 = s0 + n_in * sizeof(float2), m0 = (uintptr_t)d_mag2, m1 = m0 + n_in * sizeof(float);
        GR4_REQUIRE(!d_spectrum || a1 <= s0 || s1 <= a0, "pfb_process: d_spectrum overlaps d_in");
        GR4_REQUIRE(!d_mag2 || a1 <= m0 || m1 <= a0, "pfb_process: d_mag2 overlaps d_in");
    }
    hipStream_t st = as_stream(stream);
    if (const int rc = pfb_apply_pending(f, st)) return rc;
    PfbFront fe{static_cast<const float*>(d_in), static_cast<const float*>(f->hist.current()), static_cast<const float*>(f->d_taps.ptr), (int)P};
    FftOutputs o{};
    o.spectrum    = d_spectrum;
    o.mag2        = d_mag2;
    const auto tw = static_cast<const float2*>(f->d_tw.ptr);
    const long nf = (long)n_frames;
    int        rc = GR4HIP_OK;
    switch (N) {
    case 256: rc = pfb_fast_launch_256(fe, tw, o, nf, st); break;
    case 512: rc = pfb_fast_launch<9>(fe, tw, o, nf, st); break;
    case 1024: rc = pfb_fast_launch<10>(fe, tw, o, nf, st); break;
    case 2048: rc = pfb_fast_launch<11>(fe, tw, o, nf, st); break;
    case 4096: rc = pfb_fast_launch<12>(fe, tw, o, nf, st); break;
    case 8192: {
        bool taken = false; // the run form where a run length was asked for (P = 2 .. 4), the simple form otherwise: the same values
        if (f->run_length > 0) rc = pfb_run_launch_8192((int)P, fe.x, fe.hist, fe.taps, f->run_length, tw, o, nf, st, &taken);
        if (!rc && !taken) rc = pfb_fast_launch_8192(fe, tw, o, nf, st);
        f->last_run_form = taken;
        break;
    }
    default: {
        const size_t lds = (size_t)f->plan.fpb * N * sizeof(float2); // <= 8 KiB below 256 points
        hipLaunchKernelGGL(pfb_block_kernel, dim3((unsigned)ceil_div(nf, (long)f->plan.fpb)), dim3(f->plan.tf * f->plan.fpb), lds, st, fe, tw, f->plan, o, nf);
        GR4_LAUNCH_CHECK();
    }
    }
    if (rc) return rc;
    return f->hist.advance(d_in, n_in, (P - 1) * N, (int)sizeof(float2), st);
}

// |X|^2 summed over the integrator's frames (SPECTRUM_INTEGRATOR.md).  256 channels and more: pfb_fast_kernel's frame loop with the sink in place of the
// store; below that: gr4hip_pfb_process in pieces through the integrator's scratch, then its fold (the history makes the pieces one stream).
int gr4hip_pfb_power_integrate(gr4hip_pfb_t* f, gr4hip_specint_t* si, const void* d_in, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(f, "pfb_power_integrate: null handle");
    const size_t N = f->N;
    if (const int rc = specint_check(si, "pfb_power_integrate", N, d_in, N * sizeof(float2), 8, n_frames, d_out, n_out)) return rc;
    size_t done = 0;
    (void)gr4hip_specint_pending(si, n_frames, &done);
    hipStream_t st = as_stream(stream);
    if (n_frames > 0 && specint_takes_sink(si, N, f->P)) {
        if (const int rc = pfb_apply_pending(f, st)) return rc;
        SpecintLaunch L;
        if (const int rc = specint_begin(si, n_frames, st, &L)) return rc;
        const PfbFront fe{static_cast<const float*>(d_in), static_cast<const float*>(f->hist.current()), static_cast<const float*>(f->d_taps.ptr), (int)f->P};
        if (const int rc = specint_sink_pfb(N, fe, static_cast<const float2*>(f->d_tw.ptr), L, st)) return rc;
        if (const int rc = specint_finish(si, L, d_out, 1, st)) return rc;
        if (const int rc = f->hist.advance(d_in, n_frames * N, (f->P - 1) * N, (int)sizeof(float2), st)) return rc;
        f->last_run_form = false;
    } else if (n_frames > 0) {
        struct Ctx { gr4hip_pfb_t* f; const float2* in; } ctx{f, static_cast<const float2*>(d_in)};
        const auto produce = [](void* c, size_t first, size_t n, float* d_mag2, hipStream_t s) {
            auto* x = static_cast<Ctx*>(c);
            return gr4hip_pfb_process(x->f, x->in + first * x->f->N, n, nullptr, d_mag2, s);
        };
        if (const int rc = specint_compose(si, n_frames, d_out, st, produce, &ctx)) return rc;
    }
    *n_out = done;
    return GR4HIP_OK;
}

int gr4hip_pfb_destroy(gr4hip_pfb_t* f) {
    delete f;
    return GR4HIP_OK;
}

// test hook (exported, not declared in include/gr4hip.h): frames per workgroup of the run form (N = 8192, P = 2 .. 4); 0 = the simple form, the default
int gr4hip_internal_pfb_set_run_length(gr4hip_pfb_t* f, long frames) {
    GR4_REQUIRE(f, "pfb_set_run_length: null handle");
    f->run_length = frames;
    return GR4HIP_OK;
}
// test hook: 1 when the last process call took the run form
int gr4hip_internal_pfb_last_run_form(gr4hip_pfb_t* f, int* taken) {
    GR4_REQUIRE(f && taken, "pfb_last_run_form: bad arguments");
    *taken = f->last_run_form ? 1 : 0;
    return GR4HIP_OK;
}

} // extern "C"
