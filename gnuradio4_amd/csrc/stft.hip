// stft.hip -- overlapped and skipped FFT frames on gfx950 (the reference's `stride` setting of the FFT block, stated for a stream: OVERLAPPED_FFT.md):
// C-ABI gr4hip_stft_*, the stream rule, the gather kernel and the dispatch.  The hop front end and its kernels are in stft_kernels.hpp.
//
//   frame m of a stream = samples [m S, m S + N)   ->   the FFT block's window, forward DFT and outputs, per frame
//
// Native path (complex frames of 256 .. 8192 points): fft_fast_kernel's frame loop behind HopFront reads the frames where they lie.  The frames that begin in
// the carried history run through the same kernel over a staging span of fewer than 2 N samples (the history's tail followed by the head of the input).
// Gather path (everything else, short calls that have a seam, and GR4HIP_STFT_GATHER = 1): one frame_gather launch per piece copies the frames into a bounded scratch, the FFT block's own kernels
// run behind it.  The handle carries the last N - 1 samples in a CarriedHistory; a second small launch on the same stream writes the next call's.
#ifndef GR4_BUF_STORE_AUX
#define GR4_BUF_STORE_AUX 2
#endif
#include "stft_kernels.hpp"
#include "specint_kernels.hpp"
#include "history.hpp"

#include <algorithm>

namespace gr4 {

// dst[m][i] = (hist ++ x)[H + p0 + m S + i], i < N, m < n_frames: frames of N elements that start S elements apart, the first at element p0 of x (p0 >= -H; below 0
// the elements come from the history's tail), copied into contiguous frames.  W is the element as the lane moves it (a float, or a float2 as one 8-byte word).
// tpf lanes per frame, 256 / tpf frames per workgroup.  A frame whose source and destination are both 16-byte aligned and that lies in x moves 16 bytes per lane
// and step; every other one (S odd: every second frame; the frames that touch the history) moves element by element.
template <typename W>
__global__ __launch_bounds__(256) void frame_gather_kernel(const W* __restrict__ x, const W* __restrict__ hist, long H, long p0, long S, long N, long n_frames, W* __restrict__ dst, int tpf) {
    constexpr long VE = 16 / (long)sizeof(W);
    const int      fl = threadIdx.x / tpf, t = threadIdx.x - fl * tpf;
    const long     m = (long)blockIdx.x * (256 / tpf) + fl;
    if (m >= n_frames) return;
    const long p = p0 + m * S;
    W*         d = dst + m * N;
    if (p >= 0 && (((uintptr_t)(x + p) | (uintptr_t)d) & 15) == 0) {
        const long   nv = N / VE;
        const uint4* s4 = reinterpret_cast<const uint4*>(x + p);
        uint4*       d4 = reinterpret_cast<uint4*>(d);
        for (long i = t; i < nv; i += tpf) d4[i] = s4[i];
        for (long i = nv * VE + t; i < N; i += tpf) d[i] = x[p + i];
    } else {
        for (long i = t; i < N; i += tpf) {
            const long j = p + i;
            d[i]         = j < 0 ? hist[H + j] : x[j];
        }
    }
}

static int frame_gather_launch(int elem, const void* x, const void* hist, long H, long p0, long S, long N, long n_frames, void* dst, hipStream_t st) {
    int tpf = 1;
    while (tpf < 256 && (long)tpf * 16 < N * elem) tpf <<= 1;
    const dim3 grid((unsigned)ceil_div(n_frames, (long)(256 / tpf)));
    if (elem == 4)
        hipLaunchKernelGGL(frame_gather_kernel<unsigned>, grid, dim3(256), 0, st, static_cast<const unsigned*>(x), static_cast<const unsigned*>(hist), H, p0, S, N, n_frames, static_cast<unsigned*>(dst), tpf);
    else
        hipLaunchKernelGGL(frame_gather_kernel<unsigned long long>, grid, dim3(256), 0, st, static_cast<const unsigned long long*>(x), static_cast<const unsigned long long*>(hist), H, p0, S, N, n_frames,
                           static_cast<unsigned long long*>(dst), tpf);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

// the seam's staging span: dst[i] = (hist ++ x)[H - n_hist + i], i < span -- the history's last n_hist samples, then the head of the input; one complex sample
// (one 8-byte word) per lane, 256 per workgroup, both parts coalesced
__global__ __launch_bounds__(256) void seam_stage_kernel(const unsigned long long* __restrict__ x, const unsigned long long* __restrict__ hist, long H, long n_hist, long span,
                                                         unsigned long long* __restrict__ dst) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= span) return;
    dst[i] = i < n_hist ? hist[H - n_hist + i] : x[i - n_hist];
}

static int hop_launch(size_t N, const HopFront& fe, const float* win, const float2* tw, const FftOutputs& o, long nf, hipStream_t st) {
    switch (N) {
    case 256: return hop_fast_launch_256(fe, win, tw, o, nf, st);
    case 512: return hop_fast_launch<9>(fe, win, tw, o, nf, st);
    case 1024: return hop_fast_launch<10>(fe, win, tw, o, nf, st);
    case 2048: return hop_fast_launch<11>(fe, win, tw, o, nf, st);
    case 4096: return hop_fast_launch<12>(fe, win, tw, o, nf, st);
    case 8192: return hop_fast_launch_8192(fe, win, tw, o, nf, st);
    default: set_error("stft: internal: no hop kernel for %zu points", N); return GR4HIP_RUNTIME_ERROR;
    }
}

// the same outputs, `frames` frames further on
static FftOutputs outputs_from(FftOutputs o, long frames, long N) {
    const long nout = o.real_input ? N / 2 : N;
    if (o.spectrum) o.spectrum += frames * N * 2;
    if (o.mag2) o.mag2 += frames * N;
    if (o.re) o.re += frames * nout;
    if (o.im) o.im += frames * nout;
    if (o.mag) o.mag += frames * nout;
    if (o.phase) o.phase += frames * nout;
    if (o.phase_raw) o.phase_raw += frames * nout;
    if (o.ranges) o.ranges += frames * 8;
    return o;
}

constexpr size_t kStftPieceBytes = size_t(64) << 20; // the gather path's scratch (like the integrator's)
constexpr size_t kStftMaxSamples = size_t(1) << 40;
// frames x points of a call with a seam up to which the gather path serves it (profiles/stft_rates.txt: where it is ahead of the staging launch + second hop launch)
inline size_t stft_seam_gather_values(size_t N) { return N >= 8192 ? size_t(1) << 17 : size_t(1) << 21; }

} // namespace gr4

using namespace gr4;

struct gr4hip_stft {
    gr4hip_fft_t*  fft = nullptr; // the FFT block: tables, plans, kernels, flags
    FftBlockView   v{};
    size_t         N = 0, S = 0;
    int            elem = 8;      // bytes per input sample
    bool           native = false; // complex frames of 256 .. 8192 points: the hop front end
    long           off = 0;       // start of the next frame relative to the next call's first sample, >= -(N - 1)
    CarriedHistory hist;          // the last N - 1 samples
    DeviceBuffer   d_stage, d_frames;
    // what the last call enqueued (gr4hip_internal_stft_last_path): {frames the hop kernel read from the input, frames it read from the staging span, frames of the
    // gather path, launches: hop, staging, gather and history-carry kernels plus one per run of the FFT block's kernels behind a gather}
    long long last_path[4] = {0, 0, 0, 0};
    ~gr4hip_stft() { if (fft) gr4hip_fft_destroy(fft); }
};

// THE RULE: the frames a call of n_in samples emits when the next frame starts at `off` relative to its first sample (host arithmetic, no handle)
static size_t stft_rule(size_t N, size_t S, long off, size_t n_in) {
    const long avail = (long)n_in - off;
    return avail < (long)N ? 0 : (size_t)((avail - (long)N) / (long)S + 1);
}
static size_t stft_count(const gr4hip_stft* h, size_t n_in) { return stft_rule(h->N, h->S, h->off, n_in); }

namespace {
struct HopCtx {
    gr4hip_stft* h;
    const float* d_in;
    long         start; // of the launch's first frame relative to d_in
    long         seam;  // its frames that begin in the history
};
} // namespace

static int stft_hop_front(void* c, const FftOutputs& o, long n_frames, hipStream_t st) {
    auto*         x = static_cast<HopCtx*>(c);
    gr4hip_stft*  h = x->h;
    const long    S = (long)h->S, N = (long)h->N, ks = std::min(x->seam, n_frames);
    if (ks > 0) { // the staging span: (ks - 1) S + N < 2 N samples from sample x->start (< 0) on
        const long span = (ks - 1) * S + N;
        if (const int rc = h->d_stage.ensure((size_t)(2 * N) * sizeof(float2))) return rc;
        hipLaunchKernelGGL(seam_stage_kernel, dim3((unsigned)ceil_div(span, 256L)), dim3(256), 0, st, reinterpret_cast<const unsigned long long*>(x->d_in),
                           static_cast<const unsigned long long*>(h->hist.current()), N - 1, -x->start, span, static_cast<unsigned long long*>(h->d_stage.ptr));
        GR4_LAUNCH_CHECK();
        if (const int rc = hop_launch(h->N, HopFront{static_cast<const float*>(h->d_stage.ptr), S}, h->v.window, h->v.tw, o, ks, st)) return rc;
        h->last_path[1] += ks;
        h->last_path[3] += 2;
    }
    if (n_frames > ks) {
        if (const int rc = hop_launch(h->N, HopFront{x->d_in + 2 * (x->start + ks * S), S}, h->v.window, h->v.tw, outputs_from(o, ks, N), n_frames - ks, st)) return rc;
        h->last_path[0] += n_frames - ks;
        h->last_path[3] += 1;
    }
    return GR4HIP_OK;
}

// frames [first, first + n) of the call about to be made with d_in; the handle's stream position is not moved.  `o` names spectrum / mag2 / mag / re / im
static int stft_emit(gr4hip_stft* h, const void* d_in, size_t first, size_t n, const FftOutputs& o, float* d_phase, float* d_ranges, gr4hip_stream_t stream) {
    const long N = (long)h->N, S = (long)h->S, start = h->off + (long)first * S;
    // GR4HIP_STFT_GATHER: 1 = the gather path everywhere, 2 = the hop kernels wherever they exist, 0 = the hop kernels except for a call that has a seam and
    // few values: there the staging launch and the second hop launch cost more than the gather path's copy (OVERLAPPED_FFT.md, measured); the same bits
    const int  sw    = dev_switch(kDevStftGather);
    const bool shortSeam = start < 0 && n * (size_t)N <= stft_seam_gather_values((size_t)N);
    if (h->native && sw != 1 && (sw == 2 || !shortSeam)) {
        HopCtx ctx{h, static_cast<const float*>(d_in), start, start < 0 ? std::min((long)n, (-start + S - 1) / S) : 0};
        return fft_block_run(h->fft, nullptr, n, o, d_phase, d_ranges, stft_hop_front, &ctx, stream);
    }
    const long   nout  = h->elem == 4 ? N / 2 : N;
    const size_t piece = std::max<size_t>(1, kStftPieceBytes / ((size_t)N * h->elem));
    if (const int rc = h->d_frames.ensure(piece * (size_t)N * h->elem)) return rc; // sized once per handle, for a whole piece: never replaced while launches that read it are queued
    for (size_t f0 = 0; f0 < n; f0 += piece) {
        const size_t nf = std::min(piece, n - f0);
        if (const int rc = frame_gather_launch(h->elem, d_in, h->hist.current(), N - 1, start + (long)f0 * S, S, N, (long)nf, h->d_frames.ptr, as_stream(stream))) return rc;
        FftOutputs of = o;
        of.real_input = h->elem == 4;
        of            = outputs_from(of, (long)f0, N);
        if (const int rc = fft_block_run(h->fft, h->d_frames.ptr, nf, of, d_phase ? d_phase + f0 * nout : nullptr, d_ranges ? d_ranges + f0 * 8 : nullptr, nullptr, nullptr, stream)) return rc;
        h->last_path[2] += (long long)nf;
        h->last_path[3] += 2;
    }
    return GR4HIP_OK;
}

// the handle moves past the call's n_in samples, k frames of them emitted
static int stft_commit(gr4hip_stft* h, const void* d_in, size_t n_in, size_t k, hipStream_t st) {
    if (const int rc = h->hist.advance(d_in, n_in, h->N - 1, h->elem, st)) return rc;
    h->last_path[3] += 1;
    h->off += (long)(k * h->S) - (long)n_in;
    return GR4HIP_OK;
}

struct StftOut {
    const void* p;
    size_t      frame_bytes, align;
    const char* name;
};

// the refusals shared by the entries, before any device work; *k = the frames the call emits.  Returns 1 for an empty call (nothing to do)
static int stft_check(gr4hip_stft* h, const char* who, const void* d_in, size_t n_in, size_t* n_frames, const StftOut* outs, int n_outs, size_t* k) {
    GR4_REQUIRE(h, "%s: null handle", who);
    std::fill(h->last_path, h->last_path + 4, 0LL);
    GR4_REQUIRE(n_frames, "%s: null n_frames", who);
    *n_frames = 0;
    if (n_in == 0) return 1;
    GR4_REQUIRE(d_in, "%s: null input", who);
    GR4_REQUIRE((uintptr_t)d_in % (uintptr_t)h->elem == 0, "%s: the input must be aligned to %d bytes", who, h->elem);
    GR4_REQUIRE(n_in <= kStftMaxSamples, "%s: %zu samples in one call", who, n_in);
    bool any = false;
    for (int i = 0; i < n_outs; ++i) any = any || outs[i].p;
    GR4_REQUIRE(any, "%s: every output is null", who);
    *k = stft_count(h, n_in);
    GR4_REQUIRE(*k <= kStftMaxSamples / h->N, "%s: %zu frames of %zu points in one call", who, *k, h->N);
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + n_in * h->elem;
    for (int i = 0; i < n_outs; ++i) {
        if (!outs[i].p) continue;
        const uintptr_t o0 = (uintptr_t)outs[i].p, o1 = o0 + *k * outs[i].frame_bytes;
        GR4_REQUIRE(o0 % outs[i].align == 0, "%s: %s must be aligned to %zu bytes", who, outs[i].name, outs[i].align);
        GR4_REQUIRE(*k == 0 || a1 <= o0 || o1 <= a0, "%s: %s overlaps d_in", who, outs[i].name);
    }
    return GR4HIP_OK;
}

static int stft_run(gr4hip_stft* h, const char* who, const void* d_in, size_t n_in, const FftOutputs& o, float* d_phase, float* d_ranges, size_t* n_frames, const StftOut* outs, int n_outs,
                    gr4hip_stream_t stream) {
    size_t    k  = 0;
    const int rc = stft_check(h, who, d_in, n_in, n_frames, outs, n_outs, &k);
    if (rc) return rc == 1 ? GR4HIP_OK : rc;
    hipStream_t st = as_stream(stream);
    if (const int e = h->hist.on(st)) return e;
    if (k > 0)
        if (const int e = stft_emit(h, d_in, 0, k, o, d_phase, d_ranges, stream)) return e;
    if (const int e = stft_commit(h, d_in, n_in, k, st)) return e;
    *n_frames = k;
    return GR4HIP_OK;
}

extern "C" {

int gr4hip_stft_create(gr4hip_stft_t** out, int in_dtype, size_t fft_size, size_t stride, int window, int flags) {
    GR4_REQUIRE(out, "stft: null output handle");
    GR4_REQUIRE(in_dtype == GR4HIP_F32 || in_dtype == GR4HIP_C32, "stft: input dtype must be F32 or C32 (got %d)", in_dtype);
    GR4_REQUIRE(fft_size >= 2, "stft: fft_size must be >= 2 (got %zu)", fft_size);
    if (stride == 0) stride = fft_size;
    if (stride > kStftMaxStride) { set_error("stft: stride %zu (supported: 1 .. %zu)", stride, kStftMaxStride); return GR4HIP_UNSUPPORTED; }
    if (const int rc = have_device("stft")) return rc;
    auto* h = new (std::nothrow) gr4hip_stft();
    GR4_REQUIRE(h, "out of host memory");
    int rc = gr4hip_fft_create(&h->fft, in_dtype, fft_size, window, flags);
    if (!rc) {
        h->v      = fft_block_view(h->fft);
        h->N      = fft_size;
        h->S      = stride;
        h->elem   = in_dtype == GR4HIP_C32 ? 8 : 4;
        h->native = in_dtype == GR4HIP_C32 && h->v.kind == 0 && !h->v.smooth && fft_size >= 256;
        rc        = h->hist.resize((fft_size - 1) * h->elem);
    }
    if (rc) { delete h; return rc; }
    *out = h;
    return GR4HIP_OK;
}

int gr4hip_stft_reset(gr4hip_stft_t* h) {
    GR4_REQUIRE(h, "stft_reset: null handle");
    h->hist.reset(); // zeroed on the stream of the next call
    h->off = 0;
    return GR4HIP_OK;
}

int gr4hip_stft_pending(const gr4hip_stft_t* h, size_t n_in, size_t* n_frames) {
    GR4_REQUIRE(h && n_frames, "stft_pending: null argument");
    GR4_REQUIRE(n_in <= kStftMaxSamples, "stft_pending: %zu samples", n_in);
    *n_frames = stft_count(h, n_in);
    return GR4HIP_OK;
}

int gr4hip_stft_process(gr4hip_stft_t* h, const void* d_in, size_t n_in, float* d_mag, float* d_phase, float* d_re, float* d_im, float* d_ranges, size_t* n_frames, gr4hip_stream_t stream) {
    const size_t  fb = h ? (h->elem == 4 ? h->N / 2 : h->N) * sizeof(float) : 0;
    const StftOut outs[5] = {{d_mag, fb, 4, "d_mag"}, {d_phase, fb, 4, "d_phase"}, {d_re, fb, 4, "d_re"}, {d_im, fb, 4, "d_im"}, {d_ranges, 8 * sizeof(float), 4, "d_ranges"}};
    FftOutputs    o{};
    o.mag = d_mag;
    o.re  = d_re;
    o.im  = d_im;
    return stft_run(h, "stft_process", d_in, n_in, o, d_phase, d_ranges, n_frames, outs, 5, stream);
}

int gr4hip_stft_spectrum(gr4hip_stft_t* h, const void* d_in, size_t n_in, float* d_spectrum, size_t* n_frames, gr4hip_stream_t stream) {
    const StftOut outs[1] = {{d_spectrum, h ? h->N * sizeof(float2) : 0, 8, "d_spectrum"}};
    FftOutputs    o{};
    o.spectrum = d_spectrum;
    return stft_run(h, "stft_spectrum", d_in, n_in, o, nullptr, nullptr, n_frames, outs, 1, stream);
}

int gr4hip_stft_mag2(gr4hip_stft_t* h, const void* d_in, size_t n_in, float* d_mag2, size_t* n_frames, gr4hip_stream_t stream) {
    const StftOut outs[1] = {{d_mag2, h ? h->N * sizeof(float) : 0, 4, "d_mag2"}};
    FftOutputs    o{};
    o.mag2 = d_mag2;
    return stft_run(h, "stft_mag2", d_in, n_in, o, nullptr, nullptr, n_frames, outs, 1, stream);
}

// Welch: gr4hip_stft_mag2 followed by gr4hip_specint_process, bit for bit -- the frames' |X|^2 in pieces through the integrator's scratch, then its fold
int gr4hip_stft_mag2_integrate(gr4hip_stft_t* h, gr4hip_specint_t* si, const void* d_in, size_t n_in, float* d_out, size_t* n_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "stft_mag2_integrate: null handle");
    std::fill(h->last_path, h->last_path + 4, 0LL);
    if (n_in > 0) {
        GR4_REQUIRE(d_in, "stft_mag2_integrate: null input");
        GR4_REQUIRE((uintptr_t)d_in % (uintptr_t)h->elem == 0, "stft_mag2_integrate: the input must be aligned to %d bytes", h->elem);
        GR4_REQUIRE(n_in <= kStftMaxSamples, "stft_mag2_integrate: %zu samples in one call", n_in);
    }
    const size_t k = stft_count(h, n_in);
    if (const int rc = specint_check(si, "stft_mag2_integrate", h->N, d_in, 0, (size_t)h->elem, k, d_out, n_out)) return rc;
    size_t done = 0;
    (void)gr4hip_specint_pending(si, k, &done);
    *n_out = 0;
    if (n_in == 0) return GR4HIP_OK;
    {
        const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + n_in * h->elem, o0 = (uintptr_t)d_out, o1 = o0 + done * h->N * sizeof(float);
        GR4_REQUIRE(done == 0 || a1 <= o0 || o1 <= a0, "stft_mag2_integrate: d_out overlaps d_in");
    }
    hipStream_t st = as_stream(stream);
    if (const int rc = h->hist.on(st)) return rc;
    if (k > 0) {
        struct Ctx { gr4hip_stft_t* h; const void* in; gr4hip_stream_t stream; } ctx{h, d_in, stream};
        const auto produce = [](void* c, size_t first, size_t n, float* d_mag2, hipStream_t) {
            auto*      x = static_cast<Ctx*>(c);
            FftOutputs o{};
            o.mag2 = d_mag2;
            return stft_emit(x->h, x->in, first, n, o, nullptr, nullptr, x->stream);
        };
        if (const int rc = specint_compose(si, k, d_out, st, produce, &ctx)) return rc;
    }
    if (const int rc = stft_commit(h, d_in, n_in, k, st)) return rc;
    *n_out = done;
    return GR4HIP_OK;
}

int gr4hip_stft_destroy(gr4hip_stft_t* h) {
    delete h;
    return GR4HIP_OK;
}

// test hook (exported, not declared in include/gr4hip.h): what the last call enqueued, see gr4hip_stft::last_path
int gr4hip_internal_stft_last_path(const gr4hip_stft_t* h, long long* rec /*[4]*/) {
    GR4_REQUIRE(h && rec, "stft_last_path: bad argument");
    std::copy(h->last_path, h->last_path + 4, rec);
    return GR4HIP_OK;
}

// test hook: the frame-count rule without a handle (host only, no device)
int gr4hip_internal_stft_count(size_t fft_size, size_t stride, long long off, size_t n_in, size_t* n_frames) {
    GR4_REQUIRE(n_frames && fft_size >= 2 && stride >= 1 && off >= -(long long)(fft_size - 1) && n_in <= kStftMaxSamples, "stft_count: bad argument");
    *n_frames = stft_rule(fft_size, stride, (long)off, n_in);
    return GR4HIP_OK;
}

} // extern "C"
