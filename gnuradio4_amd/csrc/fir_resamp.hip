// fir_resamp.hip -- rational resampler (polyphase FIR, rate L / M) for gfx950 (RATIONAL_RESAMPLER.md; BASELINE.json north_star: "decimating / interpolating FIR").
//
// The reference has no such block, only the rate machinery one would declare (Resampling<inputChunk, outputChunk>, annotated.hpp:121-128; chunk bookkeeping
// Block.hpp:1576-1636), so like fir_interp.hip the definition is the project's (include/gr4hip.h, tests/rational_resampler_oracle.py):
//     u[n] = x[n / L] if n % L == 0 else 0,   v[n] = L sum_k b[k] u[n - k],   y[j] = v[j M]
// Output j = c L + p (cycle c, slot p < L) needs only the products whose u is a sample: with o_p = floor(p M / L), phi_p = (p M) mod L, Kp = ceil(K / L)
//     y[c L + p] = sum_{q < Kp} w_p[q] x[c M + o_p - q],   w_p[q] = float(L) b[q L + phi_p]   (0 where q L + phi_p >= K)
// float32, q ascending from 0, one fmaf per term and component, all Kp terms in every slot: one fixed order per output, whatever the cut into calls.
// A call consumes whole cycles (n_in a multiple of M), so it always starts at slot 0 and only the last Kp - 1 inputs are carried (capacity max(32, bit_ceil(Kp))
// like fir_interp.hip), in a pair of buffers: a second small launch writes the next call's history into the half nobody reads.
//
// fir_resamp_kernel<S, TL, MW>: a workgroup owns kRsTile cycles and walks them in chunks of cc cycles whose input span (cc M + Kp - 1 samples, the carried history below
// position 0) is staged in LDS with coalesced loads.  The host builds the slot table {o_p} and the tap table [Kp][L] (q-major: lanes on consecutive slots read
// consecutive words).  The tap table sits in LDS next to the stage (TL) while the two together leave two workgroups per CU, and is read through the L2 otherwise.  A lane
// owns one slot p and kRsR cycles of it at a time: one tap read serves kRsR multiply-adds.  With L smaller than the workgroup the lanes are dealt over (cycle, slot)
// pairs, G cycles side by side (a power of two), a lane's slot fixed; with L larger a lane walks slots p, p + lanes, ...  The outputs of a cycle leave coalesced
// across the slots.  Two forms of the inner loop (at the kernel): the gather form for any M, register windows for M <= kRsMaxWin.  Bounds: HBM ((4 + 4 M / L) S bytes
// per output) at short branches, LDS reads at long ones ((1 + 1 / kRsR) reads per multiply-add step in the gather form, 2 / kRsR in the window form).
// A single cycle whose span does not fit in LDS (M + Kp - 1 samples past 80 KiB) takes fir_resamp_direct_kernel: one output per lane straight from the L2.
#include "common.hpp"
#include "history.hpp"

#include <algorithm>
#include <type_traits>

namespace gr4 {

constexpr int    kRsBS        = 256;       // lanes per workgroup at most
constexpr int    kRsTile      = 256;       // output cycles per workgroup
constexpr int    kRsR         = 4;         // cycles per lane and register batch
constexpr size_t kRsLdsMax    = 80 * 1024; // per workgroup: two per CU
constexpr size_t kRsStageGoal = 16 * 1024; // the input stage stops growing here: more workgroups per CU (measured: 32 KB, and several tiles per workgroup, were slower)
constexpr size_t kRsTapLdsMax = 40 * 1024;
constexpr int    kRsMaxWin    = 4;         // decimations up to this run the window form

template <int S> struct rs_vec { using type = float; };
template <> struct rs_vec<2> { using type = float2; };
__device__ __forceinline__ float  rs_fma(float w, float x, float a) { return fmaf(w, x, a); }
__device__ __forceinline__ float2 rs_fma(float w, float2 x, float2 a) { return make_float2(fmaf(w, x.x, a.x), fmaf(w, x.y, a.y)); }

// stream position pos < n_in of this call: below 0 the carried history (hist[h] = position -hcap + h)
template <typename T>
__device__ __forceinline__ T rs_sample(const T* __restrict__ x, const T* __restrict__ hist, int hcap, long pos) {
    if (pos >= 0) return x[pos];
    return pos >= -(long)hcap ? hist[hcap + pos] : T{};
}

// taps: [Kp][L] (q-major), already times L.  slot_o: [L].  tap_lds_floats: the table's room in LDS (a multiple of 4 floats).  G: cycles side by side in a workgroup
// (lanes g L + p, g < G; a power of two, so that G kRsR divides the tile).  MW = 0: the gather form, any M -- a lane's kRsR cycles are G apart and every
// multiply-add reads its sample from LDS.  MW = M (1 .. kRsMaxWin): the window form -- a lane's kRsR cycles are consecutive, so the sample of cycle r at step q is
// the sample of cycle r - 1 at step q - M: M register windows (one per q mod M) of kRsR samples slide by one per step, one sample read and one tap read per
// kRsR multiply-adds.  Both forms add in the same order (q ascending from 0), so they give the same bits.
template <int S, bool TL, int MW>
__global__ __launch_bounds__(kRsBS) void fir_resamp_kernel(const typename rs_vec<S>::type* __restrict__ x, const typename rs_vec<S>::type* __restrict__ hist, int hcap,
                                                           const float* __restrict__ taps, const int* __restrict__ slot_o, int L, int M, int Kp, int cc, int G, int tap_lds_floats,
                                                           typename rs_vec<S>::type* __restrict__ y, long n_cyc) {
    using T = typename rs_vec<S>::type;
    extern __shared__ __attribute__((aligned(16))) float rs_smem[];
    T*        xs = reinterpret_cast<T*>(rs_smem + (TL ? tap_lds_floats : 0)); // [cc M + H]: positions c0 M - H .. (c0 + cc) M - 1
    const int H = Kp - 1, NT = (int)blockDim.x, t = (int)threadIdx.x;
    if constexpr (TL) {
        for (int i = t; i < Kp * L; i += NT) rs_smem[i] = taps[i];
    }
    const float* tp     = TL ? rs_smem : taps;
    const int    g      = t / L;     // (L > lanes: 0, and the lane walks slots t, t + lanes, ...)
    const int    p0     = t - g * L;
    const bool   active = g < G;
    const long   cbeg = (long)blockIdx.x * kRsTile, cend = cbeg + kRsTile < n_cyc ? cbeg + kRsTile : n_cyc;
    for (long c0 = cbeg; c0 < cend; c0 += cc) {
        const int  ncyc = (int)(cend - c0 < (long)cc ? cend - c0 : (long)cc);
        const int  span = ncyc * M + H;
        const long base = c0 * M - H;
        __syncthreads(); // every lane is done with the chunk before
        for (int i = t; i < span; i += NT) xs[i] = rs_sample(x, hist, hcap, base + i);
        __syncthreads();
        if (!active) continue;
        for (int p = p0; p < L; p += NT) {
            const int o = slot_o[p] + H; // cycle c of the chunk, step q: xs[c M + o - q]
            if constexpr (MW == 0) {
                for (int cb = g; cb < ncyc; cb += G * kRsR) {
                    int xi[kRsR];
                    T   acc[kRsR];
#pragma unroll
                    for (int r = 0; r < kRsR; ++r) {
                        const int cyc = cb + r * G;
                        xi[r]         = (cyc < ncyc ? cyc : ncyc - 1) * M + o; // (a cycle past the chunk repeats the last one and is not stored)
                        acc[r]        = T{};
                    }
#pragma unroll 4
                    for (int q = 0; q < Kp; ++q) {
                        const float w = tp[q * L + p];
#pragma unroll
                        for (int r = 0; r < kRsR; ++r) acc[r] = rs_fma(w, xs[xi[r] - q], acc[r]);
                    }
#pragma unroll
                    for (int r = 0; r < kRsR; ++r) {
                        const int cyc = cb + r * G;
                        if (cyc < ncyc) y[(c0 + cyc) * L + p] = acc[r];
                    }
                }
            } else {
                for (int cb = g * kRsR; cb < ncyc; cb += G * kRsR) {
                    const int top = cb * MW + o; // xs[top + r M - q]: cycle cb + r at step q
                    T         win[MW][kRsR], acc[kRsR];
#pragma unroll
                    for (int d = 0; d < MW; ++d)
#pragma unroll
                        for (int r = 0; r < kRsR; ++r) {
                            const int i = top - d + r * MW; // (past the chunk, or in front of it for a step d >= Kp: never used)
                            win[d][r]   = xs[i < 0 ? 0 : (i < span ? i : span - 1)];
                        }
#pragma unroll
                    for (int r = 0; r < kRsR; ++r) acc[r] = T{};
                    for (int q0 = 0; q0 < Kp; q0 += MW) {
#pragma unroll
                        for (int d = 0; d < MW; ++d) {
                            const int q = q0 + d;
                            if (q < Kp) {
                                const float w = tp[q * L + p];
#pragma unroll
                                for (int r = 0; r < kRsR; ++r) acc[r] = rs_fma(w, win[d][r], acc[r]);
#pragma unroll
                                for (int r = kRsR - 1; r > 0; --r) win[d][r] = win[d][r - 1];
                                const int nx = top - q - MW; // what cycle cb needs at step q + M
                                win[d][0]    = xs[nx < 0 ? 0 : nx];
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < kRsR; ++r)
                        if (cb + r < ncyc) y[(c0 + cb + r) * L + p] = acc[r];
                }
            }
        }
    }
}

// one output per lane straight from global memory (the L2 holds the windows): cycles too long for LDS; a corner, not the hot path
template <int S>
__global__ void fir_resamp_direct_kernel(const typename rs_vec<S>::type* __restrict__ x, const typename rs_vec<S>::type* __restrict__ hist, int hcap, const float* __restrict__ taps,
                                         const int* __restrict__ slot_o, int L, int M, int Kp, typename rs_vec<S>::type* __restrict__ y, long n_out) {
    using T = typename rs_vec<S>::type;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < n_out; j += (long)gridDim.x * blockDim.x) {
        const long c   = j / L;
        const int  p   = (int)(j - c * L);
        const long top = c * M + slot_o[p];
        T          a   = T{};
        for (int q = 0; q < Kp; ++q) a = rs_fma(taps[q * L + p], rs_sample(x, hist, hcap, top - q), a);
        y[j] = a;
    }
}

} // namespace gr4

using namespace gr4;

constexpr size_t kRsMaxRate = 1024, kRsMaxTaps = 65536;
enum { kRsPathLdsTaps = 1u, kRsPathGlobalTaps = 2u, kRsPathDirect = 4u, kRsPathWindow = 8u };

struct gr4hip_resamp {
    int                dtype = GR4HIP_F32, S = 1;
    size_t             ntaps = 0, L = 1, M = 1, Kp = 0, hcap = 32;
    std::vector<float> taps;
    DeviceBuffer       d_taps, d_slots;
    CarriedHistory     hist; // hcap samples
    // launch shape of the main kernel, fixed by (L, M, Kp, S): rs_plan
    int      lanes = kRsBS, G = 1, cc = 0; // cc = 0: fir_resamp_direct_kernel
    bool     taps_lds = false;
    size_t   tap_lds_floats = 0, lds = 0;
    unsigned last_paths = 0;
    // the stream rule (common.hpp): create / reset / set_taps only note what the device state has to become; rs_state_on() enqueues it on the stream of the next call
    std::vector<float> t_host; // image of d_taps: [Kp][L]
    std::vector<int>   o_host; // image of d_slots: [L]
    bool               taps_dirty = false;
};

static int rs_check_taps(const char* who, const float* h_taps, size_t ntaps) {
    GR4_REQUIRE(h_taps, "%s: null taps", who);
    GR4_REQUIRE(ntaps >= 1, "%s: need at least one tap", who);
    if (ntaps > kRsMaxTaps) { set_error("%s: %zu taps (supported: 1 .. %zu)", who, ntaps, kRsMaxTaps); return GR4HIP_UNSUPPORTED; }
    for (size_t k = 0; k < ntaps; ++k) GR4_REQUIRE(std::isfinite(h_taps[k]), "%s: tap %zu is not finite", who, k);
    return GR4HIP_OK;
}

// chunk length, tap placement and LDS bytes of fir_resamp_kernel
static void rs_plan(gr4hip_resamp* f) {
    const size_t es = sizeof(float) * f->S, H = f->Kp - 1;
    const auto   fit = [&](size_t avail) { return avail >= (f->M + H) * es ? (avail - H * es) / (f->M * es) : (size_t)0; }; // whole cycles staged in `avail` bytes
    size_t G = 1; // cycles side by side: a power of two up to 64, so that G kRsR divides the tile
    while (2 * G * f->L <= (size_t)kRsBS && 2 * G * kRsR <= (size_t)kRsTile) G *= 2;
    f->G              = (int)G;
    f->lanes          = f->L >= (size_t)kRsBS ? kRsBS : (int)ceil_div(G * f->L, (size_t)64) * 64;
    f->tap_lds_floats = ceil_div(f->Kp * f->L, (size_t)4) * 4;
    const size_t tb   = f->tap_lds_floats * sizeof(float);
    f->taps_lds       = tb <= kRsTapLdsMax && fit(kRsLdsMax - tb) >= 1;
    const size_t avail = kRsLdsMax - (f->taps_lds ? tb : 0);
    size_t       cc    = fit(std::min(avail, kRsStageGoal));
    if (cc == 0) cc = fit(avail);
    cc = std::min<size_t>(cc, kRsTile);
    if (cc > G * kRsR) cc -= cc % (G * kRsR); // whole register batches
    f->cc  = (int)cc;
    f->lds = (f->taps_lds ? tb : 0) + (cc * f->M + H) * es;
}

static int rs_upload(gr4hip_resamp* f) {
    const size_t L = f->L, M = f->M, K = f->ntaps;
    f->Kp = ceil_div(K, L);
    f->o_host.resize(L);
    f->t_host.assign(f->Kp * L, 0.f);
    for (size_t p = 0; p < L; ++p) {
        f->o_host[p]     = (int)(p * M / L);
        const size_t phi = p * M % L;
        for (size_t q = 0; q * L + phi < K; ++q) f->t_host[q * L + p] = (float)L * f->taps[q * L + phi];
    }
    int rc = f->d_taps.ensure(f->t_host.size() * sizeof(float)); // (growing frees the old table: hipFree waits for the device)
    if (!rc) rc = f->d_slots.ensure(L * sizeof(int));
    if (rc) return rc;
    f->taps_dirty = true; // uploaded by rs_state_on, on the stream of the next call
    rs_plan(f);
    return GR4HIP_OK;
}
static int rs_state_on(gr4hip_resamp* f, hipStream_t st) {
    if (f->taps_dirty) {
        GR4_HIP_TRY(hipMemcpyAsync(f->d_taps.ptr, f->t_host.data(), f->t_host.size() * sizeof(float), hipMemcpyHostToDevice, st));
        GR4_HIP_TRY(hipMemcpyAsync(f->d_slots.ptr, f->o_host.data(), f->o_host.size() * sizeof(int), hipMemcpyHostToDevice, st));
        f->taps_dirty = false;
    }
    return f->hist.on(st);
}

template <int S>
static int rs_launch(gr4hip_resamp* f, const void* d_in, void* d_out, long n_in, hipStream_t st) {
    using T           = typename rs_vec<S>::type;
    const T*     x    = static_cast<const T*>(d_in);
    T*           y    = static_cast<T*>(d_out);
    const T*     hist = static_cast<const T*>(f->hist.current());
    const float* taps = static_cast<const float*>(f->d_taps.ptr);
    const int*   so   = static_cast<const int*>(f->d_slots.ptr);
    const long   n_cyc = n_in / (long)f->M;
    const int    L = (int)f->L, M = (int)f->M, Kp = (int)f->Kp;
    if (f->cc == 0) {
        const long     n_out = n_cyc * L;
        const unsigned grid  = (unsigned)std::min<long>(ceil_div(n_out, 256L), 1L << 16);
        hipLaunchKernelGGL(fir_resamp_direct_kernel<S>, dim3(grid), dim3(256), 0, st, x, hist, (int)f->hcap, taps, so, L, M, Kp, y, n_out);
        GR4_LAUNCH_CHECK();
        f->last_paths = kRsPathDirect;
    } else {
        const long grid = ceil_div(n_cyc, (long)kRsTile);
        if (grid > 0x7fffffffL) { set_error("resamp_process: %ld cycles in one call (at most %ld)", n_cyc, 0x7fffffffL * kRsTile); return GR4HIP_UNSUPPORTED; }
        const int MW  = M <= kRsMaxWin ? M : 0;
        auto      pick = [&](auto tl) {
            constexpr bool TL = decltype(tl)::value;
            switch (MW) {
            case 1: return fir_resamp_kernel<S, TL, 1>;
            case 2: return fir_resamp_kernel<S, TL, 2>;
            case 3: return fir_resamp_kernel<S, TL, 3>;
            case 4: return fir_resamp_kernel<S, TL, 4>;
            default: return fir_resamp_kernel<S, TL, 0>;
            }
        };
        auto kern = f->taps_lds ? pick(std::true_type{}) : pick(std::false_type{});
        if (f->lds > 48 * 1024) GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)f->lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)f->lanes), f->lds, st, x, hist, (int)f->hcap, taps, so, L, M, Kp, f->cc, f->G, (int)f->tap_lds_floats, y, n_cyc);
        GR4_LAUNCH_CHECK();
        f->last_paths = (f->taps_lds ? kRsPathLdsTaps : kRsPathGlobalTaps) | (MW ? kRsPathWindow : 0u);
    }
    return f->hist.advance(x, (size_t)n_in, f->hcap, (int)sizeof(T), st);
}

extern "C" {

size_t gr4hip_resamp_tile(void) { return kRsTile; }

int gr4hip_resamp_design(float* h_out, size_t cap, size_t* ntaps, size_t interp, size_t decim, size_t half_len, int window, double beta) {
#pragma clang fp contract(off) // the float64 formula value by value, as tests/rational_resampler_oracle.py evaluates it
    GR4_REQUIRE(interp >= 1 && decim >= 1 && half_len >= 1, "resamp_design: interp, decim and half_len must be >= 1");
    GR4_REQUIRE(h_out || ntaps, "resamp_design: nothing to return");
    if (interp > kRsMaxRate || decim > kRsMaxRate || half_len > kRsMaxTaps) { set_error("resamp_design: interp and decim up to %zu", kRsMaxRate); return GR4HIP_UNSUPPORTED; }
    const size_t R = std::max(interp, decim), K = 2 * half_len * R + 1;
    if (K > kRsMaxTaps) { set_error("resamp_design: %zu taps (supported: up to %zu)", K, kRsMaxTaps); return GR4HIP_UNSUPPORTED; }
    if (h_out) GR4_REQUIRE(cap >= K, "resamp_design: room for %zu floats, the filter has %zu", cap, K);
    if (ntaps) *ntaps = K;
    if (!h_out) return GR4HIP_OK;
    std::vector<double> w(K), h(K);
    if (const int rc = make_window64(window, w.data(), K, beta)) return rc;
    const double fc2 = 2.0 * (0.4 / (double)R), mid = (double)(K - 1) * 0.5;
    for (size_t k = 0; k < K; ++k) {
        const double a = M_PI * (fc2 * ((double)k - mid));
        h[k]           = (w[k] * fc2) * (a == 0.0 ? 1.0 : std::sin(a) / a);
    }
    double sum = 0.0;
    for (size_t k = 0; k < K; ++k) sum = sum + h[k];
    for (size_t k = 0; k < K; ++k) h_out[k] = (float)(h[k] / sum);
    return GR4HIP_OK;
}

int gr4hip_resamp_create(gr4hip_resamp_t** out, int dtype, const float* h_taps, size_t ntaps, size_t interp, size_t decim) {
    GR4_REQUIRE(out, "resamp: null output handle");
    GR4_REQUIRE(interp >= 1 && decim >= 1, "resamp: interp and decim must be >= 1");
    if (dtype != GR4HIP_F32 && dtype != GR4HIP_C32) { set_error("resamp: dtype must be F32 or C32 (got %d)", dtype); return GR4HIP_UNSUPPORTED; }
    if (interp > kRsMaxRate || decim > kRsMaxRate) { set_error("resamp: interp %zu, decim %zu (supported: 1 .. %zu)", interp, decim, kRsMaxRate); return GR4HIP_UNSUPPORTED; }
    if (const int rc = rs_check_taps("resamp", h_taps, ntaps)) return rc;
    if (const int rc = have_device("resamp")) return rc;
    auto* f = new (std::nothrow) gr4hip_resamp();
    GR4_REQUIRE(f, "out of host memory");
    f->dtype = dtype;
    f->S     = dtype == GR4HIP_C32 ? 2 : 1;
    f->L     = interp;
    f->M     = decim;
    f->ntaps = ntaps;
    f->taps.assign(h_taps, h_taps + ntaps);
    int rc  = rs_upload(f);
    f->hcap = std::max<size_t>(32, bit_ceil(f->Kp));
    if (!rc) rc = f->hist.resize(f->hcap * f->S * sizeof(float));
    if (rc) { delete f; return rc; }
    *out = f;
    return GR4HIP_OK;
}

int gr4hip_resamp_set_taps(gr4hip_resamp_t* f, const float* h_taps, size_t ntaps) {
    GR4_REQUIRE(f, "resamp_set_taps: null handle");
    if (const int rc = rs_check_taps("resamp_set_taps", h_taps, ntaps)) return rc;
    f->taps.assign(h_taps, h_taps + ntaps);
    f->ntaps = ntaps;
    if (const int rc = rs_upload(f)) return rc;
    if (f->Kp > f->hcap) { // like fir_filter::settingsChanged: the history is replaced (lost) only when it must grow
        f->hcap = bit_ceil(f->Kp);
        return f->hist.resize(f->hcap * f->S * sizeof(float));
    }
    return GR4HIP_OK;
}

int gr4hip_resamp_reset(gr4hip_resamp_t* f) {
    GR4_REQUIRE(f, "resamp_reset: null handle");
    f->hist.reset(); // rs_state_on zeroes the history on the stream of the next call
    return GR4HIP_OK;
}

int gr4hip_resamp_process(gr4hip_resamp_t* f, const void* d_in, size_t n_in, void* d_out, size_t* n_out_p, gr4hip_stream_t stream) {
    GR4_REQUIRE(f, "resamp_process: null handle");
    GR4_REQUIRE(n_in % f->M == 0, "resamp_process: n_in (%zu) must be a multiple of decim (%zu)", n_in, f->M);
    const size_t n_out = n_in / f->M * f->L;
    if (n_out_p) *n_out_p = n_out;
    f->last_paths = 0;
    if (n_in == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in && d_out, "resamp_process: null device pointer");
    const size_t es = sizeof(float) * f->S;
    GR4_REQUIRE((uintptr_t)d_in % es == 0 && (uintptr_t)d_out % es == 0, "resamp_process: buffers must be aligned to %zu bytes", es);
    {
        const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + n_in * es, b0 = (uintptr_t)d_out, b1 = b0 + n_out * es;
        GR4_REQUIRE(a1 <= b0 || b1 <= a0, "resamp_process: d_in and d_out overlap");
    }
    hipStream_t st = as_stream(stream);
    if (const int rc = rs_state_on(f, st)) return rc;
    return f->S == 1 ? rs_launch<1>(f, d_in, d_out, (long)n_in, st) : rs_launch<2>(f, d_in, d_out, (long)n_in, st);
}

int gr4hip_resamp_destroy(gr4hip_resamp_t* f) {
    delete f;
    return GR4HIP_OK;
}

// test hook (exported, not declared in include/gr4hip.h): 1 = tap table in LDS, 2 = tap table read from global memory, 4 = the direct kernel, 8 = the window form
// (beside 1 or 2); 0 = nothing launched
int gr4hip_internal_resamp_last_paths(gr4hip_resamp_t* f, unsigned* mask) {
    GR4_REQUIRE(f && mask, "resamp_last_paths: bad arguments");
    *mask = f->last_paths;
    return GR4HIP_OK;
}

} // extern "C"
