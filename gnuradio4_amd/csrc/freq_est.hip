// freq_est.hip -- FrequencyEstimatorTimeDomain<float> / FrequencyEstimatorFrequencyDomain<float> (blocks/filter/.../FrequencyEstimator.hpp:30-351).
//
// One path per method, parameterised by the chunk C (include/gr4hip.h "frequency estimators").  A call is
//   [time domain] the Bessel biquad on the library's IIR path (gr4hip_iir_*) into the handle's scratch y,
//   fe_td_kernel / fe_fd_kernel: a raw estimate and a valid flag per output,
//   fe_fill_*: the forward fill of the last valid estimate (across tiles, and across calls through the handle's d_prev word),
//   [time domain] fe_first_bad_kernel / fe_poison_latch_kernel: a non-finite input poisons every later filtered sample until reset (the reference's DF-I state),
//   fe_hist_kernel: the last W - 1 samples (filtered for the time domain, raw for the frequency domain) into the other history buffer.
// Sample q of a call (q in [-(W-1), n_in)) is hist[W - 1 + q] for q < 0, else the call's own sample: the history holds zeros for samples never seen, and the host
// knows how many have been (seen): output m is a settling output while seen + (m + 1) C < W.
#include "common.hpp"

#include <algorithm>

namespace gr4 {

constexpr size_t kFeMaxWindow = size_t(1) << 20;
constexpr int    kFeMaxBins   = 2048; // bins i_min - 1 .. i_max of the frequency-domain search: 256 lanes x 8 bins
constexpr int    kFeFillTile  = 1024; // outputs per workgroup of the forward fill (256 lanes x 4)

__device__ __forceinline__ float fe_sample(const float* __restrict__ x, const float* __restrict__ hist, long w1, long q) {
    return q < 0 ? hist[w1 + q] : x[q];
}

// ------------------------------------------------------------------------------------------------ time domain
// A NaN / Inf input poisons the reference's DF-I state for good (NaN stays in _outputHistory's feedback); the library's parallel biquad recovers from it.  So the
// handle keeps bad[0] (poisoned since the last reset) and bad[1] (this call's first non-finite input): every filtered sample from there on reads as NaN.
__device__ __forceinline__ long long fe_poisoned_from(const unsigned long long* __restrict__ bad) {
    return bad[0] ? 0ll : bad[1] == ~0ull ? (long long)(~0ull >> 1) : (long long)bad[1];
}

__device__ __forceinline__ float fe_y(const float* __restrict__ y, const float* __restrict__ hist, long w1, long q, long long from) {
    return q >= from ? __builtin_nanf("") : fe_sample(y, hist, w1, q);
}

__global__ __launch_bounds__(256) void fe_first_bad_kernel(const float* __restrict__ x, long n, unsigned long long* __restrict__ bad) {
    unsigned long long first = ~0ull;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        if (!isfinite(x[i])) { first = (unsigned long long)i; break; }
    if (first != ~0ull) atomicMin(bad + 1, first);
}

__global__ void fe_poison_latch_kernel(unsigned long long* bad) {
    if (bad[1] != ~0ull) bad[0] = 1;
}

// One lane per run of K consecutive outputs.  Term q (the reference's data[n] with q = p - n, n = 1 .. W-2): b = y[q]^2, c = 2 a b = (y[q-1] + y[q+1])^2 / 2, skipped
// where |4 y[q]| < eps (evaluated in float like the reference: exact).  The first output of a run sums its W - 2 terms directly; the next ones slide (add the C entering
// terms, remove the C leaving ones) while that is cheaper, so no term that has left a window outlives its run.
__device__ __forceinline__ void fe_td_term(const float* __restrict__ y, const float* __restrict__ hist, long w1, long q, long long from, float eps, double& b, double& c) {
    const float ym = fe_y(y, hist, w1, q - 1, from), y0 = fe_y(y, hist, w1, q, from), yp = fe_y(y, hist, w1, q + 1, from);
    if (fabsf(4.f * y0) < eps) { b = 0.0; c = 0.0; return; }
    const double s = (double)ym + (double)yp;
    b = (double)y0 * (double)y0;
    c = 0.5 * s * s;
}

__global__ __launch_bounds__(256) void fe_td_kernel(const float* __restrict__ y, const float* __restrict__ hist, long W, long C, long n_out, long K, long first_valid,
                                                    double fs, float eps, const unsigned long long* __restrict__ bad, float* __restrict__ out,
                                                    unsigned char* __restrict__ flag) {
    const long run = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long j0  = run * K;
    if (j0 >= n_out) return;
    const long   j1    = min(j0 + K, n_out);
    const long   w1    = W - 1;
    const bool   slide = 2 * C < W - 2;
    const double    deps  = (double)eps;
    const long long from  = fe_poisoned_from(bad);
    double          B = 0.0, Cs = 0.0;
    for (long j = j0; j < j1; ++j) {
        const long p = (j + 1) * C - 1; // the window's newest sample; terms q = p - W + 2 .. p - 1
        if (j == j0 || !slide) {
            B = 0.0; Cs = 0.0;
            for (long q = p - W + 2; q <= p - 1; ++q) { double b, c; fe_td_term(y, hist, w1, q, from, eps, b, c); B += b; Cs += c; }
        } else {
            for (long q = p - C; q <= p - 1; ++q) { double b, c; fe_td_term(y, hist, w1, q, from, eps, b, c); B += b; Cs += c; }               // entering
            for (long q = p - C - W + 2; q < p - W + 2; ++q) { double b, c; fe_td_term(y, hist, w1, q, from, eps, b, c); B -= b; Cs -= c; }  // leaving
        }
        bool  ok = j >= first_valid;
        float f  = 0.f;
        if (ok) {
            if (B <= deps) ok = false; // (:153-155; NaN passes, as in the reference)
            else {
                const double z = Cs / B - 1.0;
                if (z >= 1.0 || z <= -1.0) ok = false; // (:158-161)
                else f = (float)(fs / (4.0 * 3.14159265358979323846) * acos(z));
            }
        }
        out[j]  = f;
        flag[j] = ok;
    }
}

// ------------------------------------------------------------------------------------------------ frequency domain
// One workgroup per tile of K consecutive outputs, MB bins per lane (bin lo + lane + 256 m).  Per output the lanes bring their three sums to the output's position
// (a direct sum over the window at the head of the tile or when C >= N, else C O(1) slides), store the magnitudes |X_k| 2 / N in LDS, and P outputs at a time
// are decided by one lane each: first maximum over [i_min, i_max) and the reference's fallbacks on k - 1, k, k + 1.
template <int MB>
__global__ __launch_bounds__(256) void fe_fd_kernel(const float* __restrict__ x, const float* __restrict__ hist, long N, long C, long n_out, long K, long first_valid,
                                                    int lo, int nb, int smin, int smax, int kempty, int P, double fs, float eps,
                                                    const double2* __restrict__ tw, const double2* __restrict__ twa, float* __restrict__ out, unsigned char* __restrict__ flag) {
    extern __shared__ double fe_lds[]; // [P][nb] magnitudes, then P non-finite counts
    double*   mag = fe_lds;
    int*      bad = reinterpret_cast<int*>(fe_lds + (size_t)P * nb);
    const long j0 = (long)blockIdx.x * K;
    if (j0 >= n_out) return;
    const long j1  = min(j0 + K, n_out);
    const long w1  = N - 1;
    const long msk = N - 1;
    const int  t   = threadIdx.x;
    // per bin k: theta = beta, beta + a, beta - a (beta = 2 pi k / N, eb = e^{-j beta}); the leaving sample's factor e^{-j theta (N-1)} is e^{j beta} for all three
    double2 eb[MB], S[MB][3];
    int     kk[MB];
    const double2 ea = twa[1]; // e^{-j a}
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        kk[m] = lo + t + 256 * m;
        eb[m] = tw[kk[m] & msk];
        for (int s = 0; s < 3; ++s) S[m][s] = make_double2(0.0, 0.0);
    }
    const bool slide = C < N;
    int        nbad  = 0;
    for (long jb = j0; jb < j1; jb += P) {
        const int cnt = (int)min((long)P, j1 - jb);
        for (int g = 0; g < cnt; ++g) {
            const long p = (jb + g + 1) * C - 1;
            if (!slide || jb + g == j0) { // direct: S_theta = sum_i x[p - i] e^{-j beta i} {1, e^{-j a i}, e^{+j a i}}
                nbad = 0;
#pragma unroll
                for (int m = 0; m < MB; ++m)
                    for (int s = 0; s < 3; ++s) S[m][s] = make_double2(0.0, 0.0);
                for (long i = 0; i < N; ++i) {
                    float xv = fe_sample(x, hist, w1, p - i);
                    if (!isfinite(xv)) { ++nbad; xv = 0.f; }
                    const double  xd = xv;
                    const double2 v  = twa[i];
#pragma unroll
                    for (int m = 0; m < MB; ++m) {
                        if (t + 256 * m >= nb) continue;
                        const double2 u = tw[((long)kk[m] * i) & msk];
                        const double  ur = xd * u.x, ui = xd * u.y;
                        S[m][0].x += ur;                    S[m][0].y += ui;
                        S[m][1].x += ur * v.x - ui * v.y;   S[m][1].y += ur * v.y + ui * v.x;
                        S[m][2].x += ur * v.x + ui * v.y;   S[m][2].y += ui * v.x - ur * v.y;
                    }
                }
            } else { // C slides: S <- x_new + e^{-j theta} (S - x_old e^{j beta})
                for (long q = p - C + 1; q <= p; ++q) {
                    float xn = fe_sample(x, hist, w1, q), xo = fe_sample(x, hist, w1, q - N);
                    if (!isfinite(xn)) { ++nbad; xn = 0.f; }
                    if (!isfinite(xo)) { --nbad; xo = 0.f; }
                    const double dn = xn, dq = xo;
#pragma unroll
                    for (int m = 0; m < MB; ++m) {
                        if (t + 256 * m >= nb) continue;
                        const double2 e = eb[m];
                        const double2 r[3] = {e, make_double2(e.x * ea.x - e.y * ea.y, e.x * ea.y + e.y * ea.x),  // e^{-j beta}, e^{-j (beta + a)},
                                              make_double2(e.x * ea.x + e.y * ea.y, e.y * ea.x - e.x * ea.y)}; // e^{-j (beta - a)}
                        const double orr = dq * e.x, oi = -dq * e.y;                                             // x_old e^{j beta}
#pragma unroll
                        for (int s = 0; s < 3; ++s) {
                            const double ar = S[m][s].x - orr, ai = S[m][s].y - oi;
                            S[m][s] = make_double2(dn + ar * r[s].x - ai * r[s].y, ar * r[s].y + ai * r[s].x);
                        }
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const int b = t + 256 * m;
                if (b >= nb) continue;
                const double xr = 0.5 * S[m][0].x - 0.25 * (S[m][1].x + S[m][2].x);
                const double xi = 0.5 * S[m][0].y - 0.25 * (S[m][1].y + S[m][2].y);
                mag[(size_t)g * nb + b] = sqrt(xr * xr + xi * xi) * 2.0 / (double)N;
            }
            if (t == 0) bad[g] = nbad;
        }
        __syncthreads();
        if (t < cnt) {
            const long    j  = jb + t;
            const double* mg = mag + (size_t)t * nb;
            bool          ok = j >= first_valid && bad[t] == 0;
            float         f  = 0.f;
            if (ok) {
                int k = kempty;
                if (smin < smax) { // (:308-311) first maximum of [i_min, i_max)
                    int    bs = smin;
                    double bv = mg[smin];
                    for (int s = smin + 1; s < smax; ++s)
                        if (mg[s] > bv) { bv = mg[s]; bs = s; }
                    k = lo + bs;
                }
                if (k == 0 || k >= N / 2 - 1) ok = false; // (:314-316)
                else {
                    const double sm = mg[k - 1 - lo], s0 = mg[k - lo], sp = mg[k + 1 - lo];
                    if (!(isfinite(sm) && isfinite(s0) && isfinite(sp)) || sm <= 0.0 || s0 <= 0.0 || sp <= 0.0) ok = false; // (:322-324)
                    else {
                        const double lm = log(sm), l0 = log(s0), lp = log(sp);
                        const double den = 2.0 * l0 - lm - lp;
                        if (!isfinite(den) || fabs(den) < (double)eps) ok = false; // (:332-334)
                        else {
                            const double d = 0.5 * (lp - lm) / den;
                            if (!isfinite(d) || fabs(d) >= 1.0) ok = false; // (:340-342)
                            else f = (float)(((double)k + d) * fs / (double)N);
                        }
                    }
                }
            }
            out[j]  = f;
            flag[j] = ok;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ forward fill
// (a) per tile of kFeFillTile outputs: the last valid index (-1: none); (b) one lane walks the tiles: the value each tile starts from, and the handle's new last
// estimate; (c) per tile: every invalid output takes the value of the last valid one before it (or the tile's start value).
__global__ __launch_bounds__(256) void fe_fill_last_kernel(const unsigned char* __restrict__ flag, long n_out, long long* __restrict__ tile_last) {
    __shared__ long long red[256];
    const long base = (long)blockIdx.x * kFeFillTile;
    long long  best = -1;
    for (int i = threadIdx.x; i < kFeFillTile; i += 256)
        if (base + i < n_out && flag[base + i]) best = max(best, (long long)(base + i));
    red[threadIdx.x] = best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_last[blockIdx.x] = red[0];
}

__global__ void fe_fill_scan_kernel(const long long* __restrict__ tile_last, long ntiles, const float* __restrict__ out, float* __restrict__ tile_start, float* __restrict__ prev) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float v = prev[0];
    for (long t = 0; t < ntiles; ++t) {
        tile_start[t] = v;
        if (tile_last[t] >= 0) v = out[tile_last[t]];
    }
    prev[0] = v;
}

__global__ __launch_bounds__(256) void fe_fill_apply_kernel(const unsigned char* __restrict__ flag, long n_out, const float* __restrict__ tile_start, float* __restrict__ out) {
    __shared__ long long sc[256];
    const long base = (long)blockIdx.x * kFeFillTile + (long)threadIdx.x * 4;
    long long  last = -1;
    for (int i = 0; i < 4; ++i)
        if (base + i < n_out && flag[base + i]) last = base + i;
    sc[threadIdx.x] = last;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) { // inclusive max-scan over the lanes
        const long long o = (int)threadIdx.x >= s ? sc[threadIdx.x - s] : -1;
        __syncthreads();
        sc[threadIdx.x] = max(sc[threadIdx.x], o);
        __syncthreads();
    }
    long long run = threadIdx.x ? sc[threadIdx.x - 1] : -1; // last valid output in front of this lane's four, within the tile
    const float start = tile_start[blockIdx.x];
    for (int i = 0; i < 4; ++i) {
        const long j = base + i;
        if (j >= n_out) break;
        if (flag[j]) run = j;
        else out[j] = run >= 0 ? out[run] : start; // (a valid output is never written here: reading one is race-free)
    }
}

__global__ void fe_hist_kernel(const float* __restrict__ x, const float* __restrict__ hist_old, long w1, long n_in, const unsigned long long* __restrict__ bad,
                               float* __restrict__ hist_new) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < w1) hist_new[t] = bad ? fe_y(x, hist_old, w1, n_in - w1 + t, fe_poisoned_from(bad)) : fe_sample(x, hist_old, w1, n_in - w1 + t);
}

__global__ void fe_store_kernel(float* p, float v) { p[0] = v; }

// ------------------------------------------------------------------------------------------------ host side
struct FeGeom {
    size_t W = 0, i_min = 0, i_max = 0;
};

static int fe_geometry(int method, const gr4hip_freqest_params* p, FeGeom& g) {
    GR4_REQUIRE(p, "freqest: null params");
    GR4_REQUIRE(method == GR4HIP_FREQEST_TIME_DOMAIN || method == GR4HIP_FREQEST_FREQUENCY_DOMAIN, "freqest: unknown method %d", method);
    const float fs = p->sample_rate, fmin = p->f_min, fexp = p->f_expected, fmax = p->f_max;
    GR4_REQUIRE(std::isfinite(fs) && std::isfinite(fmin) && std::isfinite(fexp) && std::isfinite(fmax) && std::isfinite(p->epsilon), "freqest: non-finite setting");
    GR4_REQUIRE(fs > 0.f, "freqest: sample_rate %g <= 0", (double)fs);
    // settingsChanged (:62-69, :222-229)
    GR4_REQUIRE(!(fmin < 0.f || fmax >= fs / 2.f || fexp < 0.f || fexp >= fs / 2.f),
                "Ill-formed block parameters: f_min: %g < f_expected: %g < f_max: %g < sample_rate/2: %g (Nyquist limit)", (double)fmin, (double)fexp, (double)fmax, (double)(fs / 2.f));
    GR4_REQUIRE(fexp > 0.f, "freqest: f_expected == 0 (the reference divides by it)");
    GR4_REQUIRE(p->chunk >= 1, "freqest: chunk == 0");
    if (fmax <= 0.f) { set_error("freqest: f_max <= 0 is not taken by the device path"); return GR4HIP_UNSUPPORTED; }
    const float per = fmin > 0.f ? fs / std::min(fmin, fexp) : fs / fexp; // float, as :72 / :232
    if (!(per < (float)kFeMaxWindow + 1.f)) { set_error("freqest: window beyond 2^20 samples"); return GR4HIP_UNSUPPORTED; }
    if (method == GR4HIP_FREQEST_TIME_DOMAIN) {
        GR4_REQUIRE(p->n_periods >= 1, "freqest: n_periods == 0");
        const uint64_t W = (uint64_t)p->n_periods * (uint64_t)(uint32_t)per; // n_periods * static_cast<Size_t>(...)
        if (p->n_periods > kFeMaxWindow || W > kFeMaxWindow) { set_error("freqest: window beyond 2^20 samples"); return GR4HIP_UNSUPPORTED; }
        g.W = (size_t)W; g.i_min = g.i_max = 0;
        return GR4HIP_OK;
    }
    const size_t m = std::max(p->min_fft_size, (size_t)per);
    if (m > kFeMaxWindow) { set_error("freqest: FFT size beyond 2^20"); return GR4HIP_UNSUPPORTED; }
    const size_t N = bit_ceil(m);
    if (N < 4) { set_error("freqest: FFT size %zu < 4", N); return GR4HIP_UNSUPPORTED; }
    const float  scaled = (float)(N / 2) * 2.f; // (:298-300)
    const size_t half = N / 2;
    size_t       a = (size_t)std::floor((fmin / fs) * scaled), b = (size_t)std::ceil((fmax / fs) * scaled);
    a = std::clamp<size_t>(a, 1, half - 1);
    b = std::clamp<size_t>(b, 1, half - 1);
    g.W = N; g.i_min = a; g.i_max = b;
    const size_t lo = a < b ? a - 1 : b - 1, hi = a < b ? b : b + 1;
    if (hi - lo + 1 > (size_t)kFeMaxBins) { set_error("freqest: search range of %zu bins (more than %d)", hi - lo + 1, kFeMaxBins - 2); return GR4HIP_UNSUPPORTED; }
    return GR4HIP_OK;
}

static int fe_design(const gr4hip_freqest_params& p, float b[3], float a[3]) {
    gr4hip_filter_params fp;
    gr4hip_filter_params_default(&fp);
    fp.order = 2;
    fp.f_low = (double)p.f_max;
    fp.fs    = (double)p.sample_rate;
    size_t ns = 0;
    float  bb[6] = {}, aa[6] = {};
    const int rc = gr4hip_iir_design(GR4HIP_LOWPASS, &fp, GR4HIP_BESSEL, bb, aa, 2, &ns);
    if (rc) return rc;
    if (ns != 1) { set_error("freqest: the order-2 Bessel design gave %zu sections", ns); return GR4HIP_ERROR; }
    std::copy(bb, bb + 3, b);
    std::copy(aa, aa + 3, a);
    return GR4HIP_OK;
}

} // namespace gr4

using namespace gr4;

struct gr4hip_freqest {
    int                   method = 0;
    gr4hip_freqest_params p{};
    FeGeom                g;
    size_t                seen = 0;              // samples since the histories were emptied (saturates at W): host-side, exact
    bool                  zero_pending = true;   // histories (and the biquad state) to be emptied in front of the next launch
    bool                  prev_pending = true;   // d_prev to be set to prev_value in front of the next launch
    float                 prev_value   = 50.f;
    int                   cur = 0;               // which history buffer holds the last W - 1 samples
    DeviceBuffer          d_hist[2], d_prev, d_y, d_flag, d_tile, d_tw, d_twa, d_bad; // d_bad: time domain, {poisoned, first non-finite input of the call}
    size_t                tw_n = 0;              // N the twiddle tables were built for
    std::vector<double>   tw_host;               // (kept for the lifetime of the upload)
    gr4hip_iir_t*         iir = nullptr;
    float                 b[3] = {}, a[3] = {};
    bool                  iir_stale = true;      // the biquad's design changed: a new IIR handle in front of the next launch
    ~gr4hip_freqest() { if (iir) gr4hip_iir_destroy(iir); }
};

static int fe_apply(gr4hip_freqest_t* h, const gr4hip_freqest_params* p, bool reset) {
    FeGeom g;
    int    rc = fe_geometry(h->method, p, g);
    if (rc) return rc;
    if (h->method == GR4HIP_FREQEST_TIME_DOMAIN) {
        float b[3], a[3];
        rc = fe_design(*p, b, a);
        if (rc) return rc;
        if (!std::equal(b, b + 3, h->b) || !std::equal(a, a + 3, h->a)) h->iir_stale = true;
        std::copy(b, b + 3, h->b);
        std::copy(a, a + 3, h->a);
        if (!h->iir_stale && h->iir) gr4hip_iir_reset(h->iir);
    }
    h->p = *p;
    h->g = g;
    h->seen = 0;
    h->zero_pending = true;
    if (reset) { h->prev_pending = true; h->prev_value = p->f_expected; }
    return GR4HIP_OK;
}

extern "C" {

int gr4hip_freqest_params_default(int method, gr4hip_freqest_params* p) {
    GR4_REQUIRE(p, "freqest: null params");
    GR4_REQUIRE(method == GR4HIP_FREQEST_TIME_DOMAIN || method == GR4HIP_FREQEST_FREQUENCY_DOMAIN, "freqest: unknown method %d", method);
    *p = gr4hip_freqest_params{1e3f, 40.f, 50.f, 60.f, 1e-8f, 4, 256, 1}; // (:46-51, :202-207)
    return GR4HIP_OK;
}

int gr4hip_freqest_geometry(int method, const gr4hip_freqest_params* p, size_t* window, size_t* i_min, size_t* i_max) {
    FeGeom g;
    const int rc = fe_geometry(method, p, g);
    if (rc) return rc;
    if (window) *window = g.W;
    if (i_min) *i_min = g.i_min;
    if (i_max) *i_max = g.i_max;
    return GR4HIP_OK;
}

int gr4hip_freqest_create(gr4hip_freqest_t** out, int method, const gr4hip_freqest_params* p) {
    GR4_REQUIRE(out, "freqest: null output handle");
    FeGeom g;
    int    rc = fe_geometry(method, p, g); // (validated before anything is allocated)
    if (rc) return rc;
    auto* h = new (std::nothrow) gr4hip_freqest();
    GR4_REQUIRE(h, "out of host memory");
    h->method = method;
    rc = fe_apply(h, p, true);
    if (!rc) rc = h->d_prev.ensure(sizeof(float));
    if (rc) { delete h; return rc; }
    *out = h;
    return GR4HIP_OK;
}

int gr4hip_freqest_set_params(gr4hip_freqest_t* h, const gr4hip_freqest_params* p) {
    GR4_REQUIRE(h, "freqest: null handle");
    return fe_apply(h, p, false);
}

int gr4hip_freqest_reset(gr4hip_freqest_t* h) {
    GR4_REQUIRE(h, "freqest: null handle");
    h->seen = 0;
    h->zero_pending = true;
    h->prev_pending = true;
    h->prev_value   = h->p.f_expected;
    if (h->iir) gr4hip_iir_reset(h->iir);
    return GR4HIP_OK;
}

int gr4hip_freqest_destroy(gr4hip_freqest_t* h) { delete h; return GR4HIP_OK; }

int gr4hip_freqest_process(gr4hip_freqest_t* h, const float* d_in, size_t n_in, float* d_out, size_t* n_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "freqest: null handle");
    const size_t C = h->p.chunk;
    GR4_REQUIRE(n_in % C == 0, "freqest: n_in %zu is not a multiple of the chunk %zu", n_in, C);
    const size_t no = n_in / C;
    if (n_out) *n_out = no;
    if (n_in == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in && (d_out || no == 0), "freqest: null device pointer");
    hipStream_t  st = as_stream(stream);
    const bool   td = h->method == GR4HIP_FREQEST_TIME_DOMAIN;
    const size_t W = h->g.W, w1 = W - 1;
    int          rc;
    // device state: buffers sized for this geometry (a replaced buffer is fresh: hipFree waited for the device), then the pending notes, on this stream
    for (auto& hb : h->d_hist)
        if ((rc = hb.ensure(std::max<size_t>(w1, 1) * sizeof(float)))) return rc;
    if (td && (rc = h->d_bad.ensure(2 * sizeof(unsigned long long)))) return rc;
    if (h->zero_pending) {
        GR4_HIP_TRY(hipMemsetAsync(h->d_hist[h->cur].ptr, 0, std::max<size_t>(w1, 1) * sizeof(float), st));
        if (td) GR4_HIP_TRY(hipMemsetAsync(h->d_bad.ptr, 0, sizeof(unsigned long long), st));
        h->zero_pending = false;
    }
    unsigned long long* bad = td ? (unsigned long long*)h->d_bad.ptr : nullptr;
    if (h->prev_pending) {
        hipLaunchKernelGGL(fe_store_kernel, dim3(1), dim3(1), 0, st, (float*)h->d_prev.ptr, h->prev_value);
        GR4_LAUNCH_CHECK();
        h->prev_pending = false;
    }
    const float* hist = (const float*)h->d_hist[h->cur].ptr;
    const float* src  = d_in; // the samples the history is made of
    if ((rc = h->d_flag.ensure(std::max<size_t>(no, 1)))) return rc;
    const size_t ntiles = ceil_div(std::max<size_t>(no, 1), (size_t)kFeFillTile);
    if ((rc = h->d_tile.ensure(ntiles * (sizeof(long long) + sizeof(float))))) return rc;
    const long first_valid = h->seen >= W ? 0 : (long)ceil_div(W - h->seen, C) - 1;
    unsigned char* flag = (unsigned char*)h->d_flag.ptr;
    if (td) {
        if (h->iir_stale || !h->iir) {
            if (h->iir) { gr4hip_iir_destroy(h->iir); h->iir = nullptr; }
            if ((rc = gr4hip_iir_create(&h->iir, GR4HIP_DF_I, 1, h->b, 3, h->a, 3))) return rc;
            h->iir_stale = false;
        }
        if ((rc = h->d_y.ensure(n_in * sizeof(float)))) return rc;
        float* y = (float*)h->d_y.ptr;
        GR4_HIP_TRY(hipMemsetAsync(bad + 1, 0xff, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(fe_first_bad_kernel, dim3((unsigned)std::min<size_t>(ceil_div(n_in, (size_t)256), 1024)), dim3(256), 0, st, d_in, (long)n_in, bad);
        GR4_LAUNCH_CHECK();
        if ((rc = gr4hip_iir_process(h->iir, d_in, n_in, y, stream))) return rc;
        src = y;
        if (no) {
            const long   K    = (long)std::clamp<size_t>(W / C, 1, 256);
            const long   runs = (long)ceil_div(no, (size_t)K);
            hipLaunchKernelGGL(fe_td_kernel, dim3((unsigned)ceil_div(runs, 256L)), dim3(256), 0, st, (const float*)y, hist, (long)W, (long)C, (long)no, K, first_valid,
                               (double)h->p.sample_rate, h->p.epsilon, (const unsigned long long*)bad, d_out, flag);
            GR4_LAUNCH_CHECK();
        }
    } else if (no) {
        const size_t N = W;
        if (h->tw_n != N) { // e^{-j 2 pi m / N} and e^{-j a i}, a = 2 pi / (N - 1), in float64
            h->d_tw.release();
            h->d_twa.release();
            if ((rc = h->d_tw.ensure(N * sizeof(double2))) || (rc = h->d_twa.ensure(N * sizeof(double2)))) return rc;
            h->tw_host.resize(4 * N);
            const double two_pi = 6.283185307179586476925286766559;
            for (size_t m = 0; m < N; ++m) {
                h->tw_host[2 * m]             = std::cos(two_pi * (double)m / (double)N);
                h->tw_host[2 * m + 1]         = -std::sin(two_pi * (double)m / (double)N);
                h->tw_host[2 * N + 2 * m]     = std::cos(two_pi * (double)m / (double)(N - 1));
                h->tw_host[2 * N + 2 * m + 1] = -std::sin(two_pi * (double)m / (double)(N - 1));
            }
            GR4_HIP_TRY(upload_fresh(h->d_tw.ptr, h->tw_host.data(), N * sizeof(double2)));
            GR4_HIP_TRY(upload_fresh(h->d_twa.ptr, h->tw_host.data() + 2 * N, N * sizeof(double2)));
            h->tw_n = N;
        }
        const size_t a = h->g.i_min, b = h->g.i_max;
        const bool   empty = a >= b;
        const int    lo = (int)(empty ? b - 1 : a - 1), hi = (int)(empty ? b + 1 : b);
        const int    nb = hi - lo + 1;
        const int    MB = nb <= 256 ? 1 : nb <= 512 ? 2 : nb <= 1024 ? 4 : 8;
        const int    P  = std::max(1, std::min(32, 4096 / nb));
        // tile: a direct sum (N steps) per tile amortised over about N slides, at least ~1024 workgroups where the call is long enough
        long K = C >= N ? 1 : (long)ceil_div(N, C);
        K = std::max(1L, std::min(K, (long)ceil_div(no, (size_t)1024)));
        const long   tiles = (long)ceil_div(no, (size_t)K);
        const size_t lds   = (size_t)P * nb * sizeof(double) + (size_t)P * sizeof(int);
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), lds, st, d_in, hist, (long)N, (long)C, (long)no, K, first_valid, lo, nb, (int)a - lo, (int)b - lo,
                               (int)b, P, (double)h->p.sample_rate, h->p.epsilon, (const double2*)h->d_tw.ptr, (const double2*)h->d_twa.ptr, d_out, flag);
        };
        if (MB == 1) launch(fe_fd_kernel<1>);
        else if (MB == 2) launch(fe_fd_kernel<2>);
        else if (MB == 4) launch(fe_fd_kernel<4>);
        else launch(fe_fd_kernel<8>);
        GR4_LAUNCH_CHECK();
    }
    if (no) {
        long long* tile_last  = (long long*)h->d_tile.ptr;
        float*     tile_start = (float*)(tile_last + ntiles);
        hipLaunchKernelGGL(fe_fill_last_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, (const unsigned char*)flag, (long)no, tile_last);
        GR4_LAUNCH_CHECK();
        hipLaunchKernelGGL(fe_fill_scan_kernel, dim3(1), dim3(64), 0, st, (const long long*)tile_last, (long)ntiles, (const float*)d_out, tile_start, (float*)h->d_prev.ptr);
        GR4_LAUNCH_CHECK();
        hipLaunchKernelGGL(fe_fill_apply_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, (const unsigned char*)flag, (long)no, (const float*)tile_start, d_out);
        GR4_LAUNCH_CHECK();
    }
    if (w1) {
        const int nxt = h->cur ^ 1;
        hipLaunchKernelGGL(fe_hist_kernel, dim3((unsigned)ceil_div(w1, (size_t)256)), dim3(256), 0, st, src, hist, (long)w1, (long)n_in, (const unsigned long long*)bad,
                           (float*)h->d_hist[nxt].ptr);
        GR4_LAUNCH_CHECK();
        h->cur = nxt;
    }
    if (td) { // (behind every reader of this call's bad[1])
        hipLaunchKernelGGL(fe_poison_latch_kernel, dim3(1), dim3(1), 0, st, bad);
        GR4_LAUNCH_CHECK();
    }
    h->seen = std::min(W, h->seen + n_in);
    return GR4HIP_OK;
}

} // extern "C"
