// svd_denoiser.hip -- gr::filter::SvdDenoiser<T> (blocks/filter/.../SvdDenoiser.hpp:14-91 over algorithm/filter/SvdFilter.hpp:143-236) for float, double,
// complex<float> and complex<double>: Hankel-SVD low-rank denoising of a stream (include/gr4hip.h "SVD denoiser", SVD_DENOISER.md).
//
// Every `hop` samples the last W samples form the L x K Hankel matrix H[i][j] = w[i + j]; the outputs of the hop are d[safe .. safe + hop) of the anti-diagonal
// average of H's rank-k approximation, k from computeEffectiveRank (SvdFilter.hpp:43-65).  Every window is an independent small dense problem:
//   one window = one wave = one workgroup, all arithmetic float64 whatever T, the window and the matrix in LDS.
//   The matrix worked on is A[r][c] = w[r + c] with m = max(L, K) rows and n = min(L, K) columns: H or its plain transpose (a Hankel matrix's transpose is the
//   Hankel matrix of the same window with L and K exchanged; for complex T the transpose's rank-k approximation is the transpose of H's, so its anti-diagonal
//   average is the same d and nothing needs conjugating).
//   One-sided (Hestenes) Jacobi on the n columns: the n / 2 disjoint pairs of a round-robin round rotate at the same time, 64 / pairs lanes per pair sharing the
//   three dot products through a butterfly; a pair is skipped when |a_i . a_j| <= eps64 m |a_i| |a_j|, or when one of its columns is numerically zero
//   (|a| <= eps64 m |A|_F, exact zeros included: no 0 / 0); a sweep without a rotation ends the loop, kSvMaxSweeps bounds it.  At the end a_j = sigma_j u_j, and
//   a numerically zero column counts as sigma = 0.
//   sigma is sorted by counting, the rank rule runs in RealT (float for float / complex<float>) without contraction, and
//   A_k = sum_{j < k} u_j (u_j^H A) needs no V: per kept j, g_j[c] = u_j^H w[c .. c + m) and d[p] += sum_r u_j[r] g_j[p - r] for the hop's p only.
//   A window with a non-finite sample skips the sweeps; it and a window that did not converge are counted and give quiet NaN for all hop outputs.
// A call is one launch of (windows + 1) workgroups: the last one hands out what the previous call's last window left pending, and writes the next call's history
// (the newest W - 1 samples) and, where the call starts no window, its pending outputs.  The state is double-buffered, so no workgroup reads what another writes.
#include "common.hpp"

#include <cmath>
#include <cstdint>
#include <limits>

namespace gr4 {

constexpr int kSvLanes     = 64;  // one wave
constexpr int kSvMaxSweeps = 30;  // (the reference: 30 max(m, n) iterations of its QR sweep)
constexpr int kSvMaxW      = 128; // real types: n = min(L, K) <= 64 columns, one per lane, 32 pairs of two lanes; 36 KB of LDS at 64 x 65
constexpr int kSvMaxWc     = 64;  // complex types: 19 KB of LDS at 32 x 33
constexpr size_t kSvStateBytes = 8192; // history (W - 1 samples) + pending (hop samples), 16 bytes each at most

struct SvCd {
    double x, y;
};

template <typename T> struct SvTraits;
template <> struct SvTraits<float>   { using real = float;  using wide = double; static constexpr bool cplx = false; };
template <> struct SvTraits<double>  { using real = double; using wide = double; static constexpr bool cplx = false; };
template <> struct SvTraits<float2>  { using real = float;  using wide = SvCd;   static constexpr bool cplx = true; };
template <> struct SvTraits<double2> { using real = double; using wide = SvCd;   static constexpr bool cplx = true; };

struct SvGeom {
    int W, L, K, hop, safe, m, n, ms, lanes_per_pair;
    size_t lds;
};

struct SvArgs {
    const void*         in;
    void*               out;
    long long           n_in;
    const void*         hist;     // the W - 1 samples in front of the call
    void*               hist_new;
    const void*         pend;     // the hop outputs of the last window so far
    void*               pend_new;
    unsigned long long* counters; // {windows not converged or not finite, sweeps}
    long long           first;    // index within the call of the first sample that starts a window
    long long           nwin;
    int                 phase, lead; // out[0 .. lead) = pend[phase .. phase + lead)
    SvGeom              g;
    unsigned long long  max_rank;
    double              rel, ab, ef; // RealT values
};

#ifdef __HIPCC__
__device__ __forceinline__ double sv_widen(float v) { return (double)v; }
__device__ __forceinline__ double sv_widen(double v) { return v; }
__device__ __forceinline__ SvCd   sv_widen(float2 v) { return SvCd{(double)v.x, (double)v.y}; }
__device__ __forceinline__ SvCd   sv_widen(double2 v) { return SvCd{v.x, v.y}; }
__device__ __forceinline__ bool   sv_finite(double v) { return isfinite(v); }
__device__ __forceinline__ bool   sv_finite(SvCd v) { return isfinite(v.x) && isfinite(v.y); }
__device__ __forceinline__ void   sv_narrow(float& o, double v) { o = (float)v; }
__device__ __forceinline__ void   sv_narrow(double& o, double v) { o = v; }
__device__ __forceinline__ void   sv_narrow(float2& o, SvCd v) { o = make_float2((float)v.x, (float)v.y); }
__device__ __forceinline__ void   sv_narrow(double2& o, SvCd v) { o = make_double2(v.x, v.y); }

__device__ __forceinline__ double sv_zero(double) { return 0.0; }
__device__ __forceinline__ SvCd   sv_zero(SvCd) { return SvCd{0.0, 0.0}; }
__device__ __forceinline__ double sv_norm2(double a) { return a * a; }
__device__ __forceinline__ double sv_norm2(SvCd a) { return a.x * a.x + a.y * a.y; }
// acc += conj(a) b
__device__ __forceinline__ void sv_cmac(double& acc, double a, double b) { acc += a * b; }
__device__ __forceinline__ void sv_cmac(SvCd& acc, SvCd a, SvCd b) {
    acc.x += a.x * b.x + a.y * b.y;
    acc.y += a.x * b.y - a.y * b.x;
}
// acc += a b
__device__ __forceinline__ void sv_mac(double& acc, double a, double b) { acc += a * b; }
__device__ __forceinline__ void sv_mac(SvCd& acc, SvCd a, SvCd b) {
    acc.x += a.x * b.x - a.y * b.y;
    acc.y += a.x * b.y + a.y * b.x;
}
__device__ __forceinline__ double sv_scale(double a, double s) { return a * s; }
__device__ __forceinline__ SvCd   sv_scale(SvCd a, double s) { return SvCd{a.x * s, a.y * s}; }
__device__ __forceinline__ double sv_add(double a, double b) { return a + b; }
__device__ __forceinline__ SvCd   sv_add(SvCd a, SvCd b) { return SvCd{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ double sv_abs(double a) { return fabs(a); }
__device__ __forceinline__ double sv_abs(SvCd a) { return hypot(a.x, a.y); }
__device__ __forceinline__ double sv_xor(double a, int o) { return __shfl_xor(a, o); }
__device__ __forceinline__ SvCd   sv_xor(SvCd a, int o) { return SvCd{__shfl_xor(a.x, o), __shfl_xor(a.y, o)}; }
__device__ __forceinline__ double sv_nan(double) { return __builtin_nan(""); }
__device__ __forceinline__ SvCd   sv_nan(SvCd) { return SvCd{__builtin_nan(""), __builtin_nan("")}; }
// a_i' = c a_i - s conj(ph) a_j,  a_j' = s ph a_i + c a_j  (ph = gamma / |gamma|: +-1 for the real types)
__device__ __forceinline__ void sv_rotate(double& x, double& y, double c, double s, double ph) {
    const double sp = s * ph, xn = c * x - sp * y;
    y = sp * x + c * y;
    x = xn;
}
__device__ __forceinline__ void sv_rotate(SvCd& x, SvCd& y, double c, double s, SvCd ph) {
    const double pr = s * ph.x, pi = s * ph.y; // s ph
    const SvCd   xn{c * x.x - (pr * y.x + pi * y.y), c * x.y - (pr * y.y - pi * y.x)};
    const SvCd   yn{(pr * x.x - pi * x.y) + c * y.x, (pr * x.y + pi * x.x) + c * y.y};
    x = xn;
    y = yn;
}

// computeEffectiveRank (SvdFilter.hpp:43-65) in R, every operation rounded on its own; the total in the order of libstdc++'s transform_reduce for random access
// iterators (four at a time, (s0^2 + s1^2) + (s2^2 + s3^2) added to the running total, the rest one by one).  sg: sigma in float64, ord: descending order.
template <typename R>
__device__ int sv_effective_rank(const double* sg, const int* ord, int n, unsigned long long max_rank, R rel, R ab, R ef) {
#pragma clang fp contract(off)
    R   tot = R(0);
    int i   = 0;
    for (; n - i >= 4; i += 4) {
        const R s0 = (R)sg[ord[i]], s1 = (R)sg[ord[i + 1]], s2 = (R)sg[ord[i + 2]], s3 = (R)sg[ord[i + 3]];
        const R v1 = s0 * s0 + s1 * s1, v2 = s2 * s2 + s3 * s3;
        tot        = tot + (v1 + v2);
    }
    for (; i < n; ++i) {
        const R s = (R)sg[ord[i]];
        tot       = tot + s * s;
    }
    const R cut  = ef * tot;
    const R s0   = (R)sg[ord[0]];
    R       cum  = R(0);
    int     rank = 0;
    bool    open = true; // (no data-dependent exit: the walk always takes n steps)
    for (i = 0; i < n; ++i) {
        const R s = (R)sg[ord[i]];
        if (open && ((unsigned long long)rank >= max_rank || s / s0 < rel || s < ab)) open = false;
        if (open) {
            cum = cum + s * s;
            ++rank;
            if (cum >= cut) open = false;
        }
    }
    return rank < 1 ? 1 : rank;
}

template <typename T>
__global__ __launch_bounds__(kSvLanes) void sv_kernel(const SvArgs a) {
    using E = typename SvTraits<T>::wide;
    using R = typename SvTraits<T>::real;
    extern __shared__ __align__(16) unsigned char sv_lds[];
    const SvGeom& g    = a.g;
    const int     lane = (int)threadIdx.x, W = g.W, m = g.m, n = g.n, ms = g.ms, hop = g.hop;
    const T*      in   = static_cast<const T*>(a.in);
    T*            out  = static_cast<T*>(a.out);
    const T*      hist = static_cast<const T*>(a.hist);
    const T*      pend = static_cast<const T*>(a.pend);
    T*            pend_new = static_cast<T*>(a.pend_new);
    const long long b = (long long)blockIdx.x;

    if (b == a.nwin) { // the hand-over workgroup
        for (int q = lane; q < a.lead; q += kSvLanes) out[q] = pend[a.phase + q];
        if (a.nwin == 0)
            for (int q = lane; q < hop; q += kSvLanes) pend_new[q] = pend[q];
        T* hist_new = static_cast<T*>(a.hist_new);
        for (int t = lane; t < W - 1; t += kSvLanes) {
            const long long idx = a.n_in - (W - 1) + t;
            hist_new[t]         = idx < 0 ? hist[(W - 1) + idx] : in[idx];
        }
        return;
    }

    E*      w   = reinterpret_cast<E*>(sv_lds);   // W
    E*      A   = w + W;                          // n columns of ms
    E*      gj  = A + (size_t)n * ms;             // n
    double* sg  = reinterpret_cast<double*>(gj + n); // n
    int*    ord = reinterpret_cast<int*>(sg + n); // n

    const long long s_h = a.first + b * hop; // the window's newest sample, within the call
    int             bad = 0;
    for (int t = lane; t < W; t += kSvLanes) {
        const long long idx = s_h - (W - 1) + t; // >= -(W - 1), <= s_h < n_in
        const E         v   = sv_widen(idx < 0 ? hist[(W - 1) + idx] : in[idx]);
        w[t]                = v;
        bad |= !sv_finite(v);
    }
    bad = __syncthreads_or(bad);
    for (int e = lane; e < m * n; e += kSvLanes) {
        const int c = e / m, r = e - c * m;
        A[c * ms + r] = w[r + c];
    }
    __syncthreads();

    // ---- one-sided Jacobi, round-robin pairs
    const int    ne = n + (n & 1), n1 = ne - 1, pairs = ne / 2, S = g.lanes_per_pair;
    const int    q = lane / S, sub = lane & (S - 1);
    const double tol    = 2.220446049250313e-16 * (double)m;
    // |A|_F^2 = sum_p count_p |w[p]|^2, the same in every lane.  A column whose norm has fallen to tol |A|_F or below is numerically zero -- its sigma is below the
    // rounding of the large ones -- and is left alone: the difference of two parallel columns is rounding noise that stays parallel to them, and rotating it
    // against its own source again and again only shrinks it by eps64 a sweep (a constant window would need more than kSvMaxSweeps to reach exact zero).
    double fro2 = 0.0;
    for (int t = lane; t < W; t += kSvLanes) {
        int cnt = t < W - 1 - t ? t : W - 1 - t;
        cnt     = (cnt < n - 1 ? cnt : n - 1) + 1;
        fro2 += (double)cnt * sv_norm2(w[t]);
    }
    for (int o = kSvLanes >> 1; o > 0; o >>= 1) fro2 += __shfl_xor(fro2, o);
    const double floor2 = tol * tol * fro2;
    bool         conv   = n <= 1;
    int          sweeps = 0;
    if (!bad) {
        for (int sw = 0; sw < kSvMaxSweeps && !conv; ++sw) {
            int rot = 0;
            for (int r = 0; r < n1; ++r) {
                int ci, cj;
                if (q == 0) {
                    ci = r;
                    cj = ne - 1;
                } else {
                    ci = (r + q) % n1;
                    cj = (r - q + n1) % n1;
                }
                const bool act = q < pairs && ci < n && cj < n;
                double     al = 0.0, be = 0.0;
                E          ga = sv_zero(E{});
                if (act) {
                    const E* pi = A + ci * ms;
                    const E* pj = A + cj * ms;
                    for (int row = sub; row < m; row += S) {
                        const E x = pi[row], y = pj[row];
                        al += sv_norm2(x);
                        be += sv_norm2(y);
                        sv_cmac(ga, x, y);
                    }
                }
                for (int o = S >> 1; o > 0; o >>= 1) { // the same sums in every lane of the pair
                    al += __shfl_xor(al, o);
                    be += __shfl_xor(be, o);
                    ga = sv_add(ga, sv_xor(ga, o));
                }
                const double gm = sv_abs(ga);
                if (act && al > floor2 && be > floor2 && gm > tol * (sqrt(al) * sqrt(be))) {
                    rot            = 1;
                    const double z = (be - al) / (2.0 * gm);
                    const double az = fabs(z);
                    double       t  = az > 1e150 ? 0.5 / az : 1.0 / (az + sqrt(1.0 + z * z));
                    t               = z < 0.0 ? -t : t;
                    const double c  = 1.0 / sqrt(1.0 + t * t), s = c * t;
                    const E      ph = sv_scale(ga, 1.0 / gm);
                    E*           pi = A + ci * ms;
                    E*           pj = A + cj * ms;
                    for (int row = sub; row < m; row += S) {
                        E x = pi[row], y = pj[row];
                        sv_rotate(x, y, c, s, ph);
                        pi[row] = x;
                        pj[row] = y;
                    }
                }
                __syncthreads(); // the next round pairs the columns anew
            }
            ++sweeps;
            conv = !__syncthreads_or(rot);
        }
    }
    const bool failed = bad || !conv;
    if (lane == 0) {
        if (failed) atomicAdd(&a.counters[0], 1ull);
        if (sweeps) atomicAdd(&a.counters[1], (unsigned long long)sweeps);
    }

    E acc[2] = {sv_zero(E{}), sv_zero(E{})};
    if (!failed) {
        // ---- sigma_j = |a_j|, descending order by counting
        for (int c = lane; c < n; c += kSvLanes) {
            double   s2 = 0.0;
            const E* pc = A + c * ms;
            for (int row = 0; row < m; ++row) s2 += sv_norm2(pc[row]);
            sg[c] = s2 > floor2 ? sqrt(s2) : 0.0; // (a numerically zero column takes no part in the sum below: its direction is noise)
        }
        __syncthreads();
        for (int c = lane; c < n; c += kSvLanes) {
            const double s    = sg[c];
            int          rank = 0;
            for (int o = 0; o < n; ++o) {
                const double so = sg[o];
                rank += (so > s || (so == s && o < c)) ? 1 : 0;
            }
            ord[rank] = c;
        }
        __syncthreads();
        int k = sv_effective_rank<R>(sg, ord, n, a.max_rank, (R)a.rel, (R)a.ab, (R)a.ef);
        k     = k < n ? k : n;
        // ---- d[p] for the hop's p: sum over the kept j of u_j (u_j^H A) along the anti-diagonal p
        for (int j = 0; j < k; ++j) {
            const int    col = ord[j];
            const double s   = sg[col];
            const double inv = s > 0.0 ? 1.0 / s : 0.0;
            const E*     pc  = A + col * ms;
            for (int c = lane; c < n; c += kSvLanes) {
                E t = sv_zero(E{});
                for (int row = 0; row < m; ++row) sv_cmac(t, pc[row], w[row + c]);
                gj[c] = sv_scale(t, inv);
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int qo = lane + h * kSvLanes;
                if (qo < hop) {
                    const int p  = g.safe + qo;
                    const int lo = p - (n - 1) > 0 ? p - (n - 1) : 0, hi = p < m - 1 ? p : m - 1;
                    E         t  = sv_zero(E{});
                    for (int row = lo; row <= hi; ++row) sv_mac(t, pc[row], gj[p - row]);
                    acc[h] = sv_add(acc[h], sv_scale(t, inv));
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int qo = lane + h * kSvLanes;
        if (qo < hop) {
            const int p   = g.safe + qo;
            int       cnt = p < W - 1 - p ? p : W - 1 - p; // pairs (r, c) on the anti-diagonal p
            cnt           = (cnt < n - 1 ? cnt : n - 1) + 1;
            const E v     = failed ? sv_nan(E{}) : sv_scale(acc[h], 1.0 / (double)cnt);
            T       o;
            sv_narrow(o, v);
            if (s_h + qo < a.n_in) out[s_h + qo] = o;
            if (b == a.nwin - 1) pend_new[qo] = o;
        }
    }
}
#endif

template <typename R>
static size_t sv_hop(size_t W, double hop_fraction) { // (:183) the product in RealT: 32 * 0.1f -> 3
    const size_t h = (size_t)((R)W * (R)hop_fraction);
    return h < 1 ? 1 : h;
}

static bool sv_is_f32(int dtype) { return dtype == GR4HIP_F32 || dtype == GR4HIP_C32; }
static bool sv_is_cplx(int dtype) { return dtype == GR4HIP_C32 || dtype == GR4HIP_C64; }

static int sv_check(const gr4hip_svddenoise_params* p, SvGeom* out) {
    GR4_REQUIRE(p, "svddenoise: null params");
    GR4_REQUIRE(p->dtype == GR4HIP_F32 || p->dtype == GR4HIP_F64 || p->dtype == GR4HIP_C32 || p->dtype == GR4HIP_C64,
                "svddenoise: dtype %d (float, double, complex<float>, complex<double>)", p->dtype);
    GR4_REQUIRE(std::isfinite(p->relative_threshold) && p->relative_threshold >= 0.0, "svddenoise: relative_threshold %g (finite, not negative)", p->relative_threshold);
    GR4_REQUIRE(std::isfinite(p->absolute_threshold) && p->absolute_threshold >= 0.0, "svddenoise: absolute_threshold %g (finite, not negative)", p->absolute_threshold);
    GR4_REQUIRE(std::isfinite(p->energy_fraction), "svddenoise: energy_fraction %g", p->energy_fraction);
    // hop > W makes the reference copy past its window (:178)
    GR4_REQUIRE(std::isfinite(p->hop_fraction) && p->hop_fraction >= 0.0 && p->hop_fraction <= 1.0, "svddenoise: hop_fraction %g (0 ... 1)", p->hop_fraction);
    const size_t W = p->window_size < 2 ? 2 : p->window_size; // (:183)
    GR4_REQUIRE(p->hankel_rows <= W, "svddenoise: hankel_rows %zu exceeds the window of %zu samples (the reference throws)", p->hankel_rows, W);
    const size_t maxW = sv_is_cplx(p->dtype) ? kSvMaxWc : kSvMaxW;
    if (W > maxW) {
        set_error("svddenoise: window_size %zu beyond the device kernel's %zu for this type (the matrix lives in LDS, one column per lane)", W, maxW);
        return GR4HIP_UNSUPPORTED;
    }
    const size_t L = p->hankel_rows == 0 ? W / 2 : p->hankel_rows, K = W - L + 1;
    const size_t hop = sv_is_f32(p->dtype) ? sv_hop<float>(W, p->hop_fraction) : sv_hop<double>(W, p->hop_fraction);
    GR4_REQUIRE(hop <= W, "svddenoise: hop %zu exceeds the window of %zu samples", hop, W);
    if (out) {
        const size_t delay = (W - 1) / 2, start = W - 1 - delay, rest = W > hop ? W - hop : 0; // (:174-176)
        SvGeom       g{};
        g.W    = (int)W;
        g.L    = (int)L;
        g.K    = (int)K;
        g.hop  = (int)hop;
        g.safe = (int)(start < rest ? start : rest);
        g.m    = (int)(L > K ? L : K);
        g.n    = (int)(L > K ? K : L);
        g.ms   = g.m | 1; // odd column stride: the pairs of a round read different banks
        int pairs = (g.n + 1) / 2, p2 = 1;
        while (p2 < pairs) p2 <<= 1;
        g.lanes_per_pair = kSvLanes / p2;
        const size_t e   = sv_is_cplx(p->dtype) ? sizeof(SvCd) : sizeof(double);
        g.lds            = (W + (size_t)g.n * g.ms + g.n) * e + (size_t)g.n * (sizeof(double) + sizeof(int));
        *out             = g;
    }
    return GR4HIP_OK;
}

} // namespace gr4

using namespace gr4;

struct gr4hip_svddenoise {
    gr4hip_svddenoise_params p{};
    SvGeom                   g{};
    bool                     init_pending = true; // the zero pre-fill to be written in front of the next launch, on its stream
    int                      cur          = 0;    // which state buffer holds the history and the pending outputs
    unsigned long long       count        = 0;    // samples since the last reset
    unsigned long long       windows      = 0;    // windows launched since create
    hipStream_t              last         = nullptr;
    DeviceBuffer             d_state[2], d_cnt;
    unsigned long long*      h_cnt = nullptr; // page-locked: where stats() receives the device counters
    ~gr4hip_svddenoise() {
        if (h_cnt) hip_quiet(hipHostFree(h_cnt));
    }
};

template <typename T>
static int sv_launch(const SvArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(sv_kernel<T>, dim3((unsigned)(a.nwin + 1)), dim3(kSvLanes), a.g.lds, st, a);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

extern "C" {

int gr4hip_svddenoise_params_default(gr4hip_svddenoise_params* p, int dtype) {
    GR4_REQUIRE(p, "svddenoise: null params");
    GR4_REQUIRE(dtype == GR4HIP_F32 || dtype == GR4HIP_F64 || dtype == GR4HIP_C32 || dtype == GR4HIP_C64, "svddenoise: dtype %d (float, double, complex<float>, complex<double>)", dtype);
    const double eps = sv_is_f32(dtype) ? (double)std::numeric_limits<float>::epsilon() : std::numeric_limits<double>::epsilon();
    *p = gr4hip_svddenoise_params{dtype, 64, 0, UINT64_MAX, eps, eps, 1.0, 0.25}; // (SvdDenoiser.hpp:37-51)
    return GR4HIP_OK;
}

int gr4hip_svddenoise_check(const gr4hip_svddenoise_params* p) { return sv_check(p, nullptr); }

size_t gr4hip_svddenoise_windows_per_group(void) { return 1; }

int gr4hip_svddenoise_create(gr4hip_svddenoise_t** out, const gr4hip_svddenoise_params* p) {
    GR4_REQUIRE(out, "svddenoise: null output handle");
    SvGeom g{};
    int    rc = sv_check(p, &g); // (validated before anything is allocated)
    if (rc) return rc;
    auto* h = new (std::nothrow) gr4hip_svddenoise();
    GR4_REQUIRE(h, "out of host memory");
    h->p = *p;
    h->g = g;
    for (auto& b : h->d_state)
        if (!rc) rc = b.ensure(kSvStateBytes);
    if (!rc) rc = h->d_cnt.ensure(2 * sizeof(unsigned long long));
    if (!rc && hipHostMalloc(reinterpret_cast<void**>(&h->h_cnt), 2 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        h->h_cnt = nullptr;
        set_error("svddenoise: no page-locked memory for the counters");
        rc = GR4HIP_RUNTIME_ERROR;
    }
    if (!rc) {
        const unsigned long long zero[2] = {0, 0};
        if (upload_fresh(h->d_cnt.ptr, zero, sizeof zero) != hipSuccess) {
            (void)hipGetLastError();
            set_error("svddenoise: clearing the counters failed");
            rc = GR4HIP_RUNTIME_ERROR;
        }
    }
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return GR4HIP_OK;
}

int gr4hip_svddenoise_set_params(gr4hip_svddenoise_t* h, const gr4hip_svddenoise_params* p) {
    GR4_REQUIRE(h, "svddenoise: null handle");
    SvGeom    g{};
    const int rc = sv_check(p, &g);
    if (rc) return rc;
    GR4_REQUIRE(p->dtype == h->p.dtype, "svddenoise: the sample type is fixed at create (%d, not %d)", h->p.dtype, p->dtype);
    h->p            = *p;
    h->g            = g;
    h->init_pending = true; // setParameters resets (SvdFilter.hpp:221-229)
    return GR4HIP_OK;
}

int gr4hip_svddenoise_reset(gr4hip_svddenoise_t* h) {
    GR4_REQUIRE(h, "svddenoise: null handle");
    h->init_pending = true;
    return GR4HIP_OK;
}

int gr4hip_svddenoise_destroy(gr4hip_svddenoise_t* h) {
    delete h;
    return GR4HIP_OK;
}

int gr4hip_svddenoise_process(gr4hip_svddenoise_t* h, const void* d_in, size_t n_in, void* d_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "svddenoise: null handle");
    if (n_in == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in && d_out, "svddenoise: null sample pointer");
    const size_t esz = dtype_size(h->p.dtype), asz = sv_is_cplx(h->p.dtype) ? esz / 2 : esz;
    GR4_REQUIRE(((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & (asz - 1)) == 0, "svddenoise: a sample pointer is not aligned to its type");
    {
        // a later window reads inputs that an earlier window's outputs would have overwritten
        const uintptr_t xi = reinterpret_cast<uintptr_t>(d_in), yi = reinterpret_cast<uintptr_t>(d_out), bytes = n_in * esz;
        GR4_REQUIRE(xi + bytes <= yi || yi + bytes <= xi, "svddenoise: the input and output ranges overlap (the block does not run in place)");
    }
    const SvGeom&      g     = h->g;
    const size_t       hop   = (size_t)g.hop;
    const size_t       phase = h->init_pending ? 0 : (size_t)(h->count % hop);
    const size_t       first = phase == 0 ? 0 : hop - phase;
    const size_t       nwin  = n_in > first ? ceil_div(n_in - first, hop) : 0;
    GR4_REQUIRE(nwin < 0x7fffffffull, "svddenoise: %zu windows in one call (a longer stream goes in several calls)", nwin);
    hipStream_t st = as_stream(stream);
    if (h->init_pending) { // reset() (:204-212): a history of zeros, nothing pending
        GR4_HIP_TRY(hipMemsetAsync(h->d_state[h->cur].ptr, 0, kSvStateBytes, st));
        h->init_pending = false;
        h->count        = 0;
    }
    const size_t pend_off = kSvStateBytes / 2; // the history takes (W - 1) * 16 bytes at most
    char*        s0       = static_cast<char*>(h->d_state[h->cur].ptr);
    char*        s1       = static_cast<char*>(h->d_state[h->cur ^ 1].ptr);
    SvArgs       a{};
    a.in       = d_in;
    a.out      = d_out;
    a.n_in     = (long long)n_in;
    a.hist     = s0;
    a.hist_new = s1;
    a.pend     = s0 + pend_off;
    a.pend_new = s1 + pend_off;
    a.counters = static_cast<unsigned long long*>(h->d_cnt.ptr);
    a.first    = (long long)first;
    a.nwin     = (long long)nwin;
    a.phase    = (int)phase;
    a.lead     = (int)(first < n_in ? first : n_in);
    a.g        = g;
    a.max_rank = h->p.max_rank;
    a.rel      = h->p.relative_threshold;
    a.ab       = h->p.absolute_threshold;
    a.ef       = h->p.energy_fraction;
    int rc;
    switch (h->p.dtype) {
    case GR4HIP_F32: rc = sv_launch<float>(a, st); break;
    case GR4HIP_F64: rc = sv_launch<double>(a, st); break;
    case GR4HIP_C32: rc = sv_launch<float2>(a, st); break;
    default: rc = sv_launch<double2>(a, st); break;
    }
    if (rc) return rc;
    h->cur ^= 1;
    h->count += n_in;
    h->windows += nwin;
    h->last = st;
    return GR4HIP_OK;
}

int gr4hip_svddenoise_stats(gr4hip_svddenoise_t* h, unsigned long long* windows, unsigned long long* not_converged) {
    GR4_REQUIRE(h, "svddenoise: null handle");
    GR4_HIP_TRY(hipMemcpyAsync(h->h_cnt, h->d_cnt.ptr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->last));
    GR4_HIP_TRY(hipStreamSynchronize(h->last));
    if (windows) *windows = h->windows;
    if (not_converged) *not_converged = h->h_cnt[0];
    return GR4HIP_OK;
}

int gr4hip_svddenoise_sweeps(gr4hip_svddenoise_t* h, unsigned long long* sweeps) {
    GR4_REQUIRE(h && sweeps, "svddenoise: null argument");
    GR4_HIP_TRY(hipMemcpyAsync(h->h_cnt, h->d_cnt.ptr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->last));
    GR4_HIP_TRY(hipStreamSynchronize(h->last));
    *sweeps = h->h_cnt[1];
    return GR4HIP_OK;
}

} // extern "C"
