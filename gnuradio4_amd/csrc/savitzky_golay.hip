// savitzky_golay.hip -- gr::filter::SavitzkyGolayFilter / SavitzkyGolayDataSetFilter (blocks/filter/.../SavitzkyGolayFilter.hpp:17-164, over
// algorithm/filter/SavitzkyGolay.hpp): the coefficient design (host code, no device) and the zero-phase filter of the DataSet block as ONE launch.  The streaming
// block needs no kernel of its own: it is the design plus gr4hip_fir_* / gr4hip_fir64_* (include/gr4hip.h "Savitzky-Golay").  Design notes: SAVITZKY_GOLAY.md.
//
// Design.  computeCoefficients<T> (SavitzkyGolay.hpp:93-151) takes the SVD of the Vandermonde matrix IN T and drops singular values below eps_T max(W, p + 1) sigma_0,
// which for float happens at ordinary settings (W 51, p 4).  Here the SVD is a one-sided Jacobi in float64 and only the RULE is T's: the kept rank is then the one an
// exact SVD would give, and row d of the truncated pseudo-inverse is rounded to T once.
//
// Zero-phase kernel.  applyZeroPhase (:177-193) is apply / reverse / apply / reverse; with coefficients c[0 .. W), D = (W - 1) / 2 and the boundary map b that is
//     t[j]   = sum_k c[k] x[b(j + k - D)]      j in [0, N)     rounded to T (the reference's std::vector<T> temp)
//     out[n] = sum_k c[k] t[b(n - k + D)]      n in [0, N)     (b acts on t: mirrored t is not the filter of mirrored x for even W or derivative coefficients)
// A workgroup owns kZpTile consecutive outputs of one row.  It stages x[tile -+ 2 (W - 1)] clipped to the row in LDS, computes t[tile -+ (W - 1)] clipped to the
// row into LDS, then the outputs, which go through LDS once more so that the global stores are as coalesced as the loads.  t never reaches HBM.  Every index b maps
// lands inside the staged ranges: a row longer than one tile is longer than W, so b wraps once and by less than W; a row of one tile is staged whole, and
// reflectIndex may wrap as often as it likes (N < W).
// A lane produces kZpRun consecutive values from a ring of kZpRun registers: one LDS read per kZpRun float64 FMAs.  The lane stride of kZpRun elements would fold
// 32 lanes onto 4 banks, so element i of an LDS array sits at i + (i >> 5): lanes 8 l + s then cover all 32 banks (4-byte elements, ds_read_b32) or all 32 bank
// pairs (8-byte elements, ds_read_b64) of a lane group, and so do the 16-byte staging accesses (lane stride 4 or 2 elements).
// Sums are float64 for both types (float x float products are exact there).  The coefficients ride in the kernel arguments (W <= 255: 2040 bytes, read with
// scalar loads), so the handle owns no device memory and set_params is a host-side note like every other mutator of this library.
#include "common.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <limits>

namespace gr4 {
namespace sg {

// ---------------------------------------------------------------------------------------------------------------- design (host)
struct Clamped {
    size_t W, p, d;
    long   D;
};
static Clamped clamp_settings(size_t window_size, size_t poly_order, size_t deriv_order, int alignment) { // (:95-97, :105)
    Clamped c;
    c.W = std::max<size_t>(window_size, 1);
    c.p = std::min(poly_order, c.W - 1);
    c.d = std::min(deriv_order, c.p);
    c.D = alignment == GR4HIP_SAVGOL_CAUSAL ? (long)(c.W - 1) : (long)((c.W - 1) / 2);
    return c;
}

constexpr size_t kDesignMaxEntries = size_t(1) << 22; // W (p + 1): the Jacobi works on the whole matrix on the host

// One-sided (Hestenes) Jacobi on the columns of a (W x m, column-major) with V (m x m) accumulated: on return the columns are U_k sigma_k.  Rotations stop when every
// pair is orthogonal to eps64; a pair with a numerically zero column is left alone.
static int jacobi_svd(std::vector<double>& a, std::vector<double>& v, size_t W, size_t m) {
    v.assign(m * m, 0.0);
    for (size_t j = 0; j < m; ++j) v[j * m + j] = 1.0;
    const double eps = DBL_EPSILON;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (size_t p = 0; p + 1 < m; ++p)
            for (size_t q = p + 1; q < m; ++q) {
                double *ap = &a[p * W], *aq = &a[q * W];
                double  alpha = 0, beta = 0, gamma = 0;
                for (size_t i = 0; i < W; ++i) {
                    alpha += ap[i] * ap[i];
                    beta += aq[i] * aq[i];
                    gamma += ap[i] * aq[i];
                }
                if (alpha == 0.0 || beta == 0.0 || std::fabs(gamma) <= eps * std::sqrt(alpha) * std::sqrt(beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t    = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (size_t i = 0; i < W; ++i) {
                    const double x = ap[i], y = aq[i];
                    ap[i] = cs * x - sn * y;
                    aq[i] = sn * x + cs * y;
                }
                double *vp = &v[p * m], *vq = &v[q * m];
                for (size_t i = 0; i < m; ++i) {
                    const double x = vp[i], y = vq[i];
                    vp[i] = cs * x - sn * y;
                    vq[i] = sn * x + cs * y;
                }
            }
        if (!rotated) return GR4HIP_OK;
    }
    set_error("savgol_design: the Jacobi SVD did not converge in 60 sweeps");
    return GR4HIP_ERROR;
}

// row d of the truncated pseudo-inverse in float64, before the rounding to T and the scale
static int pinv_row(int dtype, const Clamped& c, std::vector<double>& row, gr4hip_savgol_info* info) {
    const size_t W = c.W, m = c.p + 1;
    if (W > kDesignMaxEntries / m) {
        set_error("savgol_design: window_size %zu x (poly_order + 1) %zu is beyond %zu matrix entries", W, m, kDesignMaxEntries);
        return GR4HIP_UNSUPPORTED;
    }
    std::vector<double> a(W * m), v;
    for (size_t i = 0; i < W; ++i) { // (:108-115) the running product
        const double t     = (double)((long)i - c.D);
        double       power = 1.0;
        for (size_t j = 0; j < m; ++j) {
            a[j * W + i] = power;
            power *= t;
        }
    }
    for (double e : a)
        if (!std::isfinite(e)) {
            set_error("savgol_design: (window_size %zu)^(poly_order %zu) is not finite", W, c.p);
            return GR4HIP_UNSUPPORTED;
        }
    if (int rc = jacobi_svd(a, v, W, m)) return rc;
    std::vector<double> sigma(m);
    std::vector<size_t> order(m);
    for (size_t k = 0; k < m; ++k) {
        double s = 0;
        for (size_t i = 0; i < W; ++i) s += a[k * W + i] * a[k * W + i];
        sigma[k] = std::sqrt(s);
        order[k] = k;
    }
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return sigma[x] > sigma[y]; });
    const double eps_t     = dtype == GR4HIP_F32 ? (double)FLT_EPSILON : DBL_EPSILON;
    const double sigma0    = sigma[order[0]];
    const double tolerance = eps_t * (double)std::max(W, m) * sigma0; // (:128)
    row.assign(W, 0.0);
    size_t rank = 0;
    double smin = sigma0;
    bool   ambiguous = false;
    for (size_t kk = 0; kk < m; ++kk) { // (:130-140) in the reference's order, the largest first
        const size_t k = order[kk];
        if (std::fabs(sigma[k] - tolerance) <= 16.0 * eps_t * sigma0) ambiguous = true;
        if (sigma[k] < tolerance) continue;
        ++rank;
        smin = sigma[k];
        const double f = v[k * m + c.d] / (sigma[k] * sigma[k]); // V[d, k] / sigma_k * U[j, k], with the column holding U sigma
        for (size_t j = 0; j < W; ++j) row[j] += f * a[k * W + j];
    }
    if (info) {
        info->window_size     = W;
        info->poly_order      = c.p;
        info->deriv_order     = c.d;
        info->rank            = rank;
        info->sigma_max       = sigma0;
        info->sigma_min_kept  = smin;
        info->threshold       = tolerance;
        info->ambiguous       = ambiguous ? 1 : 0;
    }
    return GR4HIP_OK;
}

template <typename T>
static void round_and_scale(const std::vector<double>& row, size_t d, double delta_in, T* out) { // (:98, :142-148)
    const T delta = std::max((T)delta_in, std::numeric_limits<T>::epsilon());
    size_t  fact  = 1; // detail::factorial (:43-49), size_t arithmetic
    for (size_t i = 2; i <= d; ++i) fact *= i;
    const T scale = static_cast<T>(fact) / std::pow(delta, static_cast<T>(d));
    for (size_t j = 0; j < row.size(); ++j) {
        T cj = (T)row[j];
        cj *= scale;
        out[j] = cj;
    }
}

static int design(int dtype, size_t window_size, size_t poly_order, size_t deriv_order, double delta, int alignment, void* h_coeffs_out, gr4hip_savgol_info* info_out) {
    GR4_REQUIRE(dtype == GR4HIP_F32 || dtype == GR4HIP_F64, "savgol_design: dtype %d (GR4HIP_F32 or GR4HIP_F64)", dtype);
    GR4_REQUIRE(alignment == GR4HIP_SAVGOL_CENTRED || alignment == GR4HIP_SAVGOL_CAUSAL, "savgol_design: alignment %d", alignment);
    GR4_REQUIRE(h_coeffs_out != nullptr, "savgol_design: h_coeffs_out is NULL");
    const Clamped       c = clamp_settings(window_size, poly_order, deriv_order, alignment);
    std::vector<double> row;
    if (int rc = pinv_row(dtype, c, row, info_out)) return rc;
    if (dtype == GR4HIP_F32) round_and_scale<float>(row, c.d, delta, static_cast<float*>(h_coeffs_out));
    else round_and_scale<double>(row, c.d, delta, static_cast<double*>(h_coeffs_out));
    return GR4HIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- zero-phase kernel
constexpr int kZpLanes = 256;
constexpr int kZpRun   = 8;                 // consecutive values per lane
constexpr int kZpTile  = kZpLanes * kZpRun; // outputs per workgroup (gr4hip_savgol_zp_tile)
constexpr int kZpMaxW  = GR4HIP_SAVGOL_ZP_MAX_WINDOW;
constexpr int kZpXCap  = kZpTile + 4 * (kZpMaxW - 1) + kZpRun; // logical elements: the x range and the reads of a run whose values nobody keeps
constexpr int kZpTCap  = kZpTile + 2 * (kZpMaxW - 1) + kZpRun;

__host__ __device__ constexpr int zp_phys(int i) { return i + (i >> 5); }

template <typename T>
struct ZpArgs {
    const T* in;
    T*       out;
    long     n, stride, tiles;
    int      W, D, replicate;
    double   c[kZpMaxW + 1];
};

// detail::reflectIndex / replicateIndex (:51-77)
__device__ __forceinline__ long zp_map(long i, long N, bool replicate) {
    if (replicate) return i < 0 ? 0 : (i >= N ? N - 1 : i);
    if (i < 0) i = -i - 1;
    const long period = 2 * N;
    if (i >= period) i %= period;
    if (i >= N) i = period - i - 1;
    return i;
}

// [g0, g0 + count) of a row <-> logical LDS elements [0, count): 16 bytes per lane from the first aligned address on, the elements in front of it and behind the
// last whole vector one by one.  Nothing outside [g0, g0 + count) is touched.
template <typename T, bool STORE>
__device__ __forceinline__ void zp_stage(T* __restrict__ g, T* __restrict__ lds, int count) {
    constexpr int L = 16 / (int)sizeof(T);
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    union V {
        u4 u;
        T  e[L];
    };
    const int mis  = (int)((reinterpret_cast<uintptr_t>(g) & 15u) / sizeof(T));
    const int head = min((L - mis) % L, count), nvec = (count - head) / L;
    for (int v = threadIdx.x; v < nvec; v += kZpLanes) {
        const int i = head + v * L;
        V         w;
        if constexpr (STORE) {
#pragma unroll
            for (int e = 0; e < L; ++e) w.e[e] = lds[zp_phys(i + e)];
            *reinterpret_cast<u4*>(g + i) = w.u;
        } else {
            w.u = *reinterpret_cast<const u4*>(g + i);
#pragma unroll
            for (int e = 0; e < L; ++e) lds[zp_phys(i + e)] = w.e[e];
        }
    }
    const int body_end = head + nvec * L, nscalar = head + (count - body_end);
    for (int j = threadIdx.x; j < nscalar; j += kZpLanes) {
        const int i = j < head ? j : body_end + (j - head);
        if constexpr (STORE) g[i] = lds[zp_phys(i)];
        else lds[zp_phys(i)] = g[i];
    }
}

// acc[r] = sum_k coeff(k) src[b(base + r + k)], r in [0, kZpRun): `base` is the row index of the first term of acc[0]; src holds the row's [lo, lo + cap) at
// logical element (index - lo).  REV takes the coefficients back to front (the second pass).  MAPPED: every index goes through the boundary map (and is kept
// inside the array, for the values of a cut run that nobody stores); otherwise the caller has checked that base .. base + kZpRun + W - 2 lie inside the row.
template <typename T, bool REV, bool MAPPED>
__device__ __forceinline__ void zp_run(const T* __restrict__ src, long base, long lo, int cap, const ZpArgs<T>& a, double (&acc)[kZpRun]) {
    const int W   = a.W;
    const int rel = (int)(base - lo);
    auto      ld  = [&](int m) -> double { // term m of the run: row index base + m
        int i;
        if constexpr (MAPPED) i = min(max((int)(zp_map(base + m, a.n, a.replicate != 0) - lo), 0), cap - 1);
        else i = rel + m;
        return (double)src[zp_phys(i)];
    };
    double w[kZpRun];
#pragma unroll
    for (int r = 0; r < kZpRun; ++r) acc[r] = 0.0;
#pragma unroll
    for (int m = 0; m < kZpRun - 1; ++m) w[m] = ld(m);
    int kk = 0;
    for (; kk + kZpRun <= W; kk += kZpRun) {
#pragma unroll
        for (int s = 0; s < kZpRun; ++s) {
            const int k = kk + s;
            w[(s + kZpRun - 1) % kZpRun] = ld(k + kZpRun - 1);
            const double ck = a.c[REV ? W - 1 - k : k];
#pragma unroll
            for (int r = 0; r < kZpRun; ++r) acc[r] = fma(ck, w[(r + s) % kZpRun], acc[r]);
        }
    }
#pragma unroll
    for (int s = 0; s < kZpRun - 1; ++s) { // the last W mod kZpRun coefficients
        const int k = kk + s;
        if (k < W) {
            w[(s + kZpRun - 1) % kZpRun] = ld(k + kZpRun - 1);
            const double ck = a.c[REV ? W - 1 - k : k];
#pragma unroll
            for (int r = 0; r < kZpRun; ++r) acc[r] = fma(ck, w[(r + s) % kZpRun], acc[r]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kZpLanes) void savgol_zp_kernel(const ZpArgs<T> a) {
    __shared__ T sx[zp_phys(kZpXCap) + 1];
    __shared__ T st[zp_phys(kZpTCap) + 1];
    const long   row = (long)blockIdx.x / a.tiles, tile = (long)blockIdx.x % a.tiles;
    const T*     in  = a.in + row * a.stride;
    T*           out = a.out + row * a.stride;
    const long   N = a.n, o0 = tile * kZpTile;
    const int    W = a.W, D = a.D, H = W - 1;
    const long   tlo = max(o0 - H, 0L), thi = min(o0 + kZpTile + H, N); // t[tlo, thi)
    const long   xlo = max(tlo - H, 0L), xhi = min(thi + H, N);         // x[xlo, xhi)
    const int    ct = (int)(thi - tlo), cx = (int)(xhi - xlo);

    zp_stage<T, false>(const_cast<T*>(in + xlo), sx, cx);
    __syncthreads();

    // first pass: t[j] = sum_k c[k] x[b(j - D + k)]
    for (int q = threadIdx.x; q < (ct + kZpRun - 1) / kZpRun; q += kZpLanes) { // (the ballots below see the lanes still in the loop)
        const long j0 = tlo + (long)q * kZpRun, base = j0 - D;
        const bool inside = base >= 0 && base + kZpRun + W - 2 < N;
        double     acc[kZpRun];
        if (__builtin_amdgcn_ballot_w64(!inside) == 0) zp_run<T, false, false>(sx, base, xlo, kZpXCap, a, acc);
        else zp_run<T, false, true>(sx, base, xlo, kZpXCap, a, acc);
#pragma unroll
        for (int r = 0; r < kZpRun; ++r)
            if (j0 + r < thi) st[zp_phys((int)(j0 - tlo) + r)] = (T)acc[r];
    }
    __syncthreads();

    // second pass: out[n] = sum_k c[k] t[b(n + D - k)] = sum_k' c[W - 1 - k'] t[b(n + D - (W - 1) + k')]; the outputs replace x in LDS
    const long n0 = o0 + (long)threadIdx.x * kZpRun;
    const int  co = (int)(min(o0 + kZpTile, N) - o0);
    if (n0 < N) {
        const long base   = n0 + D - H;
        const bool inside = base >= 0 && base + kZpRun + W - 2 < N;
        double     acc[kZpRun];
        if (__builtin_amdgcn_ballot_w64(!inside) == 0) zp_run<T, true, false>(st, base, tlo, kZpTCap, a, acc);
        else zp_run<T, true, true>(st, base, tlo, kZpTCap, a, acc);
#pragma unroll
        for (int r = 0; r < kZpRun; ++r) sx[zp_phys((int)threadIdx.x * kZpRun + r)] = (T)acc[r];
    }
    __syncthreads();
    zp_stage<T, true>(out + o0, sx, co);
}

struct Zp {
    gr4hip_savgol_zp_params p;
    Clamped                 c;
    double                  coeffs[kZpMaxW + 1];
    gr4hip_savgol_info      info;
};

static int zp_configure(Zp* z, const gr4hip_savgol_zp_params* p) {
    GR4_REQUIRE(p != nullptr, "savgol_zp: params is NULL");
    GR4_REQUIRE(p->dtype == GR4HIP_F32 || p->dtype == GR4HIP_F64, "savgol_zp: dtype %d (GR4HIP_F32 or GR4HIP_F64)", p->dtype);
    GR4_REQUIRE(p->boundary_policy == GR4HIP_SAVGOL_REFLECT || p->boundary_policy == GR4HIP_SAVGOL_REPLICATE, "savgol_zp: boundary_policy %d", p->boundary_policy);
    const Clamped c = clamp_settings(p->window_size, p->poly_order, p->deriv_order, GR4HIP_SAVGOL_CENTRED);
    if (c.W > (size_t)kZpMaxW) {
        set_error("savgol_zp: window_size %zu is beyond %d (the caller keeps its CPU path)", c.W, kZpMaxW);
        return GR4HIP_UNSUPPORTED;
    }
    double             cf[kZpMaxW + 1] = {};
    gr4hip_savgol_info info;
    if (p->dtype == GR4HIP_F32) {
        float f[kZpMaxW];
        if (int rc = design(p->dtype, c.W, c.p, c.d, 1.0, GR4HIP_SAVGOL_CENTRED, f, &info)) return rc;
        for (size_t k = 0; k < c.W; ++k) cf[k] = (double)f[k];
    } else if (int rc = design(p->dtype, c.W, c.p, c.d, 1.0, GR4HIP_SAVGOL_CENTRED, cf, &info)) return rc;
    z->p    = *p;
    z->c    = c;
    z->info = info;
    std::memcpy(z->coeffs, cf, sizeof cf);
    return GR4HIP_OK;
}

template <typename T>
static int zp_launch(const Zp* z, const void* d_in, void* d_out, size_t n, size_t batch, size_t row_stride, hipStream_t st) {
    ZpArgs<T> a;
    a.in        = static_cast<const T*>(d_in);
    a.out       = static_cast<T*>(d_out);
    a.n         = (long)n;
    a.stride    = (long)row_stride;
    a.tiles     = (long)ceil_div<size_t>(n, kZpTile);
    a.W         = (int)z->c.W;
    a.D         = (int)z->c.D;
    a.replicate = z->p.boundary_policy == GR4HIP_SAVGOL_REPLICATE;
    std::memcpy(a.c, z->coeffs, sizeof a.c);
    const size_t blocks = (size_t)a.tiles * batch;
    hipLaunchKernelGGL(savgol_zp_kernel<T>, dim3((unsigned)blocks), dim3(kZpLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

} // namespace sg
} // namespace gr4

struct gr4hip_savgol_zp {
    gr4::sg::Zp z;
};

extern "C" {

int gr4hip_savgol_design(int dtype, size_t window_size, size_t poly_order, size_t deriv_order, double delta, int alignment, void* h_coeffs_out,
                         gr4hip_savgol_info* info_out) {
    return gr4::sg::design(dtype, window_size, poly_order, deriv_order, delta, alignment, h_coeffs_out, info_out);
}

int gr4hip_savgol_pinv_row(int dtype, size_t window_size, size_t poly_order, size_t deriv_order, int alignment, double* h_row_out, gr4hip_savgol_info* info_out) {
    GR4_REQUIRE(dtype == GR4HIP_F32 || dtype == GR4HIP_F64, "savgol_pinv_row: dtype %d (GR4HIP_F32 or GR4HIP_F64)", dtype);
    GR4_REQUIRE(alignment == GR4HIP_SAVGOL_CENTRED || alignment == GR4HIP_SAVGOL_CAUSAL, "savgol_pinv_row: alignment %d", alignment);
    GR4_REQUIRE(h_row_out != nullptr, "savgol_pinv_row: h_row_out is NULL");
    const gr4::sg::Clamped c = gr4::sg::clamp_settings(window_size, poly_order, deriv_order, alignment);
    std::vector<double>    row;
    if (int rc = gr4::sg::pinv_row(dtype, c, row, info_out)) return rc;
    std::memcpy(h_row_out, row.data(), row.size() * sizeof(double));
    return GR4HIP_OK;
}

size_t gr4hip_savgol_zp_tile(void) { return gr4::sg::kZpTile; }

int gr4hip_savgol_zp_create(gr4hip_savgol_zp_t** h, const gr4hip_savgol_zp_params* p) {
    GR4_REQUIRE(h != nullptr, "savgol_zp_create: handle pointer is NULL");
    *h = nullptr;
    auto* z = new (std::nothrow) gr4hip_savgol_zp();
    GR4_REQUIRE(z != nullptr, "savgol_zp_create: out of memory");
    if (int rc = gr4::sg::zp_configure(&z->z, p)) {
        delete z;
        return rc;
    }
    *h = z;
    return GR4HIP_OK;
}

int gr4hip_savgol_zp_set_params(gr4hip_savgol_zp_t* h, const gr4hip_savgol_zp_params* p) {
    GR4_REQUIRE(h != nullptr && p != nullptr, "savgol_zp_set_params: NULL argument");
    GR4_REQUIRE(p->dtype == h->z.p.dtype, "savgol_zp_set_params: the dtype is fixed at create (%d, got %d)", h->z.p.dtype, p->dtype);
    return gr4::sg::zp_configure(&h->z, p); // a failed call leaves the handle as it was
}

int gr4hip_savgol_zp_coeffs(const gr4hip_savgol_zp_t* h, void* h_coeffs_out, gr4hip_savgol_info* info_out) {
    GR4_REQUIRE(h != nullptr, "savgol_zp_coeffs: handle is NULL");
    if (h_coeffs_out) {
        for (size_t k = 0; k < h->z.c.W; ++k) {
            if (h->z.p.dtype == GR4HIP_F32) static_cast<float*>(h_coeffs_out)[k] = (float)h->z.coeffs[k];
            else static_cast<double*>(h_coeffs_out)[k] = h->z.coeffs[k];
        }
    }
    if (info_out) *info_out = h->z.info;
    return GR4HIP_OK;
}

int gr4hip_savgol_zp_process(gr4hip_savgol_zp_t* h, const void* d_in, void* d_out, size_t n, size_t batch, size_t row_stride, gr4hip_stream_t stream) {
    GR4_REQUIRE(h != nullptr, "savgol_zp_process: handle is NULL");
    if (n == 0 || batch == 0) return GR4HIP_OK; // (:180)
    const size_t es = h->z.p.dtype == GR4HIP_F32 ? sizeof(float) : sizeof(double);
    GR4_REQUIRE(d_in != nullptr && d_out != nullptr, "savgol_zp_process: NULL buffer");
    GR4_REQUIRE(reinterpret_cast<uintptr_t>(d_in) % es == 0 && reinterpret_cast<uintptr_t>(d_out) % es == 0, "savgol_zp_process: a buffer is not aligned to its %zu-byte samples", es);
    GR4_REQUIRE(batch == 1 || row_stride >= n, "savgol_zp_process: row_stride %zu is shorter than the rows (%zu)", row_stride, n);
    GR4_REQUIRE(n <= (size_t(1) << 40) && row_stride <= (size_t(1) << 40) && batch <= (size_t(1) << 31), "savgol_zp_process: n %zu / row_stride %zu / batch %zu out of range", n, row_stride, batch);
    const size_t tiles = gr4::ceil_div<size_t>(n, gr4::sg::kZpTile);
    GR4_REQUIRE(tiles * batch <= 0x7fffffffull, "savgol_zp_process: %zu tiles x %zu rows is beyond one launch", tiles, batch);
    const size_t    span = ((batch - 1) * row_stride + n) * es;
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(d_in), o0 = reinterpret_cast<uintptr_t>(d_out);
    GR4_REQUIRE(i0 + span <= o0 || o0 + span <= i0, "savgol_zp_process: d_in and d_out overlap (the second pass reads neighbours the first would have overwritten)");
    hipStream_t st = gr4::as_stream(stream);
    if (h->z.p.dtype == GR4HIP_F32) return gr4::sg::zp_launch<float>(&h->z, d_in, d_out, n, batch, row_stride, st);
    return gr4::sg::zp_launch<double>(&h->z, d_in, d_out, n, batch, row_stride, st);
}

int gr4hip_savgol_zp_destroy(gr4hip_savgol_zp_t* h) {
    delete h;
    return GR4HIP_OK;
}

} // extern "C"
