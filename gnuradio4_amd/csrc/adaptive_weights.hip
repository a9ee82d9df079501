// adaptive_weights.hip -- adaptive (MVDR / Capon) beamformer weights from the X-engine's matrices on gfx950 (ADAPTIVE_WEIGHTS.md): C-ABI gr4hip_mvdr_* and its
// one kernel, a batched per-bin Hermitian positive-definite solve in float64.
//
//   V[q][p][c], complex<float>: what gr4hip_xcorr_process writes, packed lower triangle p = i (i + 1) / 2 + j, j <= i, bin fastest, 2 <= S <= 32
//   a[b][s][c], complex<float>: steering vectors, 1 <= B <= 32, laid out as the beamformer's weights;   loading >= 0, a double
//   all arithmetic float64, per matrix q and bin c:
//       R_ij = V_ij (j < i),  R_ji = conj(V_ij),  R_ii = Re V_ii (the imaginary part is ignored)
//       lambda = loading * (sum_i R_ii) / S ;   R'_ii = R_ii + lambda
//       R' = L L^H   Cholesky, columns j ascending, every inner sum with k ascending:
//           s_j  = R'_jj - sum_{k<j} |L_jk|^2 ;   L_jj = sqrt(s_j)
//           L_ij = (R'_ij - sum_{k<j} L_ik conj(L_jk)) / L_jj            (i > j)
//       per beam b:   L y = a_b  (forward, k ascending) ;   d = sum_k |y_k|^2
//                     L^H u = y  (backward) ;   w = u / d
//       W[q][b][s][c] = conj(w_s)  rounded once to complex<float>
//       P[q][b][c]    = (float)(1 / d)
//   a pivot s_j that is not > 0 (NaN included) fails the bin: every W and P of that (q, c) is a quiet NaN and the bin is counted
//
// The reference has no such block: the definition is this project's, tests/adaptive_weights_oracle.py pins it.  The device evaluates every product-and-subtract
// as a chain of float64 fma in the order above (mv_msub / mv_msub_conj below); division and sqrt are the compiler's correctly rounded ones.
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace gr4 {

constexpr int    kMvMax        = 32;              // streams, beams
constexpr size_t kMvMaxBins    = size_t(1) << 20;
constexpr size_t kMvMaxWeights = size_t(1) << 24; // B S n_bins, as the beamformer's
constexpr int    kMvLdsBudget  = 160 * 1024;      // LDS of one CU: a workgroup may take all of it

typedef float  mv_f2 __attribute__((ext_vector_type(2)));
typedef double mv_d2 __attribute__((ext_vector_type(2)));

struct MvArgs {
    const float*        vis;    // [n_spectra][P][N] complex
    const float*        steer;  // [B][S][N] complex
    float*              w;      // [n_spectra][B][S][N] complex
    float*              power;  // [n_spectra][B][N] or null
    unsigned long long* failed; // device counter
    double              loading;
    int                 S, B, N, P;
    int                 tb;     // bins per workgroup = waves per workgroup
    int                 bg;     // beams per pass
    int                 tiles;  // ceil(N / tb)
    int                 stride; // bytes of LDS per bin
};

// t -= a b, complex, as four fma: re -= ar br;  re += ai bi;  im -= ar bi;  im -= ai br
__device__ __forceinline__ mv_d2 mv_msub(mv_d2 t, mv_d2 a, mv_d2 b) {
    t.x = __builtin_fma(-a.x, b.x, t.x);
    t.x = __builtin_fma(a.y, b.y, t.x);
    t.y = __builtin_fma(-a.x, b.y, t.y);
    t.y = __builtin_fma(-a.y, b.x, t.y);
    return t;
}
// t -= a conj(b): re -= ar br;  re -= ai bi;  im -= ai br;  im += ar bi
__device__ __forceinline__ mv_d2 mv_msub_conj(mv_d2 t, mv_d2 a, mv_d2 b) {
    t.x = __builtin_fma(-a.x, b.x, t.x);
    t.x = __builtin_fma(-a.y, b.y, t.x);
    t.y = __builtin_fma(-a.y, b.x, t.y);
    t.y = __builtin_fma(a.x, b.y, t.y);
    return t;
}

// what one lane stored to LDS another lane of the same wave reads next: the wave's DS operations complete in order, the compiler must keep them so
__device__ __forceinline__ void mv_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One workgroup: one matrix q and a tile of tb neighbouring bins; wave w owns bin c0 + w.  LDS per bin (stride bytes): the packed triangle M[P] as complex128
// (R', then L in place) and Y[S][bg] complex128 (a_b, then y, then u in place, then W as complex<float> in the slot's first 8 bytes with P in the next 4; the staging threads take P from row 0).
// The workgroup stages V, the steering vectors and the results with its threads running along the bins first, so HBM sees rows of tb values; the waves read and
// write only LDS.
//   Cholesky: lane i owns row i (left-looking: column j of L from the finished columns k < j, the sum in a register), the pivot comes from lane j.
//   solves:   lane b owns beam b of the pass; L_ik is one LDS address for all lanes (a broadcast), y_k the lane's own column of Y.
// Every loop runs to S, j or i: no trip count depends on the data.  A failed bin goes on computing with NaN and is replaced at the wave's store.
__global__ __launch_bounds__(1024) void mvdr_kernel(const MvArgs a) {
    extern __shared__ __align__(16) unsigned char mv_lds[];
    const int  S = a.S, B = a.B, N = a.N, P = a.P, TB = a.tb, BG = a.bg;
    const long q  = blockIdx.x / a.tiles;
    const int  c0 = (int)(blockIdx.x - q * a.tiles) * TB;
    const int  t = threadIdx.x, nt = TB * 64, lane = t & 63, wv = t >> 6;
    const bool live = c0 + wv < N; // (wave-uniform) the ragged tile's waves past N stage nothing, solve nothing and count nothing

    // ---- V -> M as float64, threads along bins
    const float* vq = a.vis + q * (long)P * N * 2;
    for (int idx = t; idx < P * TB; idx += nt) {
        const int p = idx / TB, cl = idx - p * TB;
        if (c0 + cl < N) {
            const mv_f2 v = *reinterpret_cast<const mv_f2*>(vq + ((long)p * N + c0 + cl) * 2);
            mv_d2       d;
            d.x = (double)v.x;
            d.y = (double)v.y;
            reinterpret_cast<mv_d2*>(mv_lds + (size_t)cl * a.stride)[p] = d;
        }
    }
    __syncthreads();

    mv_d2* const M = reinterpret_cast<mv_d2*>(mv_lds + (size_t)wv * a.stride);
    mv_d2* const Y = M + P;
    bool         ok = true;
    if (live) {
        // relative diagonal loading: the trace with i ascending, in every lane
        double tr = 0.0;
        for (int i = 0; i < S; ++i) tr = tr + M[i * (i + 1) / 2 + i].x;
        const double lambda = a.loading * tr / (double)S;
        mv_wave_sync();
        if (lane < S) M[lane * (lane + 1) / 2 + lane].x += lambda;
        mv_wave_sync();
        // Cholesky.  A lane outside [j, S) computes row j or S - 1 again and stores nothing.
        for (int j = 0; j < S; ++j) {
            const int i   = lane < j ? j : (lane < S ? lane : S - 1);
            const int ri  = i * (i + 1) / 2, rj = j * (j + 1) / 2;
            mv_d2     acc = M[ri + j];
            if (i == j) acc.y = 0.0;
            for (int k = 0; k < j; ++k) acc = mv_msub_conj(acc, M[ri + k], M[rj + k]);
            const double sj = __shfl(acc.x, j); // lane j's row is row j: s_j
            ok              = ok && (sj > 0.0);
            const double d  = __builtin_sqrt(sj);
            mv_d2        l;
            l.x = lane == j ? d : acc.x / d;
            l.y = lane == j ? 0.0 : acc.y / d;
            mv_wave_sync();
            if (lane >= j && lane < S) M[ri + j] = l;
            mv_wave_sync();
        }
        if (!ok && lane == 0) atomicAdd(a.failed, 1ull);
    }

    const float qnan = __builtin_nanf("");
    for (int b0 = 0; b0 < B; b0 += BG) { // (uniform)
        const int nb = B - b0 < BG ? B - b0 : BG;
        // ---- a -> Y as float64, threads along bins
        for (int idx = t; idx < nb * S * TB; idx += nt) {
            const int r = idx / TB, cl = idx - r * TB; // r = bl S + s
            if (c0 + cl < N) {
                const int   bl = r / S, s = r - bl * S;
                const mv_f2 v  = *reinterpret_cast<const mv_f2*>(a.steer + (((long)(b0 + bl) * S + s) * N + c0 + cl) * 2);
                mv_d2       d;
                d.x = (double)v.x;
                d.y = (double)v.y;
                reinterpret_cast<mv_d2*>(mv_lds + (size_t)cl * a.stride)[P + s * BG + bl] = d;
            }
        }
        __syncthreads();
        if (live && lane < nb) {
            mv_d2* const y = Y + lane; // the lane's column: y[k BG]
            double       d = 0.0;
            for (int i = 0; i < S; ++i) { // L y = a_b
                const int ri  = i * (i + 1) / 2;
                mv_d2     acc = y[i * BG];
                for (int k = 0; k < i; ++k) acc = mv_msub(acc, M[ri + k], y[k * BG]);
                const double lii = M[ri + i].x;
                acc.x            = acc.x / lii;
                acc.y            = acc.y / lii;
                y[i * BG]        = acc;
                d                = __builtin_fma(acc.x, acc.x, d);
                d                = __builtin_fma(acc.y, acc.y, d);
            }
            for (int i = S - 1; i >= 0; --i) { // L^H u = y, u over y
                mv_d2 acc = y[i * BG];
                for (int k = i + 1; k < S; ++k) {
                    mv_d2 l = M[k * (k + 1) / 2 + i];
                    l.y     = -l.y;
                    acc     = mv_msub(acc, l, y[k * BG]);
                }
                const double lii = M[i * (i + 1) / 2 + i].x;
                acc.x            = acc.x / lii;
                acc.y            = acc.y / lii;
                y[i * BG]        = acc;
            }
            mv_f2 pw;
            pw.x = ok ? (float)(1.0 / d) : qnan;
            pw.y = 0.f;
            for (int s = 0; s < S; ++s) { // W = conj(u / d), rounded once: the bits of the two floats go into the slot's first double, P into the second
                const mv_d2 u = y[s * BG];
                mv_f2       w;
                w.x = ok ? (float)(u.x / d) : qnan;
                w.y = ok ? (float)(-(u.y / d)) : qnan;
                mv_d2 slot;
                slot.x    = __builtin_bit_cast(double, w);
                slot.y    = __builtin_bit_cast(double, pw);
                y[s * BG] = slot;
            }
        }
        __syncthreads();
        // ---- results -> HBM, threads along bins
        float* wq = a.w + (q * B + b0) * (long)S * N * 2;
        for (int idx = t; idx < nb * S * TB; idx += nt) {
            const int r = idx / TB, cl = idx - r * TB;
            if (c0 + cl < N) {
                const int bl = r / S, s = r - bl * S;
                const mv_d2 slot = reinterpret_cast<const mv_d2*>(mv_lds + (size_t)cl * a.stride)[P + s * BG + bl];
                const double bits = slot.x; // (a copy: __builtin_bit_cast of a vector element reads the vector's first bytes)
                *reinterpret_cast<mv_f2*>(wq + ((long)r * N + c0 + cl) * 2) = __builtin_bit_cast(mv_f2, bits);
            }
        }
        if (a.power) {
            float* pq = a.power + (q * B + b0) * (long)N;
            for (int idx = t; idx < nb * TB; idx += nt) {
                const int bl = idx / TB, cl = idx - bl * TB;
                if (c0 + cl < N) {
                    const mv_d2  slot = reinterpret_cast<const mv_d2*>(mv_lds + (size_t)cl * a.stride)[P + bl]; // row 0 of the beam
                    const double bits = slot.y;
                    pq[(long)bl * N + c0 + cl] = __builtin_bit_cast(mv_f2, bits).x;
                }
            }
        }
        __syncthreads(); // the next pass stages over Y
    }
}

// LDS bytes of one bin: P + S bg complex128, made an odd number of 16-byte slots so that the staging threads, which run along the bins, spread over the banks
static size_t mv_stride(size_t S, size_t bg) {
    const size_t slots = S * (S + 1) / 2 + S * bg;
    return (slots | 1) * 16;
}

// bins per workgroup and beams per pass from the LDS one bin needs: the widest tile of 16, 8, 4 bins that leaves room for min(B, 8) beams per pass, then as many
// beams as fit, evened out over the passes.  S = 8: 16 bins, every beam (B = 32: 73 KiB, two workgroups per CU; B <= 8: 25 KiB, the 32-waves cap allows two);
// S = 32: 8 bins and up to 23 beams (B = 32: two passes of 16, 130 KiB, one workgroup per CU).
static void mv_geometry(size_t S, size_t B, int* tb, int* bg) {
    const size_t P = S * (S + 1) / 2;
    for (int t : {16, 8, 4}) {
        const size_t per = (size_t)kMvLdsBudget / t - 16;
        if (per < P * 16) continue;
        const size_t fit = (per - P * 16) / (S * 16);
        if (fit >= std::min<size_t>(B, 8)) {
            const size_t g      = std::min(B, fit);
            const size_t passes = (B + g - 1) / g;
            *tb = t;
            *bg = (int)((B + passes - 1) / passes);
            return;
        }
    }
    *tb = 2; // (not reached for S <= 32: 4 bins of 8448 + 8 S 16 bytes fit)
    *bg = 1;
}

} // namespace gr4

using namespace gr4;

struct gr4hip_mvdr {
    size_t              S = 0, B = 0, N = 0;
    double              loading = 0.0; // a kernel argument: set_loading holds for the calls enqueued after it
    DeviceBuffer        d_steer, d_cnt;
    bool                have_steer = false;
    unsigned long long  bins = 0; // (matrix, bin) pairs launched since create
    hipStream_t         last = nullptr;
    unsigned long long* h_cnt = nullptr; // page-locked: where stats() receives the device counter
    ~gr4hip_mvdr() {
        if (h_cnt) hip_quiet(hipHostFree(h_cnt));
    }
};

static bool mv_overlap(const void* p, size_t pb, const void* r, size_t rb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)r;
    return a < b + rb && b < a + pb;
}

extern "C" {

int gr4hip_mvdr_create(gr4hip_mvdr_t** out, size_t n_streams, size_t n_beams, size_t n_bins) {
    GR4_REQUIRE(out, "mvdr: null output handle");
    GR4_REQUIRE(n_streams >= 2, "mvdr: n_streams must be >= 2");
    GR4_REQUIRE(n_beams >= 1, "mvdr: n_beams must be >= 1");
    GR4_REQUIRE(n_bins >= 2, "mvdr: n_bins must be >= 2 (got %zu)", n_bins);
    if (n_streams > (size_t)kMvMax || n_beams > (size_t)kMvMax) { set_error("mvdr: %zu streams, %zu beams (supported: up to %d of each)", n_streams, n_beams, kMvMax); return GR4HIP_UNSUPPORTED; }
    if (n_bins > kMvMaxBins) { set_error("mvdr: %zu bins (supported: up to %zu)", n_bins, kMvMaxBins); return GR4HIP_UNSUPPORTED; }
    if (n_beams * n_streams * n_bins > kMvMaxWeights) { set_error("mvdr: %zu weights (supported: up to %zu)", n_beams * n_streams * n_bins, kMvMaxWeights); return GR4HIP_UNSUPPORTED; }
    auto* h = new (std::nothrow) gr4hip_mvdr();
    GR4_REQUIRE(h, "out of host memory");
    h->S = n_streams;
    h->B = n_beams;
    h->N = n_bins;
    *out = h; // the device buffers come with the first set_steering: everything up to there is host code
    return GR4HIP_OK;
}

int gr4hip_mvdr_set_steering(gr4hip_mvdr_t* h, const float* d_steer, gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "mvdr_set_steering: null handle");
    GR4_REQUIRE(d_steer, "mvdr_set_steering: null steering vectors");
    GR4_REQUIRE((uintptr_t)d_steer % 8 == 0, "mvdr_set_steering: the steering vectors must be aligned to 8 bytes");
    if (const int rc = have_device("mvdr")) return rc;
    const hipStream_t st = as_stream(stream);
    if (!h->d_cnt.ptr) {
        if (const int rc = h->d_cnt.ensure(sizeof(unsigned long long))) return rc;
        GR4_HIP_TRY(hipMemsetAsync(h->d_cnt.ptr, 0, sizeof(unsigned long long), st));
        h->last = st;
    }
    if (!h->h_cnt) {
        if (hipHostMalloc(reinterpret_cast<void**>(&h->h_cnt), sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            h->h_cnt = nullptr;
            set_error("mvdr: no page-locked memory for the counter");
            return GR4HIP_RUNTIME_ERROR;
        }
        // the kernel may take all of a CU's LDS
        GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mvdr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMvLdsBudget));
    }
    const size_t bytes = h->B * h->S * h->N * 2 * sizeof(float);
    if (const int rc = h->d_steer.ensure(bytes)) return rc;
    GR4_HIP_TRY(hipMemcpyAsync(h->d_steer.ptr, d_steer, bytes, hipMemcpyDeviceToDevice, st));
    h->have_steer = true;
    return GR4HIP_OK;
}

int gr4hip_mvdr_set_loading(gr4hip_mvdr_t* h, double loading) {
    GR4_REQUIRE(h, "mvdr_set_loading: null handle");
    GR4_REQUIRE(std::isfinite(loading) && loading >= 0.0, "mvdr_set_loading: loading must be finite and >= 0 (got %g)", loading);
    h->loading = loading;
    return GR4HIP_OK;
}

int gr4hip_mvdr_process(gr4hip_mvdr_t* h, const float* d_vis, size_t n_spectra, float* d_weights, float* d_power, gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "mvdr_process: null handle");
    if (n_spectra == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_vis, "mvdr_process: null matrices");
    GR4_REQUIRE(d_weights, "mvdr_process: null weights output");
    GR4_REQUIRE((uintptr_t)d_vis % 8 == 0 && (uintptr_t)d_weights % 8 == 0, "mvdr_process: the matrices and the weights must be aligned to 8 bytes");
    GR4_REQUIRE((uintptr_t)d_power % 4 == 0, "mvdr_process: the power output must be aligned to 4 bytes");
    const size_t P = h->S * (h->S + 1) / 2;
    GR4_REQUIRE(n_spectra <= (size_t(1) << 40) / (h->B * h->S * h->N), "mvdr_process: %zu matrices in one call", n_spectra);
    const size_t vb = n_spectra * P * h->N * 8, wb = n_spectra * h->B * h->S * h->N * 8, pb = n_spectra * h->B * h->N * 4;
    GR4_REQUIRE(!mv_overlap(d_weights, wb, d_vis, vb), "mvdr_process: the weights overlap the matrices");
    if (d_power) {
        GR4_REQUIRE(!mv_overlap(d_power, pb, d_vis, vb), "mvdr_process: the power output overlaps the matrices");
        GR4_REQUIRE(!mv_overlap(d_power, pb, d_weights, wb), "mvdr_process: the power output overlaps the weights");
    }
    GR4_REQUIRE(h->have_steer, "mvdr_process: no steering vectors yet (gr4hip_mvdr_set_steering)");
    GR4_REQUIRE(!mv_overlap(d_weights, wb, h->d_steer.ptr, h->d_steer.bytes) && !(d_power && mv_overlap(d_power, pb, h->d_steer.ptr, h->d_steer.bytes)),
                "mvdr_process: an output overlaps the handle's steering vectors");
    MvArgs a{};
    a.steer   = static_cast<const float*>(h->d_steer.ptr);
    a.failed  = static_cast<unsigned long long*>(h->d_cnt.ptr);
    a.loading = h->loading;
    a.S       = (int)h->S;
    a.B       = (int)h->B;
    a.N       = (int)h->N;
    a.P       = (int)P;
    mv_geometry(h->S, h->B, &a.tb, &a.bg);
    a.tiles  = (int)((h->N + a.tb - 1) / a.tb);
    a.stride = (int)mv_stride(h->S, (size_t)a.bg);
    const size_t      lds   = (size_t)a.stride * a.tb;
    const size_t      piece = 0x7fffffffu / (size_t)a.tiles; // matrices per launch (a cut like any other: the values do not depend on it)
    const hipStream_t st    = as_stream(stream);
    for (size_t q = 0; q < n_spectra; q += piece) {
        const size_t m = std::min(piece, n_spectra - q);
        a.vis   = d_vis + q * P * h->N * 2;
        a.w     = d_weights + q * h->B * h->S * h->N * 2;
        a.power = d_power ? d_power + q * h->B * h->N : nullptr;
        hipLaunchKernelGGL(mvdr_kernel, dim3((unsigned)(m * a.tiles)), dim3((unsigned)(64 * a.tb)), lds, st, a);
        GR4_LAUNCH_CHECK();
    }
    h->bins += (unsigned long long)n_spectra * h->N;
    h->last = st;
    return GR4HIP_OK;
}

int gr4hip_mvdr_stats(gr4hip_mvdr_t* h, unsigned long long* bins_solved, unsigned long long* bins_failed) {
    GR4_REQUIRE(h, "mvdr_stats: null handle");
    unsigned long long failed = 0;
    if (h->d_cnt.ptr && h->h_cnt) { // (before the first set_steering there is nothing on the device)
        GR4_HIP_TRY(hipMemcpyAsync(h->h_cnt, h->d_cnt.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->last));
        GR4_HIP_TRY(hipStreamSynchronize(h->last));
        failed = *h->h_cnt;
    }
    if (bins_solved) *bins_solved = h->bins - failed;
    if (bins_failed) *bins_failed = failed;
    return GR4HIP_OK;
}

int gr4hip_mvdr_destroy(gr4hip_mvdr_t* h) {
    delete h;
    return GR4HIP_OK;
}

} // extern "C"
