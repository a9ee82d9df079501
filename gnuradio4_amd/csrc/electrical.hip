// electrical.hip -- gr::electrical::PowerFactor and gr::electrical::SystemUnbalance (blocks/electrical/.../PowerEstimators.hpp:144-257) as streaming kernels, and
// the stateless entry points gr4hip_powerfactor_process / gr4hip_unbalance_process.  The arithmetic is gr4/electrical_ops.hpp, the host mirror blocks' own.
//
// Both blocks are per sample and HBM-bound, so the kernels have the shape of convert_kernel (convert.hip): a lane moves L = 16 bytes / sizeof(T) consecutive
// samples of a row per access and keeps kElItems / L such vectors per row in flight; every row is contiguous across the lanes of a wave.  Rows need the alignment
// of T only and sit a stride apart, so they need not agree: [0, n) is cut into an element-wise head, a body of kElItems samples per lane and an element-wise tail,
// with the head chosen (on the host) so that as many rows as possible have their body accesses 16-byte aligned; a row that stays off moves its L samples element
// by element, for that row alone.  The power factor's phases are independent rows (blockIdx.y, a head per phase); the unbalance kernel's lane holds all N phases
// of its samples, N = 2 and 3 at compile time, any other N as a run-time loop over the rows that keeps only sums and maxima in registers.
#include "common.hpp"
#include "../host/include/gr4/electrical_ops.hpp"

#include <cmath>

namespace gr4 {
namespace el {

namespace ops = gr4::electrical_ops;

constexpr int kElLanes  = 256;
constexpr int kElItems  = 8;                   // samples per lane and row: two 16-byte vectors of float, four of double
constexpr int kElTile   = kElLanes * kElItems; // samples per workgroup (gr4hip_electrical_tile)
constexpr int kElPhases = 16;

template <int BYTES> struct VecB;
template <> struct VecB<16> { typedef unsigned int type __attribute__((ext_vector_type(4))); };
template <typename T, int N> union ElVec {
    typename VecB<(int)sizeof(T) * N>::type u;
    T                                        e[N];
};

template <typename T> __device__ __forceinline__ bool el_aligned(const T* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// L samples from src on: one aligned 16-byte access, or element by element (vec is uniform across the workgroup).  NT: streamed once.
template <typename T, int L, bool NT>
__device__ __forceinline__ void el_load(const T* __restrict__ src, bool vec, T (&x)[L]) {
    if (vec) {
        ElVec<T, L> v;
        const auto* p = reinterpret_cast<const typename VecB<16>::type*>(src);
        if constexpr (NT) v.u = __builtin_nontemporal_load(p);
        else v.u = *p;
#pragma unroll
        for (int e = 0; e < L; ++e) x[e] = v.e[e];
    } else {
#pragma unroll
        for (int e = 0; e < L; ++e) x[e] = src[e];
    }
}
template <typename T, int L>
__device__ __forceinline__ void el_store(T* __restrict__ dst, bool vec, const T (&y)[L]) {
    if (vec) {
        ElVec<T, L> v;
#pragma unroll
        for (int e = 0; e < L; ++e) v.e[e] = y[e];
        __builtin_nontemporal_store(v.u, reinterpret_cast<typename VecB<16>::type*>(dst));
    } else {
#pragma unroll
        for (int e = 0; e < L; ++e) dst[e] = y[e];
    }
}

// ---------------------------------------------------------------------------------------------------------------- PowerFactor
template <typename T>
struct PfArgs {
    const T*      P;
    const T*      S;
    T*            pf; // (may be null)
    T*            ph; // (may be null)
    long          in_stride, out_stride, n;
    unsigned char head[kElPhases]; // per phase: the samples in front of the body
};

template <typename T>
__global__ __launch_bounds__(kElLanes) void powerfactor_kernel(const PfArgs<T> a) {
    constexpr int L = 16 / (int)sizeof(T), SL = kElItems / L;
    const long    r = blockIdx.y;
    const T*      P  = a.P + r * a.in_stride;
    const T*      S  = a.S + r * a.in_stride;
    T*            pf = a.pf ? a.pf + r * a.out_stride : nullptr;
    T*            ph = a.ph ? a.ph + r * a.out_stride : nullptr;
    const long    head = min((long)a.head[r], a.n), nvec = (a.n - head) / L;
    const long    v0   = (long)blockIdx.x * (kElLanes * SL) + threadIdx.x;
    if (v0 < nvec) { // all loads of the lane first: 2 SL accesses in flight
        const bool vP = el_aligned(P + head), vS = el_aligned(S + head), vf = pf && el_aligned(pf + head), vh = ph && el_aligned(ph + head);
        T          p[SL][L], s[SL][L];
#pragma unroll
        for (int k = 0; k < SL; ++k) {
            const long v = v0 + (long)k * kElLanes;
            if (v < nvec) {
                el_load<T, L, true>(P + head + v * L, vP, p[k]);
                el_load<T, L, true>(S + head + v * L, vS, s[k]);
            } else {
#pragma unroll
                for (int e = 0; e < L; ++e) p[k][e] = s[k][e] = T(0);
            }
        }
#pragma unroll
        for (int k = 0; k < SL; ++k) {
            const long v = v0 + (long)k * kElLanes;
            T          c[L];
#pragma unroll
            for (int e = 0; e < L; ++e) c[e] = ops::power_factor<T>(p[k][e], s[k][e]);
            if (v < nvec && pf) el_store<T, L>(pf + head + v * L, vf, c);
            if (v < nvec && ph) { // (uniform: an unconnected phase port costs no acos)
#pragma unroll
                for (int e = 0; e < L; ++e) c[e] = ops::acos_of(c[e]);
                el_store<T, L>(ph + head + v * L, vh, c);
            }
        }
    }
    const long body_end = head + nvec * L, nscalar = head + (a.n - body_end);
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < nscalar; j += (long)gridDim.x * blockDim.x) { // head and tail samples
        const long i = j < head ? j : body_end + (j - head);
        const T    c = ops::power_factor<T>(P[i], S[i]);
        if (pf) pf[i] = c;
        if (ph) ph[i] = ops::acos_of(c);
    }
}

// ---------------------------------------------------------------------------------------------------------------- SystemUnbalance
template <typename T>
struct UbArgs {
    const T* U;
    const T* I;
    const T* P;
    T*       Pt; // (any may be null)
    T*       Uu;
    T*       Iu;
    long     in_stride, n, head;
    int      n_phases;
};

// NC: the phase count at compile time, 0: a.n_phases
template <typename T, int NC>
__global__ __launch_bounds__(kElLanes) void unbalance_kernel(const UbArgs<T> a) {
    constexpr int L = 16 / (int)sizeof(T), SL = kElItems / L;
    const int     N = NC ? NC : a.n_phases;
    const long    head = a.head, nvec = (a.n - head) / L;
    const long    v0   = (long)blockIdx.x * (kElLanes * SL) + threadIdx.x;
    if (v0 < nvec) {
        const bool vt = a.Pt && el_aligned(a.Pt + head), vu = a.Uu && el_aligned(a.Uu + head), vi = a.Iu && el_aligned(a.Iu + head);
        if constexpr (NC != 0) { // every row of the lane's samples in registers: all loads first
            T u[SL][NC][L], c[SL][NC][L], p[SL][NC][L];
#pragma unroll
            for (int k = 0; k < SL; ++k) {
                const long v = v0 + (long)k * kElLanes;
#pragma unroll
                for (int i = 0; i < NC; ++i) {
                    const long o = (long)i * a.in_stride + head;
#pragma unroll
                    for (int e = 0; e < L; ++e) u[k][i][e] = c[k][i][e] = p[k][i][e] = T(0);
                    if (v < nvec) { // (a row no connected output needs is not read: uniform)
                        if (a.Uu) el_load<T, L, true>(a.U + o + v * L, el_aligned(a.U + o), u[k][i]);
                        if (a.Iu) el_load<T, L, true>(a.I + o + v * L, el_aligned(a.I + o), c[k][i]);
                        if (a.Pt) el_load<T, L, true>(a.P + o + v * L, el_aligned(a.P + o), p[k][i]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < SL; ++k) {
                const long v = v0 + (long)k * kElLanes;
                if (v >= nvec) continue;
                T y[L];
                if (a.Pt) {
#pragma unroll
                    for (int e = 0; e < L; ++e) y[e] = ops::sum_of<T>([&](int i) { return p[k][i][e]; }, NC);
                    el_store<T, L>(a.Pt + head + v * L, vt, y);
                }
                if (a.Uu) {
#pragma unroll
                    for (int e = 0; e < L; ++e) y[e] = ops::voltage_unbalance<T>([&](int i) { return u[k][i][e]; }, NC);
                    el_store<T, L>(a.Uu + head + v * L, vu, y);
                }
                if (a.Iu) {
#pragma unroll
                    for (int e = 0; e < L; ++e) y[e] = ops::current_unbalance<T>([&](int i) { return c[k][i][e]; }, NC);
                    el_store<T, L>(a.Iu + head + v * L, vi, y);
                }
            }
        } else { // two passes over the rows (the second from the cache): only sums, averages and maxima stay in registers
            T su[SL][L], si[SL][L], sp[SL][L], m[SL][L], best[SL][L];
#pragma unroll
            for (int k = 0; k < SL; ++k)
#pragma unroll
                for (int e = 0; e < L; ++e) su[k][e] = si[k][e] = sp[k][e] = m[k][e] = best[k][e] = T(0);
            for (int i = 0; i < N; ++i) {
                const long o  = (long)i * a.in_stride + head;
                const bool au = el_aligned(a.U + o), ai = el_aligned(a.I + o), ap = el_aligned(a.P + o);
#pragma unroll
                for (int k = 0; k < SL; ++k) {
                    const long v = v0 + (long)k * kElLanes;
                    if (v >= nvec) continue;
                    T x[L];
                    if (a.Uu) {
                        el_load<T, L, false>(a.U + o + v * L, au, x);
#pragma unroll
                        for (int e = 0; e < L; ++e) su[k][e] = su[k][e] + x[e];
                    }
                    if (a.Iu) {
                        el_load<T, L, false>(a.I + o + v * L, ai, x);
#pragma unroll
                        for (int e = 0; e < L; ++e) {
                            si[k][e] = si[k][e] + x[e];
                            if (i == 0) best[k][e] = x[e];
                        }
                    }
                    if (a.Pt) {
                        el_load<T, L, true>(a.P + o + v * L, ap, x);
#pragma unroll
                        for (int e = 0; e < L; ++e) sp[k][e] = sp[k][e] + x[e];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < SL; ++k)
#pragma unroll
                for (int e = 0; e < L; ++e) {
                    su[k][e] = ops::mean_of<T>(su[k][e], N);
                    si[k][e] = ops::mean_of<T>(si[k][e], N);
                }
            if (a.Uu || a.Iu) {
                for (int i = 0; i < N; ++i) {
                    const long o  = (long)i * a.in_stride + head;
                    const bool au = el_aligned(a.U + o), ai = el_aligned(a.I + o);
#pragma unroll
                    for (int k = 0; k < SL; ++k) {
                        const long v = v0 + (long)k * kElLanes;
                        if (v >= nvec) continue;
                        T x[L];
                        if (a.Uu) {
                            el_load<T, L, false>(a.U + o + v * L, au, x);
#pragma unroll
                            for (int e = 0; e < L; ++e) ops::voltage_step<T>(m[k][e], x[e], su[k][e]);
                        }
                        if (a.Iu && i > 0) {
                            el_load<T, L, false>(a.I + o + v * L, ai, x);
#pragma unroll
                            for (int e = 0; e < L; ++e) ops::current_step<T>(best[k][e], x[e], si[k][e]);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < SL; ++k) {
                const long v = v0 + (long)k * kElLanes;
                if (v >= nvec) continue;
                T y[L];
                if (a.Pt) el_store<T, L>(a.Pt + head + v * L, vt, sp[k]);
                if (a.Uu) {
#pragma unroll
                    for (int e = 0; e < L; ++e) y[e] = ops::percent_of<T>(m[k][e], su[k][e]);
                    el_store<T, L>(a.Uu + head + v * L, vu, y);
                }
                if (a.Iu) {
#pragma unroll
                    for (int e = 0; e < L; ++e) y[e] = ops::percent_of<T>(ops::abs_of(best[k][e] - si[k][e]), si[k][e]);
                    el_store<T, L>(a.Iu + head + v * L, vi, y);
                }
            }
        }
    }
    const long body_end = head + nvec * L, nscalar = head + (a.n - body_end);
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < nscalar; j += (long)gridDim.x * blockDim.x) { // head and tail samples, read in place
        const long i = j < head ? j : body_end + (j - head);
        if (a.Pt) a.Pt[i] = ops::sum_of<T>([&](int k) { return a.P[(long)k * a.in_stride + i]; }, N);
        if (a.Uu) a.Uu[i] = ops::voltage_unbalance<T>([&](int k) { return a.U[(long)k * a.in_stride + i]; }, N);
        if (a.Iu) a.Iu[i] = ops::current_unbalance<T>([&](int k) { return a.I[(long)k * a.in_stride + i]; }, N);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// the fewest samples after which the most of the given row starts are 16-byte aligned (rows aligned to T: the head is below 16 / sizeof(T))
static long pick_head(const uintptr_t* rows, int count, size_t esize) {
    const long L = (long)(16 / esize);
    long       head = 0;
    int        best = -1;
    for (long hd = 0; hd < L; ++hd) {
        int ok = 0;
        for (int k = 0; k < count; ++k) ok += rows[k] && (rows[k] + (uintptr_t)hd * esize) % 16 == 0;
        if (ok > best) {
            best = ok;
            head = hd;
        }
    }
    return head;
}

static bool overlaps(uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) { return !(a + a_bytes <= b || b + b_bytes <= a); }

template <typename T>
static int launch_powerfactor(size_t np, const void* d_P, const void* d_S, size_t in_stride, void* d_pf, void* d_ph, size_t out_stride, size_t n, hipStream_t st) {
    constexpr long L = 16 / (long)sizeof(T);
    PfArgs<T>      a{};
    a.P          = static_cast<const T*>(d_P);
    a.S          = static_cast<const T*>(d_S);
    a.pf         = static_cast<T*>(d_pf);
    a.ph         = static_cast<T*>(d_ph);
    a.in_stride  = (long)in_stride;
    a.out_stride = (long)out_stride;
    a.n          = (long)n;
    long nvec_max = 0;
    for (size_t r = 0; r < np; ++r) {
        const uintptr_t rows[4] = {reinterpret_cast<uintptr_t>(a.P + r * in_stride), reinterpret_cast<uintptr_t>(a.S + r * in_stride),
                                   a.pf ? reinterpret_cast<uintptr_t>(a.pf + r * out_stride) : 0, a.ph ? reinterpret_cast<uintptr_t>(a.ph + r * out_stride) : 0};
        const long      head    = std::min<long>(pick_head(rows, 4, sizeof(T)), (long)n);
        a.head[r]               = (unsigned char)head;
        nvec_max                = std::max(nvec_max, ((long)n - head) / L);
    }
    const long per_block = kElLanes * (kElItems / L);
    GR4_REQUIRE(ceil_div(nvec_max + 1, per_block) < (1L << 31), "powerfactor: span too long for one launch");
    const unsigned grid = (unsigned)std::max<long>(ceil_div(nvec_max, per_block), 1L);
    hipLaunchKernelGGL(powerfactor_kernel<T>, dim3(grid, (unsigned)np), dim3(kElLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

template <typename T>
static int launch_unbalance(size_t np, const void* d_U, const void* d_I, const void* d_P, size_t in_stride, void* d_Pt, void* d_Uu, void* d_Iu, size_t n, hipStream_t st) {
    constexpr long L = 16 / (long)sizeof(T);
    UbArgs<T>      a{};
    a.U         = static_cast<const T*>(d_U);
    a.I         = static_cast<const T*>(d_I);
    a.P         = static_cast<const T*>(d_P);
    a.Pt        = static_cast<T*>(d_Pt);
    a.Uu        = static_cast<T*>(d_Uu);
    a.Iu        = static_cast<T*>(d_Iu);
    a.in_stride = (long)in_stride;
    a.n         = (long)n;
    a.n_phases  = (int)np;
    uintptr_t rows[3 * kElPhases + 3];
    int       count = 0;
    for (size_t r = 0; r < np; ++r) { // (the rows of an input that no connected output needs are not read)
        if (a.Uu) rows[count++] = reinterpret_cast<uintptr_t>(a.U + r * in_stride);
        if (a.Iu) rows[count++] = reinterpret_cast<uintptr_t>(a.I + r * in_stride);
        if (a.Pt) rows[count++] = reinterpret_cast<uintptr_t>(a.P + r * in_stride);
    }
    rows[count++] = reinterpret_cast<uintptr_t>(a.Pt);
    rows[count++] = reinterpret_cast<uintptr_t>(a.Uu);
    rows[count++] = reinterpret_cast<uintptr_t>(a.Iu);
    a.head        = std::min<long>(pick_head(rows, count, sizeof(T)), (long)n);
    const long nvec = ((long)n - a.head) / L, per_block = kElLanes * (kElItems / L);
    GR4_REQUIRE(ceil_div(nvec + 1, per_block) < (1L << 31), "unbalance: span too long for one launch");
    const unsigned grid = (unsigned)std::max<long>(ceil_div(nvec, per_block), 1L);
    if (np == 2) hipLaunchKernelGGL((unbalance_kernel<T, 2>), dim3(grid), dim3(kElLanes), 0, st, a);
    else if (np == 3) hipLaunchKernelGGL((unbalance_kernel<T, 3>), dim3(grid), dim3(kElLanes), 0, st, a);
    else hipLaunchKernelGGL((unbalance_kernel<T, 0>), dim3(grid), dim3(kElLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

} // namespace el
} // namespace gr4

using namespace gr4;

extern "C" {

size_t gr4hip_electrical_tile(void) { return (size_t)el::kElTile; }

int gr4hip_powerfactor_process(int dtype, size_t n_phases, const void* d_P, const void* d_S, size_t in_stride, void* d_power_factor, void* d_phase, size_t out_stride,
                               size_t n, gr4hip_stream_t stream) {
    GR4_REQUIRE(dtype == GR4HIP_F32 || dtype == GR4HIP_F64, "powerfactor: dtype %d (float or double)", dtype);
    GR4_REQUIRE(n_phases >= 1 && n_phases <= (size_t)el::kElPhases, "powerfactor: n_phases %zu (1 ... 16)", n_phases);
    GR4_REQUIRE(n < ((size_t)1 << 40), "powerfactor: n %zu too large", n);
    if (n == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_P && d_S, "powerfactor: null input pointer");
    GR4_REQUIRE(in_stride >= n && out_stride >= n, "powerfactor: a stride (%zu in, %zu out) smaller than the row (%zu)", in_stride, out_stride, n);
    GR4_REQUIRE(in_stride < ((size_t)1 << 40) && out_stride < ((size_t)1 << 40), "powerfactor: stride too large");
    const size_t es = dtype_size(dtype);
    const void*  ptrs[4] = {d_P, d_S, d_power_factor, d_phase};
    for (const void* p : ptrs) GR4_REQUIRE(reinterpret_cast<uintptr_t>(p) % es == 0, "powerfactor: a pointer is not aligned to its element type");
    const size_t in_span = ((n_phases - 1) * in_stride + n) * es, out_span = ((n_phases - 1) * out_stride + n) * es;
    for (const void* o : {(const void*)d_power_factor, (const void*)d_phase})
        for (const void* i : {d_P, d_S})
            GR4_REQUIRE(!o || !el::overlaps(reinterpret_cast<uintptr_t>(o), out_span, reinterpret_cast<uintptr_t>(i), in_span), "powerfactor: an output overlaps an input");
    if (!d_power_factor && !d_phase) return GR4HIP_OK; // no port connected: nothing to compute
    hipStream_t st = as_stream(stream);
    return dtype == GR4HIP_F32 ? el::launch_powerfactor<float>(n_phases, d_P, d_S, in_stride, d_power_factor, d_phase, out_stride, n, st)
                               : el::launch_powerfactor<double>(n_phases, d_P, d_S, in_stride, d_power_factor, d_phase, out_stride, n, st);
}

int gr4hip_unbalance_process(int dtype, size_t n_phases, const void* d_Urms, const void* d_Irms, const void* d_P, size_t in_stride, void* d_P_total, void* d_U_unbalance,
                             void* d_I_unbalance, size_t n, gr4hip_stream_t stream) {
    GR4_REQUIRE(dtype == GR4HIP_F32 || dtype == GR4HIP_F64, "unbalance: dtype %d (float or double)", dtype);
    GR4_REQUIRE(n_phases >= 2 && n_phases <= (size_t)el::kElPhases, "unbalance: n_phases %zu (2 ... 16)", n_phases);
    GR4_REQUIRE(n < ((size_t)1 << 40), "unbalance: n %zu too large", n);
    if (n == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_Urms && d_Irms && d_P, "unbalance: null input pointer");
    GR4_REQUIRE(in_stride >= n, "unbalance: the stride %zu is smaller than the row (%zu)", in_stride, n);
    GR4_REQUIRE(in_stride < ((size_t)1 << 40), "unbalance: stride too large");
    const size_t es = dtype_size(dtype);
    const void*  ptrs[6] = {d_Urms, d_Irms, d_P, d_P_total, d_U_unbalance, d_I_unbalance};
    for (const void* p : ptrs) GR4_REQUIRE(reinterpret_cast<uintptr_t>(p) % es == 0, "unbalance: a pointer is not aligned to its element type");
    const size_t in_span = ((n_phases - 1) * in_stride + n) * es, out_span = n * es;
    for (const void* o : {(const void*)d_P_total, (const void*)d_U_unbalance, (const void*)d_I_unbalance})
        for (const void* i : {d_Urms, d_Irms, d_P})
            GR4_REQUIRE(!o || !el::overlaps(reinterpret_cast<uintptr_t>(o), out_span, reinterpret_cast<uintptr_t>(i), in_span), "unbalance: an output overlaps an input");
    if (!d_P_total && !d_U_unbalance && !d_I_unbalance) return GR4HIP_OK;
    hipStream_t st = as_stream(stream);
    return dtype == GR4HIP_F32 ? el::launch_unbalance<float>(n_phases, d_Urms, d_Irms, d_P, in_stride, d_P_total, d_U_unbalance, d_I_unbalance, n, st)
                               : el::launch_unbalance<double>(n_phases, d_Urms, d_Irms, d_P, in_stride, d_P_total, d_U_unbalance, d_I_unbalance, n, st);
}

} // extern "C"
