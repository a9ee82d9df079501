// signal_generator.hip -- gr::basic::SignalGenerator<T> (blocks/basic/.../SignalGenerator.hpp:68-83: one SignalGeneratorCore<T>::generateSample() per sample) as a
// device source for T in {float, double, complex<float>, int16} (include/gr4hip.h "Signal generator", SIGNAL_GENERATOR.md).  The reference is sequential in three
// ways; each is evaluated here at the absolute sample index, so that the values do not depend on how a stream is cut into calls:
//   time      t += 1 / sample_rate in the compute type F (ToneGenerator.hpp:47,224-225) is piecewise linear in n: inside one binade fl(t + tick) - t is constant after
//             at most one settling step, so the host keeps a table of (n_start, mantissa, increment, scale) segments that covers 2^64 samples, and the device
//             evaluates (mantissa + (n - n_start) * increment) * scale exactly in integers (sg_build_table, sg_time);
//   noise     xoshiro256++ (Xoshiro256pp.hpp:32-66) is linear over GF(2): T^(2^k), k = 0 .. 63, as 256 x 256 bit matrices (built once on the host by repeated
//             squaring) let every lane own a run of consecutive draws.  A lane's start state is ONE matrix-vector product away from a lower lane's (doubling
//             across the lanes of a workgroup, sg_spread), the workgroups' start states come from the same doubling one level up (sg_starts_kernel);
//   Gaussian  Marsaglia's polar method (GaussianNoise.hpp:33-55): attempt k of a call is draws 2k and 2k + 1; the lanes test their attempts and count the accepted
//             ones (sg_gauss_kernel<.., false>), the counts order them, and the accepted pairs are written in order (sg_gauss_kernel<.., true>).  The stream's state
//             afterwards is the one behind the attempt that gave the last needed output.  sg_gauss_tail_kernel, queued in every call, finishes sequentially what
//             the launched attempts did not give, and exits at once when nothing is missing.
// FastSin / FastCos (ToneGenerator.hpp:216-232) are the closed form of the reference's rounded constants in float64, not its recurrence (gr4hip.h states the bound).
// Every +, -, x and / is rounded on its own, in the reference's order: contraction is off for the whole file.  sin / cos / log of F = float are evaluated in
// double on the float argument and rounded once.
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <type_traits>

#pragma clang fp contract(off)

namespace gr4 {

using u64 = unsigned long long;

constexpr int kSgLanes   = 256;
constexpr int kSgRun     = 16;                 // samples per lane: gr4hip_siggen_run
constexpr int kSgTile    = kSgLanes * kSgRun;  // samples per workgroup: gr4hip_siggen_tile
constexpr int kSgGaussJ  = 8;                  // Gaussian attempts per lane (16 draws)
constexpr int kSgGaussB  = kSgLanes * kSgGaussJ;
constexpr int kSgMatU64  = 256 * 4;            // one 256 x 256 bit matrix: column i (the image of state bit i) in 4 words
constexpr int kSgMats    = 64;
constexpr size_t kSgTabCap = 4096;             // segments (a few hundred cover 2^64 samples)

enum SgType { kConst = 0, kSin, kCos, kSquare, kSaw, kTriangle, kFastSin, kFastCos, kUniform, kTriangular, kGaussian, kSgTypes };

struct SgSeg {   // t_n = (a + (n - n0) * b) * scale for n0 <= n < the next segment's n0
    u64    n0, a, b;
    double scale;
};

struct SgState { // the handle's device-side stream state
    u64    s[4];
    double spare;      // the cached second variate (an F value)
    int    has_spare;
    int    pad;
    u64    total;      // accepted pairs the parallel Gaussian kernels delivered to this call (>= the needed number: nothing is left for the tail)
};

struct SgArgs {
    void*        out;
    u64          n, n0, k0; // samples of this call; absolute index of its first sample; samples since configure in front of it
    int          type;
    int          lane_log;  // log2 of the draws of one lane
    double       f, a, o, ph, omega, cyc0; // F values
    double       arg_p0, arg_rot, mag_p0, magpow[16]; // the phasor model: |rot|^(2^b)
    const SgSeg* tab;
    int          ntab;
    const u64*   M;
    const SgState* st;
    SgState*     stn;
    u64*         bstate;
    unsigned*    cnt;
    u64          nblk;
    u64          N, P; // Gaussian: variates this call outputs; pairs it needs from the stream
    int          c;    // a spare is carried in
};

// ---------------------------------------------------------------------------------------------- xoshiro256++ and its jumps
__host__ __device__ __forceinline__ u64 sg_rotl(u64 x, int k) { return (x << k) | (x >> (64 - k)); }
__host__ __device__ __forceinline__ u64 sg_next(u64* s) { // Xoshiro256pp.hpp:41-52
    const u64 r = sg_rotl(s[0] + s[3], 23) + s[0], t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = sg_rotl(s[3], 45);
    return r;
}
__host__ __device__ __forceinline__ void sg_matvec(const u64* __restrict__ M, const u64* s, u64* o) {
    u64 o0 = 0, o1 = 0, o2 = 0, o3 = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const u64 sw = s[w];
#pragma unroll 4
        for (int b = 0; b < 64; ++b) {
            const u64  m = 0ull - ((sw >> b) & 1ull);
            const u64* c = M + (size_t)(w * 64 + b) * 4;
            o0 ^= c[0] & m;
            o1 ^= c[1] & m;
            o2 ^= c[2] & m;
            o3 ^= c[3] & m;
        }
    }
    o[0] = o0;
    o[1] = o1;
    o[2] = o2;
    o[3] = o3;
}

static u64*           g_sg_mats = nullptr; // [64][256][4]: T^(2^k)
static std::once_flag g_sg_mats_once;
static const u64*     sg_host_mats() {
    std::call_once(g_sg_mats_once, [] {
        u64* m = new u64[(size_t)kSgMats * kSgMatU64];
        for (int i = 0; i < 256; ++i) { // T itself: every basis state stepped once
            u64 s[4] = {0, 0, 0, 0};
            s[i >> 6] = 1ull << (i & 63);
            (void)sg_next(s);
            std::memcpy(m + (size_t)i * 4, s, 32);
        }
        for (int k = 1; k < kSgMats; ++k) // T^(2^k) = (T^(2^(k-1)))^2, column by column
            for (int i = 0; i < 256; ++i) sg_matvec(m + (size_t)(k - 1) * kSgMatU64, m + (size_t)(k - 1) * kSgMatU64 + (size_t)i * 4, m + (size_t)k * kSgMatU64 + (size_t)i * 4);
        g_sg_mats = m;
    });
    return g_sg_mats;
}

static void sg_jump_host(const u64 in[4], u64 n_draws, u64 out[4]) {
    const u64* m = sg_host_mats();
    u64        s[4] = {in[0], in[1], in[2], in[3]};
    for (int k = 0; k < 64; ++k)
        if ((n_draws >> k) & 1ull) {
            u64 o[4];
            sg_matvec(m + (size_t)k * kSgMatU64, s, o);
            std::memcpy(s, o, 32);
        }
    std::memcpy(out, s, 32);
}

static void sg_seed(u64 v, u64 s[4]) { // splitmix64 (Xoshiro256pp.hpp:33-39)
    for (int i = 0; i < 4; ++i) {
        v += 0x9e3779b97f4a7c15ULL;
        u64 z = v;
        z     = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z     = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        s[i]  = z ^ (z >> 31);
    }
}

// ---------------------------------------------------------------------------------------------- the time table
// The sequence t_0 = t, t_{n+1} = fl(t_n + tick) in F from (n, t) on, as segments.  Inside the binade [2^e, 2^(e+1)) every t is a multiple of ulp = 2^(e-p+1), and
// fl(t + tick) = t + q ulp with q = tick / ulp rounded: to nearest when tick / ulp is no tie, and on a tie to the even neighbour, whose parity is the same at every
// step after the first (even + q keeps its parity).  So after one settling step the increment is constant up to and including the step that lands on 2^(e+1)
// (rounding on the finer grid below it and on the coarser grid at it agree there); the step behind that is a real addition, which starts the next segment.  Steps
// the argument does not cover (t = 0, the settling step, the last step or two below a binade's top) become segments of one sample.
template <typename F>
static int sg_build_table(F tick, u64 n, F t, std::vector<SgSeg>& tab) {
    constexpr int kP      = std::numeric_limits<F>::digits;
    constexpr int kMinExp = std::numeric_limits<F>::min_exponent - 1;
    tab.clear();
    while (tab.size() < kSgTabCap) {
        SgSeg sg{n, 0, 0, 1.0};
        int   ge = 0;
        if (t > F(0) && std::isfinite(t)) {
            ge       = std::max(std::ilogb(t), kMinExp) - (kP - 1);
            sg.a     = (u64)std::ldexp((double)t, -ge);
            sg.scale = std::ldexp(1.0, ge);
        } else if (t != F(0)) { // not finite: it stays
            sg.scale = (double)t;
            sg.a     = 1;
            tab.push_back(sg);
            return GR4HIP_OK;
        }
        const F t1 = t + tick;
        if (t1 == t) { // the stall: the reference's time stands still from here on
            tab.push_back(sg);
            return GR4HIP_OK;
        }
        bool run = false;
        if (t > F(0) && std::isfinite(t1)) {
            const F top = std::ldexp(F(1), ge + kP);
            const F t2  = t1 + tick;
            run         = std::isfinite(top) && t1 < top && t2 <= top && (t1 - t) == (t2 - t1);
            if (run) {
                const u64 room = (u64)std::ldexp((double)(top - t), -ge), inc = (u64)std::ldexp((double)(t1 - t), -ge);
                const u64 K    = room / inc; // t .. t + K inc are this segment's values
                sg.b           = inc;
                tab.push_back(sg);
                if (n + K + 1 <= n) return GR4HIP_OK; // 2^64 samples covered
                n += K + 1;
                const F tK = (F)std::ldexp((double)(sg.a + K * inc), ge);
                t          = tK + tick;
            }
        }
        if (!run) {
            tab.push_back(sg);
            if (n + 1 == 0) return GR4HIP_OK;
            n += 1;
            t = t1;
        }
    }
    set_error("signal generator: the time table needs more than %zu segments", kSgTabCap);
    return GR4HIP_RUNTIME_ERROR;
}

__host__ __device__ __forceinline__ double sg_time(const SgSeg& s, u64 n) { return (double)(s.a + (n - s.n0) * s.b) * s.scale; }

static double sg_time_host(const std::vector<SgSeg>& tab, u64 n) {
    size_t lo = 0, hi = tab.size();
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) / 2;
        if (tab[mid].n0 <= n) lo = mid;
        else hi = mid;
    }
    return sg_time(tab[lo], n);
}

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------------------- device: values
__device__ __forceinline__ float  sg_sin(float x) { return (float)sin((double)x); }
__device__ __forceinline__ float  sg_cos(float x) { return (float)cos((double)x); }
__device__ __forceinline__ float  sg_log(float x) { return (float)log((double)x); }
__device__ __forceinline__ float  sg_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double sg_sin(double x) { return sin(x); }
__device__ __forceinline__ double sg_cos(double x) { return cos(x); }
__device__ __forceinline__ double sg_log(double x) { return log(x); }
__device__ __forceinline__ double sg_sqrt(double x) { return sqrt(x); }

template <typename F>
__device__ __forceinline__ F sg_u01(u64 r) { // Xoshiro256pp.hpp:55-61
    if constexpr (std::is_same_v<F, float>) return (float)(unsigned)(r >> 40) * 0x1.0p-24f;
    else return (double)(r >> 11) * 0x1.0p-53;
}
template <typename F>
__device__ __forceinline__ F sg_um11(u64* s) { return F(2) * sg_u01<F>(sg_next(s)) - F(1); }

template <typename T>
struct SgF {
    using type = double; // SignalGeneratorCore.hpp:27-41
};
template <>
struct SgF<float2> {
    using type = float;
};

template <typename T, typename F>
__device__ __forceinline__ T sg_cast(F raw) { // SignalGeneratorCore.hpp:49-60
    if constexpr (std::is_same_v<T, short>) {
        if (raw >= F(32767)) return (short)32767;
        if (raw <= F(-32768)) return (short)-32768;
        return (short)raw;
    } else {
        return (T)raw;
    }
}

__device__ __forceinline__ int sg_find_seg(const SgSeg* __restrict__ tab, int ntab, u64 n) {
    int lo = 0, hi = ntab;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].n0 <= n) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the phasor of sample k since configure: the closed form of p0 rot^k with the reference's renormalisation every 65536 samples, in float64
__device__ __forceinline__ void sg_phasor(const SgArgs& a, u64 k, double& re, double& im) {
    double         mag = k < 65536ull ? a.mag_p0 : 1.0;
    const unsigned j   = (unsigned)(k & 0xFFFFull);
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if ((j >> b) & 1u) mag = mag * a.magpow[b];
    const double th = a.arg_p0 + (double)k * a.arg_rot;
    re = mag * cos(th);
    im = mag * sin(th);
}

// one sample of a tone (ToneGenerator.hpp:235-255; complex: :77-102) at time t, k samples after configure
template <typename T>
__device__ __forceinline__ T sg_tone(const SgArgs& a, int type, double td, u64 k) {
    using F = typename SgF<T>::type;
    constexpr bool CPLX = std::is_same_v<T, float2>;
    const F t = (F)td, A = (F)a.a, O = (F)a.o;
    F       re = F(0), im = F(0);
    switch (type) {
    case kSin:
    case kCos: {
        const F theta = (F)a.omega * t + (F)a.ph;
        const F sn = sg_sin(theta), cs = sg_cos(theta);
        if (type == kSin) {
            re = A * sn + O;
            im = -A * cs;
        } else {
            re = A * cs + O;
            im = A * sn;
        }
        break;
    }
    case kFastSin:
    case kFastCos: {
        double pr, pi;
        sg_phasor(a, k, pr, pi);
        if constexpr (CPLX) { // the model in float64 on the F constants, rounded once
            if (type == kFastSin) {
                re = (F)(a.a * pi + a.o);
                im = (F)(-a.a * pr);
            } else {
                re = (F)(a.a * pr + a.o);
                im = (F)(a.a * pi);
            }
        } else {
            re = (F)(a.a * (type == kFastSin ? pi : pr) + a.o);
        }
        break;
    }
    case kSquare:
    case kSaw:
    case kTriangle: {
        const F cycle = (F)a.f * t + (F)a.cyc0;
        if (type == kSquare) re = (cycle - floor(cycle) < F(0.5)) ? A + O : -A + O;
        else if (type == kSaw) re = A * (F(2) * (cycle - floor(cycle + F(0.5)))) + O;
        else re = A * (F(4) * fabs(cycle - floor(cycle + F(0.75)) + F(0.25)) - F(1)) + O;
        break;
    }
    default: re = A + O; break;
    }
    if constexpr (CPLX) return make_float2(re, im);
    else return sg_cast<T, F>(re);
}

template <typename F>
__device__ __forceinline__ F sg_noise_one(int type, u64* s) {
    if (type == kUniform) return sg_um11<F>(s);
    const F x = sg_u01<F>(sg_next(s)), y = sg_u01<F>(sg_next(s));
    return x + y - F(1);
}
// one sample of Uniform / Triangular noise (NoiseGenerator.hpp:112-118,157-164)
template <typename T>
__device__ __forceinline__ T sg_noise(const SgArgs& a, int type, u64* s) {
    using F = typename SgF<T>::type;
    const F A = (F)a.a, O = (F)a.o;
    if constexpr (std::is_same_v<T, float2>) {
        const F n1 = sg_noise_one<F>(type, s), n2 = sg_noise_one<F>(type, s);
        return make_float2(A * n1 + O, A * n2);
    } else {
        return sg_cast<T, F>(A * sg_noise_one<F>(type, s) + O);
    }
}

// The pending settings travel as kernel arguments: they are copied when the launch is queued, so the host images may change (or go) as soon as process returns,
// and the stores are ordered on the call's stream like everything else the handle does.
constexpr int kSgUploadSegs = 96;
struct SgUpload {
    SgSeg seg[kSgUploadSegs];
};
__global__ void sg_upload_tab_kernel(const SgUpload u, SgSeg* __restrict__ dst, int count) {
    const int i = threadIdx.x;
    if (i < count) dst[i] = u.seg[i];
}
__global__ void sg_upload_state_kernel(const SgState s, SgState* __restrict__ dst) {
    if (threadIdx.x == 0) *dst = s;
}

// doubling across the lanes: ls[0] holds the first lane's state; lane j with top bit b is T^(2^(log0 + b)) times lane j - 2^b
__device__ __forceinline__ void sg_spread(u64 (*ls)[4], const u64* __restrict__ M, int log0) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int b = 0; b < 8; ++b) {
        if (t >= (1 << b) && t < (2 << b)) {
            u64 src[4], dst[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) src[w] = ls[t - (1 << b)][w];
            sg_matvec(M + (size_t)(log0 + b) * kSgMatU64, src, dst);
#pragma unroll
            for (int w = 0; w < 4; ++w) ls[t][w] = dst[w];
        }
        __syncthreads();
    }
}

// the workgroups' start states: lane j of workgroup w serves workgroup w * 256 + j of the kernel behind it
__global__ __launch_bounds__(kSgLanes) void sg_starts_kernel(const SgArgs a) {
    __shared__ u64 ls[kSgLanes][4];
    const int t = threadIdx.x;
    const int blk_log = a.lane_log + 8;
    if (t == 0) {
        u64 s[4] = {a.st->s[0], a.st->s[1], a.st->s[2], a.st->s[3]};
        const u64 w = blockIdx.x;
        for (int i = 0; i < 32; ++i)
            if (((w >> i) & 1ull) && blk_log + 8 + i < kSgMats) {
                u64 o[4];
                sg_matvec(a.M + (size_t)(blk_log + 8 + i) * kSgMatU64, s, o);
#pragma unroll
                for (int q = 0; q < 4; ++q) s[q] = o[q];
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) ls[0][q] = s[q];
    }
    sg_spread(ls, a.M, blk_log);
    const u64 i = (u64)blockIdx.x * kSgLanes + t;
    if (i < a.nblk) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a.bstate[i * 4 + q] = ls[t][q];
    }
}

__device__ __forceinline__ int sg_pad(int i) { return i + (i >> 4); }
constexpr int kSgLds = kSgTile + (kSgTile >> 4);

// Const, the tones, Uniform and Triangular noise: every lane a run of 16 consecutive samples, staged in LDS, stored in rows of 256 consecutive elements
template <typename T, bool NOISE>
__global__ __launch_bounds__(kSgLanes) void sg_main_kernel(const SgArgs a) {
    __shared__ T   sx[kSgLds];
    __shared__ u64 ls[NOISE ? kSgLanes : 1][4];
    const int t    = threadIdx.x;
    const u64 blk0 = (u64)blockIdx.x * kSgTile;
    const u64 p0   = blk0 + (u64)t * kSgRun;
    const int m    = p0 >= a.n ? 0 : (int)min((u64)kSgRun, a.n - p0);
    u64       s[4] = {0, 0, 0, 0};
    if constexpr (NOISE) {
        if (t == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) ls[0][q] = a.bstate[(u64)blockIdx.x * 4 + q];
        }
        sg_spread(ls, a.M, a.lane_log);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = ls[t][q];
    }
    if (m > 0) {
        int seg = 0;
        if constexpr (!NOISE) seg = sg_find_seg(a.tab, a.ntab, a.n0 + p0);
        for (int j = 0; j < m; ++j) {
            T v;
            if constexpr (NOISE) {
                v = sg_noise<T>(a, a.type, s);
            } else {
                const u64 n = a.n0 + p0 + j;
                while (seg + 1 < a.ntab && a.tab[seg + 1].n0 <= n) ++seg;
                v = sg_tone<T>(a, a.type, sg_time(a.tab[seg], n), a.k0 + p0 + j);
            }
            sx[sg_pad(t * kSgRun + j)] = v;
        }
        if constexpr (NOISE) {
            if (p0 + m == a.n) { // the stream's end state, for the next call
#pragma unroll
                for (int q = 0; q < 4; ++q) a.stn->s[q] = s[q];
                a.stn->spare     = 0.0;
                a.stn->has_spare = 0;
                a.stn->pad       = 0;
                a.stn->total     = 0;
            }
        }
    }
    __syncthreads();
    T* out = static_cast<T*>(a.out);
#pragma unroll
    for (int it = 0; it < kSgRun; ++it) {
        const int i = it * kSgLanes + t;
        if (blk0 + i < a.n) out[blk0 + i] = sx[sg_pad(i)];
    }
}

// ---------------------------------------------------------------------------------------------- Gaussian
// one attempt (GaussianNoise.hpp:33-55): two draws; accepted iff 0 < s < 1
template <typename F>
__device__ __forceinline__ bool sg_attempt(u64* s, F& u, F& v, F& q) {
    u = sg_um11<F>(s);
    v = sg_um11<F>(s);
    q = u * u + v * v;
    return q < F(1) && q != F(0);
}
template <typename F>
__device__ __forceinline__ void sg_pair(F u, F v, F q, F& g1, F& g2) {
    const F f = sg_sqrt(F(-2) * sg_log(q) / q);
    g1 = u * f;
    g2 = v * f;
}
// variate `slot` of the call as a component of the output: a sample of a real T; of complex<float> the real (even slot) or imaginary part of sample slot / 2
template <typename T>
struct SgComp {
    using type = T;
};
template <>
struct SgComp<float2> {
    using type = float;
};
template <typename T>
__device__ __forceinline__ typename SgComp<T>::type sg_gauss_comp(const SgArgs& a, typename SgF<T>::type g, u64 slot) {
    using F = typename SgF<T>::type;
    if constexpr (std::is_same_v<T, float2>) {
        const F scale = F(1) / (F)1.41421356237309504880168872420969808; // 1 / sqrt2_v<F>, in F
        const F x     = g * scale;
        return (slot & 1ull) ? (F)a.a * x : (F)a.a * x + (F)a.o;
    } else {
        return sg_cast<T, F>((F)a.a * g + (F)a.o);
    }
}

// APPLY false: the accepted attempts of every workgroup's 2048.  APPLY true: the accepted pairs in order, the state behind the last needed one.
template <typename T, bool APPLY>
__global__ __launch_bounds__(kSgLanes) void sg_gauss_kernel(const SgArgs a) {
    using F  = typename SgF<T>::type;
    using Tc = typename SgComp<T>::type;
    __shared__ u64      ls[kSgLanes][4];
    __shared__ unsigned sc[kSgLanes];
    __shared__ u64      red[kSgLanes];
    __shared__ Tc       sx[APPLY ? 2 * kSgGaussB : 1];
    const int t = threadIdx.x;
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ls[0][q] = a.bstate[(u64)blockIdx.x * 4 + q];
    }
    sg_spread(ls, a.M, a.lane_log);
    u64 s0[4], s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) s0[q] = s[q] = ls[t][q];
    unsigned acc = 0; // which of the lane's attempts are accepted
    for (int j = 0; j < kSgGaussJ; ++j) {
        F u, v, q;
        if (sg_attempt<F>(s, u, v, q)) acc |= 1u << j;
    }
    const unsigned mine = __popc(acc);
    // inclusive scan of the lanes' counts
    sc[t] = mine;
    __syncthreads();
    unsigned incl = mine;
    for (int off = 1; off < kSgLanes; off <<= 1) {
        const unsigned add = t >= off ? sc[t - off] : 0u;
        __syncthreads();
        incl += add;
        sc[t] = incl;
        __syncthreads();
    }
    const unsigned blk_cnt = sc[kSgLanes - 1];
    if constexpr (!APPLY) {
        if (t == 0) a.cnt[blockIdx.x] = blk_cnt;
    } else {
        // the accepted attempts in front of this workgroup (every workgroup adds them up itself: none waits for another)
        u64 part = 0;
        for (u64 i = t; i < (u64)blockIdx.x; i += kSgLanes) part += a.cnt[i];
        red[t] = part;
        __syncthreads();
        for (int off = kSgLanes / 2; off > 0; off >>= 1) {
            if (t < off) red[t] += red[t + off];
            __syncthreads();
        }
        const u64 before = red[0];
        Tc*       outc   = static_cast<Tc*>(a.out);
        if (blockIdx.x == 0 && t == 0) {
            if (a.c && a.N > 0) outc[0] = sg_gauss_comp<T>(a, (F)a.st->spare, 0); // the carried-in spare is output 0
            if (a.P == 0) { // nothing needed from the stream: only the spare is used up
                SgState e   = *a.st;
                e.has_spare = (a.c && a.N == 0) ? 1 : 0;
                e.total     = 0;
                *a.stn      = e;
            }
        }
        unsigned  lr   = incl - mine;           // the lane's first rank inside the workgroup
        u64       rank = before + lr;           // ... and in the call
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = s0[q];
        for (int j = 0; j < kSgGaussJ; ++j) {
            F u, v, q;
            if (sg_attempt<F>(s, u, v, q)) {
                if (rank < a.P) {
                    F g1, g2;
                    sg_pair<F>(u, v, q, g1, g2);
                    const u64 slot = (u64)a.c + 2 * rank;
                    sx[2 * lr]     = sg_gauss_comp<T>(a, g1, slot);
                    sx[2 * lr + 1] = sg_gauss_comp<T>(a, g2, slot + 1);
                    if (rank == a.P - 1) { // the attempt that gave the last needed output: the stream goes on behind it
                        SgState e;
#pragma unroll
                        for (int w = 0; w < 4; ++w) e.s[w] = s[w];
                        e.has_spare = slot + 1 >= a.N ? 1 : 0; // its second variate is not part of this call
                        e.spare     = (double)g2;
                        e.pad       = 0;
                        e.total     = a.P;
                        *a.stn      = e;
                    }
                }
                ++rank;
                ++lr;
            }
        }
        if (blockIdx.x == a.nblk - 1 && t == kSgLanes - 1 && rank < a.P) { // short: the tail kernel goes on from the state behind all launched attempts
            SgState e;
#pragma unroll
            for (int w = 0; w < 4; ++w) e.s[w] = s[w];
            e.has_spare = 0;
            e.spare     = 0.0;
            e.pad       = 0;
            e.total     = rank;
            *a.stn      = e;
        }
        __syncthreads();
        const u64 slot0 = (u64)a.c + 2 * before;
        for (unsigned i = t; i < 2 * blk_cnt; i += kSgLanes) {
            const u64 slot = slot0 + i;
            if (slot < a.N && before + (i >> 1) < a.P) outc[slot] = sx[i];
        }
    }
}

// what the launched attempts did not give, sequentially; nothing to do when they gave all
template <typename T>
__global__ void sg_gauss_tail_kernel(const SgArgs a) {
    using F  = typename SgF<T>::type;
    using Tc = typename SgComp<T>::type;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    u64 rank = a.stn->total;
    if (rank >= a.P) return;
    u64 s[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) s[w] = a.stn->s[w];
    Tc* outc = static_cast<Tc*>(a.out);
    F   g1 = F(0), g2 = F(0);
    u64 slot = 0;
    while (rank < a.P) {
        F u, v, q;
        if (!sg_attempt<F>(s, u, v, q)) continue;
        sg_pair<F>(u, v, q, g1, g2);
        slot = (u64)a.c + 2 * rank;
        if (slot < a.N) outc[slot] = sg_gauss_comp<T>(a, g1, slot);
        if (slot + 1 < a.N) outc[slot + 1] = sg_gauss_comp<T>(a, g2, slot + 1);
        ++rank;
    }
    SgState e;
#pragma unroll
    for (int w = 0; w < 4; ++w) e.s[w] = s[w];
    e.has_spare = slot + 1 >= a.N ? 1 : 0;
    e.spare     = (double)g2;
    e.pad       = 0;
    e.total     = a.P;
    *a.stn      = e;
}
#endif // __HIPCC__

// ---------------------------------------------------------------------------------------------- host
static bool sg_dtype_f32(int dtype) { return dtype == GR4HIP_C32; } // F = float for complex<float> only

static int sg_check(const gr4hip_siggen_params* p) {
    GR4_REQUIRE(p, "signal generator: null params");
    GR4_REQUIRE(p->signal_type >= 0 && p->signal_type < kSgTypes, "signal generator: unknown signal type %d", p->signal_type);
    GR4_REQUIRE(p->dtype >= 0 && p->dtype <= GR4HIP_UF64, "signal generator: unknown dtype %d", p->dtype);
    GR4_REQUIRE(std::isfinite(p->sample_rate) && p->sample_rate > 0.f, "signal generator: sample_rate %g (finite, > 0)", (double)p->sample_rate);
    GR4_REQUIRE(std::isfinite(p->frequency) && std::isfinite(p->amplitude) && std::isfinite(p->offset) && std::isfinite(p->phase),
                "signal generator: frequency %g, amplitude %g, offset %g, phase %g must be finite", (double)p->frequency, (double)p->amplitude, (double)p->offset,
                (double)p->phase);
    if (p->dtype != GR4HIP_F32 && p->dtype != GR4HIP_F64 && p->dtype != GR4HIP_C32 && p->dtype != GR4HIP_I16) {
        set_error("signal generator: dtype %d (float, double, complex<float> and int16 are implemented)", p->dtype);
        return GR4HIP_UNSUPPORTED;
    }
    if (sg_dtype_f32(p->dtype)) GR4_REQUIRE(std::isfinite(1.0f / p->sample_rate), "signal generator: 1 / sample_rate is not finite in float");
    return GR4HIP_OK;
}

} // namespace gr4

using namespace gr4;

struct gr4hip_siggen {
    gr4hip_siggen_params p{};
    u64                  n_abs = 0, n_cfg = 0; // samples since reset / since configure
    int                  has_spare = 0;        // (its value is on the device; whether there is one follows from the sample count)
    std::vector<SgSeg>   tab;                  // the time table's host image (it reaches the device as kernel arguments)
    SgState              st_host{};
    bool                 tab_dirty = true, seed_pending = true;
    int                  cur = 0;
    const u64*           d_mats = nullptr;
    DeviceBuffer         d_state[2], d_tab, d_bstate, d_cnt;
    SgArgs               a{}; // the settings as the kernels take them
};

static std::mutex g_sg_dev_mutex;
static u64*       g_sg_dev_mats[PerDevice::kMax] = {};

static int sg_device_mats(const u64** out) {
    int dev = 0;
    GR4_HIP_TRY(hipGetDevice(&dev));
    GR4_REQUIRE(dev >= 0 && dev < PerDevice::kMax, "signal generator: device index %d", dev);
    std::lock_guard<std::mutex> lock(g_sg_dev_mutex);
    if (!g_sg_dev_mats[dev]) { // once per device, for the life of the process
        void*        p     = nullptr;
        const size_t bytes = (size_t)kSgMats * kSgMatU64 * sizeof(u64);
        GR4_HIP_TRY(hipMalloc(&p, bytes));
        if (upload_fresh(p, sg_host_mats(), bytes) != hipSuccess) {
            hip_quiet(hipFree(p));
            set_error("signal generator: uploading the jump matrices failed");
            return GR4HIP_RUNTIME_ERROR;
        }
        g_sg_dev_mats[dev] = static_cast<u64*>(p);
    }
    *out = g_sg_dev_mats[dev];
    return GR4HIP_OK;
}

template <typename F>
static int sg_retime(gr4hip_siggen_t* h, bool from_zero) {
    const F tick = F(1) / static_cast<F>(h->p.sample_rate); // ToneGenerator.hpp:47
    const F t    = from_zero || h->tab.empty() ? F(0) : (F)sg_time_host(h->tab, h->n_abs);
    std::vector<SgSeg> tab;
    const int          rc = sg_build_table<F>(tick, h->n_abs, t, tab);
    if (rc) return rc;
    h->tab.swap(tab);
    h->tab_dirty = true;
    return GR4HIP_OK;
}

// configure (SignalGeneratorCore.hpp:88-108, ToneGenerator.hpp:40-60, initPhasor :204-214, NoiseGenerator.hpp:78): the constants in F, the noise re-seeded, the
// spare dropped, the phasor and its count from the start; the time base keeps running
template <typename F>
static int sg_configure(gr4hip_siggen_t* h, const gr4hip_siggen_params& p, bool retime, bool from_zero) {
    h->p = p;
    if (retime) {
        const int rc = sg_retime<F>(h, from_zero);
        if (rc) return rc;
    }
    constexpr F pi2 = F(2) * F(3.14159265358979323846264338327950288);
    const F     f = static_cast<F>(p.frequency), ph = static_cast<F>(p.phase), tick = F(1) / static_cast<F>(p.sample_rate);
    SgArgs&     a = h->a;
    a.type = p.signal_type;
    if (a.type <= kFastCos && f <= F(0)) a.type = kConst; // ToneGenerator.hpp:48
    a.f     = (double)f;
    a.a     = (double)static_cast<F>(p.amplitude);
    a.o     = (double)static_cast<F>(p.offset);
    a.ph    = (double)ph;
    a.omega = (double)(pi2 * f);
    a.cyc0  = (double)(ph / pi2);
    const F  rr = std::cos(pi2 * f * tick), ri = std::sin(pi2 * f * tick), pr = std::cos(ph), pi = std::sin(ph);
    a.arg_rot = std::atan2((double)ri, (double)rr);
    a.arg_p0  = std::atan2((double)pi, (double)pr);
    a.mag_p0  = std::hypot((double)pr, (double)pi);
    double m  = std::hypot((double)rr, (double)ri);
    for (int b = 0; b < 16; ++b) {
        a.magpow[b] = m;
        m           = m * m;
    }
    h->n_cfg = 0;
    sg_seed(p.seed, h->st_host.s);
    h->st_host.spare     = 0.0;
    h->st_host.has_spare = 0;
    h->st_host.pad       = 0;
    h->st_host.total     = 0;
    h->has_spare         = 0;
    h->seed_pending      = true;
    return GR4HIP_OK;
}

static int sg_configure_d(gr4hip_siggen_t* h, const gr4hip_siggen_params& p, bool retime, bool from_zero) {
    return sg_dtype_f32(p.dtype) ? sg_configure<float>(h, p, retime, from_zero) : sg_configure<double>(h, p, retime, from_zero);
}

template <typename T>
static int sg_launch(gr4hip_siggen_t* h, SgArgs& a, hipStream_t st) {
    constexpr bool CPLX = std::is_same_v<T, float2>;
    const int      type = a.type;
    if (type < kUniform) {
        a.nblk = ceil_div(a.n, (u64)kSgTile);
        hipLaunchKernelGGL((sg_main_kernel<T, false>), dim3((unsigned)a.nblk), dim3(kSgLanes), 0, st, a);
        GR4_LAUNCH_CHECK();
        return GR4HIP_OK;
    }
    int rc;
    if (type != kGaussian) {
        const int ld = (type == kTriangular ? 1 : 0) + (CPLX ? 1 : 0); // draws per sample: 1, 2 or 4
        a.lane_log   = 4 + ld;
        a.nblk       = ceil_div(a.n, (u64)kSgTile);
        if ((rc = h->d_bstate.ensure(std::max<size_t>(a.nblk * 32, 1 << 16)))) return rc;
        a.bstate = static_cast<u64*>(h->d_bstate.ptr);
        hipLaunchKernelGGL(sg_starts_kernel, dim3((unsigned)ceil_div(a.nblk, (u64)kSgLanes)), dim3(kSgLanes), 0, st, a);
        GR4_LAUNCH_CHECK();
        hipLaunchKernelGGL((sg_main_kernel<T, true>), dim3((unsigned)a.nblk), dim3(kSgLanes), 0, st, a);
        GR4_LAUNCH_CHECK();
        h->cur ^= 1;
        return GR4HIP_OK;
    }
    // Gaussian: N variates, the first of them a carried-in spare; P pairs from the stream
    a.N = CPLX ? 2 * a.n : a.n;
    a.c = h->has_spare;
    a.P = a.N > (u64)a.c ? (a.N - a.c + 1) / 2 : 0;
    // attempts to launch: the acceptance is pi / 4 with a standard deviation of 0.41 sqrt(attempts); eight of those and a floor on top.  Correctness does not rest
    // on it (the tail kernel); GR4HIP_SIGGEN_GAUSS_PERMILLE sets the attempts per 1000 needed pairs instead
    const int permille = dev_switch(kDevSiggenGaussPermille);
    u64       att;
    if (permille > 0) att = std::max<u64>(1, (a.P * (u64)permille + 999) / 1000);
    else att = (u64)std::ceil((double)a.P * (4.0 / 3.14159265358979323846)) + (u64)(4.0 * std::sqrt((double)a.P)) + 64;
    a.lane_log = 4;
    a.nblk     = ceil_div(att, (u64)kSgGaussB);
    if ((rc = h->d_bstate.ensure(std::max<size_t>(a.nblk * 32, 1 << 16))) || (rc = h->d_cnt.ensure(std::max<size_t>(a.nblk * 4, 1 << 14)))) return rc;
    a.bstate = static_cast<u64*>(h->d_bstate.ptr);
    a.cnt    = static_cast<unsigned*>(h->d_cnt.ptr);
    hipLaunchKernelGGL(sg_starts_kernel, dim3((unsigned)ceil_div(a.nblk, (u64)kSgLanes)), dim3(kSgLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL((sg_gauss_kernel<T, false>), dim3((unsigned)a.nblk), dim3(kSgLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL((sg_gauss_kernel<T, true>), dim3((unsigned)a.nblk), dim3(kSgLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_gauss_tail_kernel<T>, dim3(1), dim3(64), 0, st, a);
    GR4_LAUNCH_CHECK();
    h->has_spare = (a.N > (u64)a.c) ? (int)((a.N - a.c) & 1ull) : (a.N == 0 ? a.c : 0);
    h->cur ^= 1;
    return GR4HIP_OK;
}

extern "C" {

size_t gr4hip_siggen_run(void) { return (size_t)kSgRun; }

size_t gr4hip_siggen_tile(void) { return (size_t)kSgTile; }

int gr4hip_siggen_check(const gr4hip_siggen_params* p) { return sg_check(p); }

int gr4hip_siggen_jump_host(const unsigned long long in[4], unsigned long long n_draws, unsigned long long out[4]) {
    GR4_REQUIRE(in && out, "signal generator: null state");
    sg_jump_host(in, n_draws, out);
    return GR4HIP_OK;
}

int gr4hip_siggen_time_host(int dtype, float sample_rate, unsigned long long n0, size_t count, double* t_out) {
    gr4hip_siggen_params p{dtype, 0, sample_rate, 1.f, 1.f, 0.f, 0.f, 0};
    int                  rc = sg_check(&p);
    if (rc) return rc;
    GR4_REQUIRE(count == 0 || t_out, "signal generator: null output");
    std::vector<SgSeg> tab;
    rc = sg_dtype_f32(dtype) ? sg_build_table<float>(1.0f / sample_rate, 0, 0.f, tab) : sg_build_table<double>(1.0 / (double)sample_rate, 0, 0.0, tab);
    if (rc) return rc;
    for (size_t i = 0; i < count; ++i) t_out[i] = sg_time_host(tab, n0 + i);
    return GR4HIP_OK;
}

int gr4hip_siggen_create(gr4hip_siggen_t** out, const gr4hip_siggen_params* p) {
    GR4_REQUIRE(out, "signal generator: null output handle");
    int rc = sg_check(p); // (validated before anything is allocated)
    if (rc) return rc;
    auto* h = new (std::nothrow) gr4hip_siggen();
    GR4_REQUIRE(h, "out of host memory");
    rc = sg_device_mats(&h->d_mats);
    for (auto& b : h->d_state)
        if (!rc) rc = b.ensure(sizeof(SgState));
    if (!rc) rc = h->d_tab.ensure(kSgTabCap * sizeof(SgSeg));
    if (!rc) rc = sg_configure_d(h, *p, true, true); // start(): configure + reset
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return GR4HIP_OK;
}

int gr4hip_siggen_configure(gr4hip_siggen_t* h, const gr4hip_siggen_params* p) {
    GR4_REQUIRE(h, "signal generator: null handle");
    const int rc = sg_check(p);
    if (rc) return rc;
    GR4_REQUIRE(p->dtype == h->p.dtype, "signal generator: the sample type is fixed at create (%d, not %d)", h->p.dtype, p->dtype);
    return sg_configure_d(h, *p, p->sample_rate != h->p.sample_rate, false);
}

int gr4hip_siggen_reset(gr4hip_siggen_t* h) {
    GR4_REQUIRE(h, "signal generator: null handle");
    h->n_abs = 0;
    return sg_configure_d(h, h->p, true, true);
}

void gr4hip_siggen_destroy(gr4hip_siggen_t* h) { delete h; }

int gr4hip_siggen_process(gr4hip_siggen_t* h, void* d_out, size_t n, gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "signal generator: null handle");
    if (n == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_out, "signal generator: null output pointer");
    GR4_REQUIRE(n <= ((size_t)1 << 40), "signal generator: n %zu exceeds 2^40 (a longer stream goes in several calls)", n);
    const size_t esz = dtype_size(h->p.dtype), align = h->p.dtype == GR4HIP_C32 ? 4 : esz;
    GR4_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & (align - 1)) == 0, "signal generator: the output is not aligned to its sample type");
    hipStream_t st = as_stream(stream);
    if (h->tab_dirty) { // the pending settings, on this stream in front of this call's launches (the stream rule)
        GR4_REQUIRE(h->tab.size() <= kSgTabCap, "signal generator: time table of %zu segments", h->tab.size());
        for (size_t at = 0; at < h->tab.size(); at += kSgUploadSegs) {
            SgUpload  u{};
            const int cnt = (int)std::min<size_t>(kSgUploadSegs, h->tab.size() - at);
            std::copy_n(h->tab.begin() + (std::ptrdiff_t)at, cnt, u.seg);
            hipLaunchKernelGGL(sg_upload_tab_kernel, dim3(1), dim3(kSgUploadSegs), 0, st, u, static_cast<SgSeg*>(h->d_tab.ptr) + at, cnt);
            GR4_LAUNCH_CHECK();
        }
        h->tab_dirty = false;
    }
    if (h->seed_pending) {
        hipLaunchKernelGGL(sg_upload_state_kernel, dim3(1), dim3(64), 0, st, h->st_host, static_cast<SgState*>(h->d_state[h->cur].ptr));
        GR4_LAUNCH_CHECK();
        h->seed_pending = false;
    }
    SgArgs a = h->a;
    a.out    = d_out;
    a.n      = n;
    a.n0     = h->n_abs;
    a.k0     = h->n_cfg;
    a.tab    = static_cast<const SgSeg*>(h->d_tab.ptr);
    a.ntab   = (int)h->tab.size();
    a.M      = h->d_mats;
    a.st     = static_cast<const SgState*>(h->d_state[h->cur].ptr);
    a.stn    = static_cast<SgState*>(h->d_state[h->cur ^ 1].ptr);
    int rc;
    switch (h->p.dtype) {
    case GR4HIP_F32: rc = sg_launch<float>(h, a, st); break;
    case GR4HIP_F64: rc = sg_launch<double>(h, a, st); break;
    case GR4HIP_I16: rc = sg_launch<short>(h, a, st); break;
    default: rc = sg_launch<float2>(h, a, st); break;
    }
    if (rc) return rc;
    if (a.type <= kFastCos) h->n_abs += n; // the time base advances with the tones only (SignalGeneratorCore.hpp:110-135)
    h->n_cfg += n;
    return GR4HIP_OK;
}

} // extern "C"
