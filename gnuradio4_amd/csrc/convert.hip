// convert.hip -- the type-converter blocks (blocks/basic/.../ConverterBlocks.hpp:13-277) as one streaming kernel template, and the gr4hip_convert_* entry points.
//
// Every kind is a functor over ITEMS: what one processOne call takes from each input port and gives to each output port -- one element per port, except for the
// interleaved port of ComplexToInterleaved / InterleavedToComplex, which carries two.  The kernel is HBM-bound: a lane moves L consecutive items, L chosen so that
// the port with the WIDEST item moves 16 bytes per access (1 B -> 8 B: two items, a 2-byte load and a 16-byte store); cheap kinds keep several such vectors in
// flight per lane.  The two-port kinds read or write both streams from the same registers: each stream is contiguous across the lanes of a wave by itself.
// A ring span starts at any element and the spans of the ports advance independently, so the launch cuts [0, n) into an element-wise head, a body of L items
// per lane, and an element-wise tail, with the head chosen so that the widest accesses of the body are aligned; a port whose body accesses stay unaligned (its
// misalignment disagrees with the others', or an interleaved stream starts at an odd element) moves its L items element by element while the other ports keep
// their wide accesses.  Programs of per-sample neighbours ride in the launch as load / store hooks (ewise.hpp), on the values in registers.
#include "ewise.hpp"
#include "../host/include/gr4/converter_ops.hpp"

#include <cmath>
#include <limits>
#include <type_traits>

namespace gr4 {
namespace cv {

// ---- the arithmetic: the integer and cast rules are the host mirror blocks' own (one header for both domains)
using gr4::converter_ops::abs_int;
using gr4::converter_ops::cast;
using gr4::converter_ops::mul;

// complex<float>: float64 on the float arguments, one rounding (SIGNAL_GENERATOR.md's convention); x^2 + y^2 cannot overflow there
__device__ __forceinline__ float abs_c(float2 z) {
#pragma clang fp contract(off)
    if (__builtin_isinf(z.x) || __builtin_isinf(z.y)) return __builtin_inff(); // hypot: an infinite component wins over a NaN
    const double x = z.x, y = z.y;
    return (float)::sqrt(x * x + y * y);
}
__device__ __forceinline__ double abs_c(double2 z) { return ::hypot(z.x, z.y); }
__device__ __forceinline__ float  arg_c(float2 z) { return (float)::atan2((double)z.y, (double)z.x); }
__device__ __forceinline__ double arg_c(double2 z) { return ::atan2(z.y, z.x); }
__device__ __forceinline__ float2 polar_c(float r, float t) {
#pragma clang fp contract(off)
    double s, c;
    ::sincos((double)t, &s, &c);
    return make_float2((float)((double)r * c), (float)((double)r * s));
}
__device__ __forceinline__ double2 polar_c(double r, double t) {
#pragma clang fp contract(off)
    double s, c;
    ::sincos(t, &s, &c);
    return make_double2(r * c, r * s);
}

template <typename T> struct BaseOf { using type = T; };
template <> struct BaseOf<float2> { using type = float; };
template <> struct BaseOf<double2> { using type = double; };
template <typename F> struct CplxOf;
template <> struct CplxOf<float> { using type = float2; };
template <> struct CplxOf<double> { using type = double2; };
template <typename F> __device__ __forceinline__ typename CplxOf<F>::type make_c(F re, F im) {
    typename CplxOf<F>::type z;
    z.x = re;
    z.y = im;
    return z;
}

// ---- the kinds: TI / TO element types of the ports, NI / NO ports, EI / EO elements per item and port; apply() converts ONE item (in[p * EI + e], out[q * EO + e])
template <typename TI_, int NI_, int EI_, typename TO_, int NO_, int EO_, bool HEAVY_ = false>
struct Shape {
    using TI = TI_;
    using TO = TO_;
    static constexpr int  NI = NI_, EI = EI_, NO = NO_, EO = EO_;
    static constexpr bool HEAVY = HEAVY_; // a transcendental per item: one vector per lane (the others keep several in flight)
};
template <typename T, typename R>
struct OpScale : Shape<T, 1, 1, R, 1, 1> { // (:25-31, :51-58)
    static __device__ __forceinline__ void apply(const T* in, R* out, unsigned long long scale_bits) {
        T s;
        __builtin_memcpy(&s, &scale_bits, sizeof(T));
        out[0] = cast<R>(mul<T>(in[0], s));
    }
};
template <typename T>
struct OpAbs : Shape<T, 1, 1, typename BaseOf<T>::type, 1, 1, ew_is_complex<T>::value> { // (:73-79)
    static __device__ __forceinline__ void apply(const T* in, typename BaseOf<T>::type* out, unsigned long long) {
        if constexpr (ew_is_complex<T>::value) out[0] = abs_c(in[0]);
        else if constexpr (std::is_same_v<T, float>) out[0] = __builtin_fabsf(in[0]);
        else if constexpr (std::is_same_v<T, double>) out[0] = __builtin_fabs(in[0]);
        else out[0] = abs_int<T>(in[0]);
    }
};
template <typename T, int WHICH> // 0: Real (:110), 1: Imag (:95), 2: Arg (:125)
struct OpPart : Shape<T, 1, 1, typename BaseOf<T>::type, 1, 1, WHICH == 2> {
    static __device__ __forceinline__ void apply(const T* in, typename BaseOf<T>::type* out, unsigned long long) {
        if constexpr (WHICH == 0) out[0] = in[0].x;
        else if constexpr (WHICH == 1) out[0] = in[0].y;
        else out[0] = arg_c(in[0]);
    }
};
template <typename F, bool TO_DEG> // (:140-142, :157-159): a true division, then a multiplication
struct OpAngle : Shape<F, 1, 1, F, 1, 1> {
    static __device__ __forceinline__ void apply(const F* in, F* out, unsigned long long) {
#pragma clang fp contract(off)
        constexpr F pi = (F)3.141592653589793238462643383279502884L; // std::numbers::pi_v<F>
        out[0] = TO_DEG ? (in[0] / pi) * F(180) : (in[0] / F(180)) * pi;
    }
};
template <typename T, bool POLAR> // ToRealImag (:175-177), ToMagPhase (:210-212)
struct OpSplit : Shape<T, 1, 1, typename BaseOf<T>::type, 2, 1, POLAR> {
    static __device__ __forceinline__ void apply(const T* in, typename BaseOf<T>::type* out, unsigned long long) {
        out[0] = POLAR ? abs_c(in[0]) : in[0].x;
        out[1] = POLAR ? arg_c(in[0]) : in[0].y;
    }
};
template <typename F, bool POLAR> // RealImagToComplex (:192-194), MagPhaseToComplex (:228-230)
struct OpJoin : Shape<F, 2, 1, typename CplxOf<F>::type, 1, 1, POLAR> {
    static __device__ __forceinline__ void apply(const F* in, typename CplxOf<F>::type* out, unsigned long long) {
        if constexpr (POLAR) out[0] = polar_c(in[0], in[1]);
        else out[0] = make_c<F>(in[0], in[1]);
    }
};
template <typename T, typename R> // (:247-253)
struct OpC2I : Shape<T, 1, 1, R, 1, 2> {
    static __device__ __forceinline__ void apply(const T* in, R* out, unsigned long long) {
        out[0] = cast<R>(in[0].x);
        out[1] = cast<R>(in[0].y);
    }
};
template <typename T, typename R> // (:271-276)
struct OpI2C : Shape<T, 1, 2, R, 1, 1> {
    static __device__ __forceinline__ void apply(const T* in, R* out, unsigned long long) {
        using F = typename BaseOf<R>::type;
        out[0]  = make_c<F>((F)in[0], (F)in[1]);
    }
};

// ---- the kernel
template <class Op> constexpr int item_bytes_max() {
    constexpr int a = (int)sizeof(typename Op::TI) * Op::EI, b = (int)sizeof(typename Op::TO) * Op::EO;
    return a > b ? a : b;
}
template <class Op> constexpr int lane_items() { return 16 / item_bytes_max<Op>(); }                                      // L: the widest port moves 16 bytes per access
template <class Op> constexpr int lane_slabs() { return Op::HEAVY ? 1 : lane_items<Op>() >= 8 ? 1 : lane_items<Op>() >= 4 ? 2 : 4; } // vectors of L items a lane holds

template <int BYTES> struct VecB;
template <> struct VecB<16> { typedef unsigned int type __attribute__((ext_vector_type(4))); };
template <> struct VecB<8> { typedef unsigned int type __attribute__((ext_vector_type(2))); };
template <> struct VecB<4> { typedef unsigned int type; };
template <> struct VecB<2> { typedef unsigned short type; };
template <> struct VecB<1> { typedef unsigned char type; };
template <typename T, int N> union CvVec {
    typename VecB<(int)sizeof(T) * N>::type u;
    T                                        e[N];
};

template <class Op>
struct CvArgs {
    const typename Op::TI* in[Op::NI];
    typename Op::TO*       out[Op::NO];
    long                   n, head, nvec; // items; [head, head + nvec L) is the body: L items per lane and access
    unsigned               unaligned;     // bit p: input p, bit NI + q: output q -- the port's body accesses are not aligned to their width: element by element there
    unsigned long long     scale_bits;
    EwiseHook              pre, post;
};

// L items from item i0 on: VEC -- one aligned access of L * (item bytes) per port; otherwise element by element (L == 1)
template <class Op, int L, bool VEC>
__device__ __forceinline__ void cv_load(const CvArgs<Op>& a, long i0, typename Op::TI (&x)[Op::NI][L * Op::EI]) {
    using TI = typename Op::TI;
    constexpr int NE = L * Op::EI;
#pragma unroll
    for (int p = 0; p < Op::NI; ++p) {
        const TI* src = a.in[p] + i0 * Op::EI;
        if (VEC && !((a.unaligned >> p) & 1u)) { // (uniform)
            CvVec<TI, NE> v;
            v.u = __builtin_nontemporal_load(reinterpret_cast<const typename VecB<(int)sizeof(TI) * NE>::type*>(src));
#pragma unroll
            for (int e = 0; e < NE; ++e) x[p][e] = v.e[e];
        } else {
#pragma unroll
            for (int e = 0; e < NE; ++e) x[p][e] = src[e];
        }
    }
}
template <class Op, int L>
__device__ __forceinline__ void cv_compute(const CvArgs<Op>& a, long i0, typename Op::TI (&x)[Op::NI][L * Op::EI], typename Op::TO (&y)[Op::NO][L * Op::EO]) {
    using TI = typename Op::TI;
    using TO = typename Op::TO;
    if constexpr (Op::NI == 1) ewise_apply<TI, L * Op::EI>(x[0], a.pre.ops, a.pre.n_ops, a.pre.has_div, [&](int j) { return a.pre.pos + i0 + j / Op::EI; });
#pragma unroll
    for (int l = 0; l < L; ++l) {
        TI in[Op::NI * Op::EI];
        TO out[Op::NO * Op::EO];
#pragma unroll
        for (int p = 0; p < Op::NI; ++p)
#pragma unroll
            for (int e = 0; e < Op::EI; ++e) in[p * Op::EI + e] = x[p][l * Op::EI + e];
        Op::apply(in, out, a.scale_bits);
#pragma unroll
        for (int q = 0; q < Op::NO; ++q)
#pragma unroll
            for (int e = 0; e < Op::EO; ++e) y[q][l * Op::EO + e] = out[q * Op::EO + e];
    }
    if constexpr (Op::NO == 1) ewise_apply<TO, L * Op::EO>(y[0], a.post.ops, a.post.n_ops, a.post.has_div, [&](int j) { return a.post.pos + i0 + j / Op::EO; });
}
template <class Op, int L, bool VEC>
__device__ __forceinline__ void cv_store(const CvArgs<Op>& a, long i0, const typename Op::TO (&y)[Op::NO][L * Op::EO]) {
    using TO = typename Op::TO;
    constexpr int NE = L * Op::EO;
#pragma unroll
    for (int q = 0; q < Op::NO; ++q) {
        if (!a.out[q]) continue; // an unconnected port (uniform)
        TO* dst = a.out[q] + i0 * Op::EO;
        if (VEC && !((a.unaligned >> (Op::NI + q)) & 1u)) { // (uniform)
            CvVec<TO, NE> v;
#pragma unroll
            for (int e = 0; e < NE; ++e) v.e[e] = y[q][e];
            __builtin_nontemporal_store(v.u, reinterpret_cast<typename VecB<(int)sizeof(TO) * NE>::type*>(dst));
        } else {
#pragma unroll
            for (int e = 0; e < NE; ++e) dst[e] = y[q][e];
        }
    }
}

template <class Op>
__global__ __launch_bounds__(256) void convert_kernel(const CvArgs<Op> a) {
    using TI = typename Op::TI;
    using TO = typename Op::TO;
    constexpr int L = lane_items<Op>(), SL = lane_slabs<Op>();
    const long    v0 = (long)blockIdx.x * (256 * SL) + threadIdx.x;
    if (v0 < a.nvec) { // all loads of the lane first: SL accesses in flight per port
        TI x[SL][Op::NI][L * Op::EI];
        TO y[SL][Op::NO][L * Op::EO];
#pragma unroll
        for (int s = 0; s < SL; ++s) {
            const long v = v0 + (long)s * 256;
            if (v < a.nvec) cv_load<Op, L, true>(a, a.head + v * L, x[s]);
            else
#pragma unroll
                for (int p = 0; p < Op::NI; ++p)
#pragma unroll
                    for (int e = 0; e < L * Op::EI; ++e) x[s][p][e] = TI{};
        }
#pragma unroll
        for (int s = 0; s < SL; ++s) cv_compute<Op, L>(a, a.head + (v0 + (long)s * 256) * L, x[s], y[s]);
#pragma unroll
        for (int s = 0; s < SL; ++s) {
            const long v = v0 + (long)s * 256;
            if (v < a.nvec) cv_store<Op, L, true>(a, a.head + v * L, y[s]);
        }
    }
    const long body_end = a.head + a.nvec * L, nscalar = a.head + (a.n - body_end);
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < nscalar; j += (long)gridDim.x * blockDim.x) { // head and tail items
        const long i = j < a.head ? j : body_end + (j - a.head);
        TI         x[Op::NI][Op::EI];
        TO         y[Op::NO][Op::EO];
        cv_load<Op, 1, false>(a, i, x);
        cv_compute<Op, 1>(a, i, x, y);
        cv_store<Op, 1, false>(a, i, y);
    }
}

} // namespace cv
} // namespace gr4

using namespace gr4;

struct gr4hip_convert {
    gr4hip_convert_params p{};
    unsigned long long    scale_bits = 0; // the scale as in_dtype
    long                  pos        = 0; // items since create / reset
    gr4hip_ewise*         pre        = nullptr;
    gr4hip_ewise*         post       = nullptr;
    std::vector<gr4hip_ewise*> retired;      // programs a set_* call took off: their device copies are freed by the next process call (the stream rule) or with the handle
    void drop_retired() { for (auto* e : retired) delete e; retired.clear(); }
    ~gr4hip_convert() { delete pre; delete post; drop_retired(); }
};

namespace gr4 {
namespace cv {

template <typename T> struct Tag { using type = T; };

template <typename F>
static int with_arith(int dtype, F&& f) {
    switch (dtype) {
    case GR4HIP_U8: return f(Tag<uint8_t>{});
    case GR4HIP_U16: return f(Tag<uint16_t>{});
    case GR4HIP_U32: return f(Tag<uint32_t>{});
    case GR4HIP_U64: return f(Tag<uint64_t>{});
    case GR4HIP_I8: return f(Tag<int8_t>{});
    case GR4HIP_I16: return f(Tag<int16_t>{});
    case GR4HIP_I32: return f(Tag<int32_t>{});
    case GR4HIP_I64: return f(Tag<int64_t>{});
    case GR4HIP_F32: return f(Tag<float>{});
    case GR4HIP_F64: return f(Tag<double>{});
    default: return GR4HIP_INVALID_ARGUMENT;
    }
}
template <typename F>
static int with_interleavable(int dtype, F&& f) {
    switch (dtype) {
    case GR4HIP_I8: return f(Tag<int8_t>{});
    case GR4HIP_I16: return f(Tag<int16_t>{});
    case GR4HIP_F32: return f(Tag<float>{});
    case GR4HIP_F64: return f(Tag<double>{});
    default: return GR4HIP_INVALID_ARGUMENT;
    }
}
template <typename F>
static int with_float(int dtype, F&& f) { // F32 / C32 -> float, F64 / C64 -> double
    switch (dtype) {
    case GR4HIP_F32: case GR4HIP_C32: return f(Tag<float>{});
    case GR4HIP_F64: case GR4HIP_C64: return f(Tag<double>{});
    default: return GR4HIP_INVALID_ARGUMENT;
    }
}

static bool is_arith(int d) { return d >= GR4HIP_U8 && d <= GR4HIP_F64; }
static bool is_float(int d) { return d == GR4HIP_F32 || d == GR4HIP_F64; }
static bool is_cplx(int d) { return d == GR4HIP_C32 || d == GR4HIP_C64; }
static bool is_interleavable(int d) { return is_float(d) || d == GR4HIP_I8 || d == GR4HIP_I16; }
static int  base_of(int d) { return d == GR4HIP_C32 ? GR4HIP_F32 : d == GR4HIP_C64 ? GR4HIP_F64 : d; }
static int  cplx_of(int d) { return d == GR4HIP_F32 ? GR4HIP_C32 : GR4HIP_C64; }

// the block's R for the kinds whose output type follows from T (-1: the kind has a second type parameter, -2: T is excluded)
static int result_dtype(int kind, int in) {
    switch (kind) {
    case GR4HIP_CONVERT: case GR4HIP_SCALING_CONVERT: return is_arith(in) ? -1 : -2;
    case GR4HIP_CONVERT_ABS: return is_arith(in) || is_cplx(in) ? base_of(in) : -2;
    case GR4HIP_CONVERT_REAL: case GR4HIP_CONVERT_IMAG: case GR4HIP_CONVERT_ARG: case GR4HIP_TO_REAL_IMAG: case GR4HIP_TO_MAG_PHASE: return is_cplx(in) ? base_of(in) : -2;
    case GR4HIP_RADIANS_TO_DEGREE: case GR4HIP_DEGREE_TO_RADIANS: return is_float(in) ? in : -2;
    case GR4HIP_REAL_IMAG_TO_COMPLEX: case GR4HIP_MAG_PHASE_TO_COMPLEX: return is_float(in) ? cplx_of(in) : -2;
    case GR4HIP_COMPLEX_TO_INTERLEAVED: return is_cplx(in) ? -1 : -2;
    case GR4HIP_INTERLEAVED_TO_COMPLEX: return is_interleavable(in) ? -1 : -2;
    default: return -2;
    }
}

// calls f(Op{}) with the functor of a CHECKED parameter set
template <typename F>
static int dispatch(const gr4hip_convert_params& p, F&& f) {
    switch (p.kind) {
    case GR4HIP_CONVERT: case GR4HIP_SCALING_CONVERT:
        return with_arith(p.in_dtype, [&](auto t) { return with_arith(p.out_dtype, [&](auto r) { return f(OpScale<typename decltype(t)::type, typename decltype(r)::type>{}); }); });
    case GR4HIP_CONVERT_ABS:
        if (p.in_dtype == GR4HIP_C32) return f(OpAbs<float2>{});
        if (p.in_dtype == GR4HIP_C64) return f(OpAbs<double2>{});
        return with_arith(p.in_dtype, [&](auto t) { return f(OpAbs<typename decltype(t)::type>{}); });
    case GR4HIP_CONVERT_REAL: return with_float(p.in_dtype, [&](auto t) { return f(OpPart<typename CplxOf<typename decltype(t)::type>::type, 0>{}); });
    case GR4HIP_CONVERT_IMAG: return with_float(p.in_dtype, [&](auto t) { return f(OpPart<typename CplxOf<typename decltype(t)::type>::type, 1>{}); });
    case GR4HIP_CONVERT_ARG: return with_float(p.in_dtype, [&](auto t) { return f(OpPart<typename CplxOf<typename decltype(t)::type>::type, 2>{}); });
    case GR4HIP_RADIANS_TO_DEGREE: return with_float(p.in_dtype, [&](auto t) { return f(OpAngle<typename decltype(t)::type, true>{}); });
    case GR4HIP_DEGREE_TO_RADIANS: return with_float(p.in_dtype, [&](auto t) { return f(OpAngle<typename decltype(t)::type, false>{}); });
    case GR4HIP_TO_REAL_IMAG: return with_float(p.in_dtype, [&](auto t) { return f(OpSplit<typename CplxOf<typename decltype(t)::type>::type, false>{}); });
    case GR4HIP_TO_MAG_PHASE: return with_float(p.in_dtype, [&](auto t) { return f(OpSplit<typename CplxOf<typename decltype(t)::type>::type, true>{}); });
    case GR4HIP_REAL_IMAG_TO_COMPLEX: return with_float(p.in_dtype, [&](auto t) { return f(OpJoin<typename decltype(t)::type, false>{}); });
    case GR4HIP_MAG_PHASE_TO_COMPLEX: return with_float(p.in_dtype, [&](auto t) { return f(OpJoin<typename decltype(t)::type, true>{}); });
    case GR4HIP_COMPLEX_TO_INTERLEAVED:
        return with_float(p.in_dtype, [&](auto t) { return with_interleavable(p.out_dtype, [&](auto r) { return f(OpC2I<typename CplxOf<typename decltype(t)::type>::type, typename decltype(r)::type>{}); }); });
    case GR4HIP_INTERLEAVED_TO_COMPLEX:
        return with_interleavable(p.in_dtype, [&](auto t) { return with_float(p.out_dtype, [&](auto r) { return f(OpI2C<typename decltype(t)::type, typename CplxOf<typename decltype(r)::type>::type>{}); }); });
    default: return GR4HIP_INVALID_ARGUMENT;
    }
}

static unsigned long long scale_as(int dtype, double scale) { // static_cast<T>(scale), with the library's float -> integer rule
    unsigned long long bits = 0;
    with_arith(dtype, [&](auto t) {
        using T   = typename decltype(t)::type;
        const T s = cast<T>(scale);
        std::memcpy(&bits, &s, sizeof(T));
        return 0;
    });
    return bits;
}

template <class Op>
static int launch(const gr4hip_convert* h, const void* const* d_in, void* const* d_out, long n, const EwiseHook& pre, const EwiseHook& post, hipStream_t st) {
    using TI = typename Op::TI;
    using TO = typename Op::TO;
    constexpr long L = lane_items<Op>(), SL = lane_slabs<Op>();
    CvArgs<Op>     a{};
    for (int p = 0; p < Op::NI; ++p) a.in[p] = static_cast<const TI*>(d_in[p]);
    for (int q = 0; q < Op::NO; ++q) a.out[q] = static_cast<TO*>(d_out[q]);
    // the head: the fewest items after which the accesses of L items are aligned to their own width on as many ports as possible, the widest accesses first (a
    // ring's input and output spans advance independently, so the ports need not agree); a port left unaligned moves its L items element by element, the
    // others keep their wide accesses
    const auto misaligned = [&](long hd) {
        unsigned m = 0;
        for (int p = 0; p < Op::NI; ++p) m |= unsigned((reinterpret_cast<uintptr_t>(a.in[p]) + (uintptr_t)hd * sizeof(TI) * Op::EI) % (L * sizeof(TI) * Op::EI) != 0) << p;
        for (int q = 0; q < Op::NO; ++q) m |= unsigned(a.out[q] && (reinterpret_cast<uintptr_t>(a.out[q]) + (uintptr_t)hd * sizeof(TO) * Op::EO) % (L * sizeof(TO) * Op::EO) != 0) << (Op::NI + q);
        return m;
    };
    const auto cost = [&](unsigned m) { // bytes per item that would move element-wise
        long c = 0;
        for (int p = 0; p < Op::NI; ++p) c += ((m >> p) & 1u) * (long)(sizeof(TI) * Op::EI);
        for (int q = 0; q < Op::NO; ++q) c += ((m >> (Op::NI + q)) & 1u) * (long)(sizeof(TO) * Op::EO);
        return c;
    };
    long head = 0;
    for (long hd = 1; hd < 16; ++hd)
        if (cost(misaligned(hd)) < cost(misaligned(head))) head = hd;
    a.n          = n;
    a.head       = std::min(head, n);
    a.nvec       = (n - a.head) / L;
    a.unaligned  = misaligned(head);
    a.scale_bits = h->p.kind == GR4HIP_SCALING_CONVERT ? h->scale_bits : scale_as(h->p.in_dtype, 1.0);
    a.pre        = pre;
    a.post       = post;
    GR4_REQUIRE(ceil_div(a.nvec + 1, 256L * SL) < (1L << 31), "convert: span too long for one launch");
    const long     nscalar = n - a.nvec * L;
    const unsigned grid    = (unsigned)std::max<long>({ceil_div(a.nvec, 256L * SL), std::min<long>(ceil_div(nscalar, 1024L), 16384L), 1L});
    hipLaunchKernelGGL(convert_kernel<Op>, dim3(grid), dim3(256), 0, st, a);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

struct Ports { int n_in, n_out, in_chunk, out_chunk; };
static Ports ports_of(const gr4hip_convert_params& p) {
    Ports r{};
    dispatch(p, [&](auto op) {
        using Op = decltype(op);
        r        = Ports{Op::NI, Op::NO, Op::EI, Op::EO};
        return 0;
    });
    return r;
}

static int set_hook(gr4hip_convert* h, const gr4hip_ewise_t* prog, bool prologue) {
    const char* what = prologue ? "prologue" : "epilogue";
    GR4_REQUIRE(h, "convert_set_%s: null handle", what);
    gr4hip_ewise* copy = nullptr;
    if (prog) {
        const Ports pt   = ports_of(h->p);
        const int   want = prologue ? h->p.in_dtype : h->p.out_dtype;
        if ((prologue ? pt.n_in : pt.n_out) != 1) { set_error("convert_set_%s: kind %d has %d %s ports", what, h->p.kind, prologue ? pt.n_in : pt.n_out, prologue ? "input" : "output"); return GR4HIP_UNSUPPORTED; }
        if (prog->dtype != want) { set_error("convert_set_%s: the program's dtype %d is not the port's (%d)", what, prog->dtype, want); return GR4HIP_UNSUPPORTED; }
        if (!prog->user.empty()) {
            copy = ewise_clone(prog);
            GR4_REQUIRE(copy, "out of host memory");
        }
    }
    gr4hip_ewise*& slot = prologue ? h->pre : h->post;
    if (slot) h->retired.push_back(slot); // (a launch that reads its device copy may still be in flight: no hipFree from a set_* call)
    slot = copy;
    return GR4HIP_OK;
}

} // namespace cv
} // namespace gr4

extern "C" {

int gr4hip_convert_params_default(gr4hip_convert_params* p, int kind, int in_dtype) {
    GR4_REQUIRE(p, "convert_params_default: null argument");
    const int r  = cv::result_dtype(kind, in_dtype);
    p->kind      = kind;
    p->in_dtype  = in_dtype;
    p->out_dtype = r >= 0 ? r : in_dtype;
    p->scale     = 1.0;
    return GR4HIP_OK;
}

int gr4hip_convert_params_check(const gr4hip_convert_params* p) {
    GR4_REQUIRE(p, "convert_params_check: null argument");
    GR4_REQUIRE(p->kind >= GR4HIP_CONVERT && p->kind <= GR4HIP_INTERLEAVED_TO_COMPLEX, "convert: unknown kind %d", p->kind);
    const int r = cv::result_dtype(p->kind, p->in_dtype);
    GR4_REQUIRE(r != -2, "convert: kind %d does not take input dtype %d", p->kind, p->in_dtype);
    if (r >= 0) GR4_REQUIRE(p->out_dtype == r, "convert: kind %d on dtype %d produces dtype %d, not %d", p->kind, p->in_dtype, r, p->out_dtype);
    else if (p->kind == GR4HIP_COMPLEX_TO_INTERLEAVED) GR4_REQUIRE(cv::is_interleavable(p->out_dtype), "convert: ComplexToInterleaved writes float, double, int8 or int16 (dtype %d)", p->out_dtype);
    else if (p->kind == GR4HIP_INTERLEAVED_TO_COMPLEX) GR4_REQUIRE(cv::is_cplx(p->out_dtype), "convert: InterleavedToComplex writes complex<float> or complex<double> (dtype %d)", p->out_dtype);
    else GR4_REQUIRE(cv::is_arith(p->out_dtype), "convert: Convert / ScalingConvert write an arithmetic type (dtype %d)", p->out_dtype);
    return GR4HIP_OK;
}

int gr4hip_convert_create(gr4hip_convert_t** out, const gr4hip_convert_params* p) {
    GR4_REQUIRE(out, "convert: null output handle");
    if (const int rc = gr4hip_convert_params_check(p)) return rc;
    if (const int rc = have_device("convert")) return rc;
    auto* h = new (std::nothrow) gr4hip_convert();
    GR4_REQUIRE(h, "out of host memory");
    h->p          = *p;
    h->scale_bits = cv::scale_as(p->in_dtype, p->scale);
    *out          = h;
    return GR4HIP_OK;
}

int gr4hip_convert_destroy(gr4hip_convert_t* h) { delete h; return GR4HIP_OK; }

int gr4hip_convert_set_scale(gr4hip_convert_t* h, double scale) {
    GR4_REQUIRE(h, "convert_set_scale: null handle");
    GR4_REQUIRE(h->p.kind == GR4HIP_SCALING_CONVERT, "convert_set_scale: only ScalingConvert has a scale (kind %d)", h->p.kind);
    h->p.scale    = scale;
    h->scale_bits = cv::scale_as(h->p.in_dtype, scale); // an argument of the next launch: ordered with the data by the stream
    return GR4HIP_OK;
}

int gr4hip_convert_reset(gr4hip_convert_t* h) {
    GR4_REQUIRE(h, "convert_reset: null handle");
    h->pos = 0;
    return GR4HIP_OK;
}

int gr4hip_convert_ports(const gr4hip_convert_t* h, size_t* n_in, size_t* n_out, size_t* in_chunk, size_t* out_chunk) {
    GR4_REQUIRE(h, "convert_ports: null handle");
    const cv::Ports pt = cv::ports_of(h->p);
    if (n_in) *n_in = (size_t)pt.n_in;
    if (n_out) *n_out = (size_t)pt.n_out;
    if (in_chunk) *in_chunk = (size_t)pt.in_chunk;
    if (out_chunk) *out_chunk = (size_t)pt.out_chunk;
    return GR4HIP_OK;
}

int gr4hip_convert_set_prologue(gr4hip_convert_t* h, const gr4hip_ewise_t* prog) { return cv::set_hook(h, prog, true); }
int gr4hip_convert_set_epilogue(gr4hip_convert_t* h, const gr4hip_ewise_t* prog) { return cv::set_hook(h, prog, false); }

size_t gr4hip_convert_tile(const gr4hip_convert_params* p) {
    if (!p || gr4hip_convert_params_check(p) != GR4HIP_OK) return 0;
    size_t w = 0;
    cv::dispatch(*p, [&](auto op) {
        using Op = decltype(op);
        w        = (size_t)256 * cv::lane_items<Op>() * cv::lane_slabs<Op>();
        return 0;
    });
    return w;
}

int gr4hip_convert_process(gr4hip_convert_t* h, const void* const* d_in, void* const* d_out, size_t n_in, size_t* n_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "convert_process: null handle");
    const cv::Ports pt = cv::ports_of(h->p);
    GR4_REQUIRE(n_in % (size_t)pt.in_chunk == 0, "convert_process: InterleavedToComplex takes whole (re, im) pairs (n_in = %zu)", n_in);
    GR4_REQUIRE(n_in <= (size_t)1 << 40, "convert_process: n_in = %zu", n_in);
    const long n = (long)(n_in / (size_t)pt.in_chunk);
    if (n_out) *n_out = (size_t)n * (size_t)pt.out_chunk;
    if (n == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in && d_out, "convert_process: null pointer array");
    for (int p = 0; p < pt.n_in; ++p) {
        GR4_REQUIRE(d_in[p], "convert_process: input %d is NULL", p);
        GR4_REQUIRE(reinterpret_cast<uintptr_t>(d_in[p]) % dtype_size(h->p.in_dtype) == 0, "convert_process: input %d is not aligned to its element type", p);
    }
    for (int q = 0; q < pt.n_out; ++q)
        GR4_REQUIRE(!d_out[q] || reinterpret_cast<uintptr_t>(d_out[q]) % dtype_size(h->p.out_dtype) == 0, "convert_process: output %d is not aligned to its element type", q);
    hipStream_t st = as_stream(stream);
    h->drop_retired(); // hipFree waits for the launches that still read them
    EwiseHook   pre{}, post{};
    if (h->pre) { if (const int rc = ewise_device_ops(h->pre, &pre, st)) return rc; }
    if (h->post) { if (const int rc = ewise_device_ops(h->post, &post, st)) return rc; }
    pre.pos = post.pos = h->pos; // the handle's position, not the copies'
    const int rc = cv::dispatch(h->p, [&](auto op) { return cv::launch<decltype(op)>(h, d_in, d_out, n, pre, post, st); });
    if (rc) return rc;
    h->pos += n;
    return GR4HIP_OK;
}

} // extern "C"
