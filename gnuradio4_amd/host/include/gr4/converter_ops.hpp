// converter_ops.hpp -- the arithmetic rules of the type-converter blocks (blocks/basic/.../ConverterBlocks.hpp), ONE definition for the host mirror blocks
// (gr4/blocks.hpp) and the device kernels (csrc/convert.hip): the host and the device domain of a block then agree on every input, also where the reference's
// C++ is undefined (CONVERTERS.md): float -> integer saturates and NaN -> 0; signed overflow of input * scale and of abs wraps modulo 2^w.
#pragma once
#include <limits>
#include <type_traits>

#if defined(__HIPCC__)
#define GR4_CONV_HD __host__ __device__ __forceinline__
#else
#define GR4_CONV_HD inline
#endif

namespace gr4::converter_ops {

// float -> integer: truncation toward zero inside R's range; saturation outside, NaN -> 0 (as SignalGenerator's integer outputs)
template <typename R, typename F>
GR4_CONV_HD R sat_cast(F v) {
    constexpr int bits = 8 * (int)sizeof(R) - (std::is_signed_v<R> ? 1 : 0);
    const F       hi   = (F)(1ull << (bits - 1)) * F(2); // 2^bits: exact in float and double
    const F       lo   = std::is_signed_v<R> ? -hi : F(0);
    if (v != v) return R(0);
    if (v >= hi) return std::numeric_limits<R>::max();
    if (v <= lo) return std::numeric_limits<R>::min();
    return (R)v;
}
// static_cast<R>(v): integers narrow modulo 2^w, integer -> float rounds once, float -> float rounds to nearest, float -> integer as above
template <typename R, typename P>
GR4_CONV_HD R cast(P v) {
    if constexpr (std::is_floating_point_v<P> && std::is_integral_v<R>) return sat_cast<R>(v);
    else return (R)v;
}
// input * scale in the promoted type of T (int for the 8- and 16-bit types); signed overflow wraps modulo 2^w
template <typename T>
GR4_CONV_HD auto mul(T x, T s) {
    using P = decltype(T() * T());
    if constexpr (std::is_integral_v<P>) {
        using U = std::make_unsigned_t<P>;
        return (P)((U)(P)x * (U)(P)s);
    } else {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        return (P)(x * s);
    }
}
// static_cast<T>(std::abs(static_cast<std::make_signed_t<T>>(x))) (ConverterBlocks.hpp:74-79); abs of the minimum wraps to itself
template <typename T>
GR4_CONV_HD T abs_int(T x) {
    using S   = std::make_signed_t<T>;
    using U   = std::make_unsigned_t<T>;
    const S s = (S)x;
    const U u = (U)s;
    return (T)(s < 0 ? (U)(U(0) - u) : u);
}

} // namespace gr4::converter_ops
