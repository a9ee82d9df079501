// The converter blocks of libgr4hip_blocks.so (ConverterBlocks.hpp:13-256), one twelfth per translation unit: compiled with -DGR4HIP_CONVERTER_PART=0 .. 11 and
// linked into the plugin (gr4hip_blocks.cpp calls the twelve functions).  Each block under its OWN name (the reference's macros of RealImagToComplex, ToMagPhase
// and MagPhaseToComplex repeat ToRealImag) with the reference's type lists; the interleaved kinds also with int8 / int16 (the templates' constraint: the I/Q of
// an SDR or ADC).  Parts 0 .. 9: Convert / ScalingConvert from one input type to all ten, and Abs of that type; parts 10, 11: the float and the double kinds.
#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

#ifndef GR4HIP_CONVERTER_PART
#error "compile with -DGR4HIP_CONVERTER_PART=0 .. 11"
#endif

namespace {
using namespace gr;
using namespace gr::blocks::type::converter;

template <typename T> constexpr std::string_view portable() {
    if constexpr (std::is_same_v<T, std::uint8_t>) return "uint8"; else if constexpr (std::is_same_v<T, std::uint16_t>) return "uint16";
    else if constexpr (std::is_same_v<T, std::uint32_t>) return "uint32"; else if constexpr (std::is_same_v<T, std::uint64_t>) return "uint64";
    else if constexpr (std::is_same_v<T, std::int8_t>) return "int8"; else if constexpr (std::is_same_v<T, std::int16_t>) return "int16";
    else if constexpr (std::is_same_v<T, std::int32_t>) return "int32"; else if constexpr (std::is_same_v<T, std::int64_t>) return "int64";
    else if constexpr (std::is_same_v<T, float>) return "float32"; else if constexpr (std::is_same_v<T, double>) return "float64";
    else if constexpr (std::is_same_v<T, std::complex<float>>) return "complex<float32>"; else return "complex<float64>";
}
template <typename T> std::string named(std::string_view base) { return "gr::blocks::type::converter::" + std::string(base) + "<" + std::string(portable<T>()) + ">"; }
template <typename T, typename R> std::string named2(std::string_view base) {
    return "gr::blocks::type::converter::" + std::string(base) + "<" + std::string(portable<T>()) + ", " + std::string(portable<R>()) + ">";
}
template <typename T, typename R>
void pair(BlockRegistry& r) {
    r.insert<Convert<T, R>>(named2<T, R>("Convert"));
    r.insert<ScalingConvert<T, R>>(named2<T, R>("ScalingConvert"));
}
template <typename T>
[[maybe_unused]] void from(BlockRegistry& r) {
    pair<T, std::uint8_t>(r); pair<T, std::uint16_t>(r); pair<T, std::uint32_t>(r); pair<T, std::uint64_t>(r);
    pair<T, std::int8_t>(r); pair<T, std::int16_t>(r); pair<T, std::int32_t>(r); pair<T, std::int64_t>(r);
    pair<T, float>(r); pair<T, double>(r);
    r.insert<Abs<T>>(named<T>("Abs"));
}
template <typename F>
[[maybe_unused]] void of(BlockRegistry& r) { // F = float, double
    using Cx = std::complex<F>;
    r.insert<Abs<Cx>>(named<Cx>("Abs"));
    r.insert<Real<Cx>>(named<Cx>("Real"));
    r.insert<Imag<Cx>>(named<Cx>("Imag"));
    r.insert<Arg<Cx>>(named<Cx>("Arg"));
    r.insert<ToRealImag<Cx>>(named<Cx>("ToRealImag"));
    r.insert<ToMagPhase<Cx>>(named<Cx>("ToMagPhase"));
    r.insert<RadiansToDegree<F>>(named<F>("RadiansToDegree"));
    r.insert<DegreeToRadians<F>>(named<F>("DegreeToRadians"));
    r.insert<RealImagToComplex<F>>(named<F>("RealImagToComplex"));
    r.insert<MagPhaseToComplex<F>>(named<F>("MagPhaseToComplex"));
    r.insert<ComplexToInterleaved<Cx, float>>(named2<Cx, float>("ComplexToInterleaved"));
    r.insert<ComplexToInterleaved<Cx, double>>(named2<Cx, double>("ComplexToInterleaved"));
    r.insert<ComplexToInterleaved<Cx, std::int8_t>>(named2<Cx, std::int8_t>("ComplexToInterleaved"));
    r.insert<ComplexToInterleaved<Cx, std::int16_t>>(named2<Cx, std::int16_t>("ComplexToInterleaved"));
    r.insert<InterleavedToComplex<float, Cx>>(named2<float, Cx>("InterleavedToComplex"));
    r.insert<InterleavedToComplex<double, Cx>>(named2<double, Cx>("InterleavedToComplex"));
    r.insert<InterleavedToComplex<std::int8_t, Cx>>(named2<std::int8_t, Cx>("InterleavedToComplex"));
    r.insert<InterleavedToComplex<std::int16_t, Cx>>(named2<std::int16_t, Cx>("InterleavedToComplex"));
}
} // namespace

#define GR4HIP_CAT2(a, b) a##b
#define GR4HIP_CAT(a, b) GR4HIP_CAT2(a, b)
void GR4HIP_CAT(gr4hip_register_converters_, GR4HIP_CONVERTER_PART)(gr::BlockRegistry& r) {
#if GR4HIP_CONVERTER_PART == 0
    from<std::uint8_t>(r);
#elif GR4HIP_CONVERTER_PART == 1
    from<std::uint16_t>(r);
#elif GR4HIP_CONVERTER_PART == 2
    from<std::uint32_t>(r);
#elif GR4HIP_CONVERTER_PART == 3
    from<std::uint64_t>(r);
#elif GR4HIP_CONVERTER_PART == 4
    from<std::int8_t>(r);
#elif GR4HIP_CONVERTER_PART == 5
    from<std::int16_t>(r);
#elif GR4HIP_CONVERTER_PART == 6
    from<std::int32_t>(r);
#elif GR4HIP_CONVERTER_PART == 7
    from<std::int64_t>(r);
#elif GR4HIP_CONVERTER_PART == 8
    from<float>(r);
#elif GR4HIP_CONVERTER_PART == 9
    from<double>(r);
#elif GR4HIP_CONVERTER_PART == 10
    of<float>(r);
#else
    of<double>(r);
#endif
}
