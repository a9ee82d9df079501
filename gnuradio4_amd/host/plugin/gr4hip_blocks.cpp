// libgr4hip_blocks.so -- the hot-path blocks as a GNU Radio 4 plugin (core/include/gnuradio-4.0/Plugin.hpp:82-85).
//
// Exports gr_plugin_make / gr_plugin_free; the blocks are registered under the names the reference's registry uses for them
// (GR_REGISTER_BLOCK lines of time_domain_filter.hpp:20-213, Math.hpp:25-71, Rotator.hpp:15, fft.hpp:29; portable type names
// float32 / complex<float32> / int32 ... of meta/utils.hpp:481-490), so a graph description that names
//     gr::filter::fir_filter<float32>   with   compute_domain: "gpu:hip:0"
// resolves to the block whose work() goes through the device seam (gr4/hip.hpp) into libgr4hip.so.  With compute_domain "host" (the
// default) the same block runs its host body.
#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

GR_PLUGIN("gr4hip hot-path blocks (MI355X)", "gr4-hip", "LGPL-3.0-or-later", "r01")

namespace {
using namespace gr;

template <typename T> constexpr std::string_view portable() {
    if constexpr (std::is_same_v<T, std::uint8_t>) return "uint8"; else if constexpr (std::is_same_v<T, std::uint16_t>) return "uint16";
    else if constexpr (std::is_same_v<T, std::uint32_t>) return "uint32"; else if constexpr (std::is_same_v<T, std::uint64_t>) return "uint64";
    else if constexpr (std::is_same_v<T, std::int8_t>) return "int8"; else if constexpr (std::is_same_v<T, std::int16_t>) return "int16";
    else if constexpr (std::is_same_v<T, std::int32_t>) return "int32"; else if constexpr (std::is_same_v<T, std::int64_t>) return "int64";
    else if constexpr (std::is_same_v<T, float>) return "float32"; else if constexpr (std::is_same_v<T, double>) return "float64";
    else if constexpr (std::is_same_v<T, std::complex<float>>) return "complex<float32>"; else return "complex<float64>";
}
template <typename T> std::string named(std::string_view base, std::string_view extra = "") { return std::string(base) + "<" + std::string(portable<T>()) + std::string(extra) + ">"; }

template <typename T>
void register_math(BlockRegistry& r) {
    using namespace gr::blocks::math;
    r.insert<AddConst<T>>(named<T>("gr::blocks::math::AddConst"));
    r.insert<SubtractConst<T>>(named<T>("gr::blocks::math::SubtractConst"));
    r.insert<MultiplyConst<T>>(named<T>("gr::blocks::math::MultiplyConst"));
    r.insert<DivideConst<T>>(named<T>("gr::blocks::math::DivideConst"));
    r.insert<Add<T>>(named<T>("gr::blocks::math::Add"));
    r.insert<Subtract<T>>(named<T>("gr::blocks::math::Subtract"));
    r.insert<Multiply<T>>(named<T>("gr::blocks::math::Multiply"));
    r.insert<Divide<T>>(named<T>("gr::blocks::math::Divide"));
    r.insert<gr::filter::Decimator<T>>(named<T>("gr::filter::Decimator"));
}
template <typename T>
void register_io(BlockRegistry& r) { // sources / sinks / converters so that a whole graph can come out of the registry
    r.insert<gr::testing::VectorSource<T>>(named<T>("gr::testing::VectorSource"));
    r.insert<gr::testing::VectorSink<T>>(named<T>("gr::testing::VectorSink"));
    r.insert<gr::testing::NullSink<T>>(named<T>("gr::testing::NullSink"));
    r.insert<gr::hip::H2D<T>>(named<T>("gr::hip::H2D"));
    r.insert<gr::hip::D2H<T>>(named<T>("gr::hip::D2H"));
}

template <typename T>
void register_schmitt(BlockRegistry& r) { // basic/Trigger.hpp:11-13; SchmittTriggerPolynomial (:14) has no device implementation and is not registered
    using namespace gr::blocks::basic;
    r.insert<SchmittTriggerNoInterpolation<T>>(named<T>("gr::blocks::basic::SchmittTriggerNoInterpolation"));
    r.insert<SchmittTriggerBasic<T>>(named<T>("gr::blocks::basic::SchmittTriggerBasic"));
    r.insert<SchmittTriggerLinear<T>>(named<T>("gr::blocks::basic::SchmittTrigger"));
}

template <typename T>
void register_power_quality(BlockRegistry& r) { // PowerEstimators.hpp:141-142, 190-191; the gr::UncertainValue<T> instantiations are left out, as for PowerMetrics
    using namespace gr::electrical;
    r.insert<SinglePhasePowerFactorCalculator<T>>(named<T>("gr::electrical::SinglePhasePowerFactorCalculator"));
    r.insert<ThreePhasePowerFactorCalculator<T>>(named<T>("gr::electrical::ThreePhasePowerFactorCalculator"));
    r.insert<TwoPhaseSystemUnbalanceCalculator<T>>(named<T>("gr::electrical::TwoPhaseSystemUnbalanceCalculator"));
    r.insert<ThreePhaseSystemUnbalanceCalculator<T>>(named<T>("gr::electrical::ThreePhaseSystemUnbalanceCalculator"));
}

template <typename T>
void register_signal_generator(BlockRegistry& r) { // basic/SignalGenerator.hpp:25 registers every fundamental type; the four with a device implementation are offered
    r.insert<gr::basic::SignalGenerator<T>>(named<T>("gr::basic::SignalGenerator"));
    r.insert<gr::hip::SignalSource<T>>(named<T>("gr::hip::SignalSource"));
}

} // namespace
// the converter blocks (ConverterBlocks.hpp:13-256; gr4hip_converters.cpp): a work loop per registered block type costs seconds of compile time, so the 246 types
// are compiled as twelve translation units side by side
#define GR4HIP_CONVERTER_PART(k) void gr4hip_register_converters_##k(gr::BlockRegistry&);
GR4HIP_CONVERTER_PART(0) GR4HIP_CONVERTER_PART(1) GR4HIP_CONVERTER_PART(2) GR4HIP_CONVERTER_PART(3) GR4HIP_CONVERTER_PART(4) GR4HIP_CONVERTER_PART(5)
GR4HIP_CONVERTER_PART(6) GR4HIP_CONVERTER_PART(7) GR4HIP_CONVERTER_PART(8) GR4HIP_CONVERTER_PART(9) GR4HIP_CONVERTER_PART(10) GR4HIP_CONVERTER_PART(11)
namespace {
using namespace gr;
const bool registered = [] {
    BlockRegistry& r = grPluginInstance();
    using namespace gr::filter;
    register_math<std::uint8_t>(r); register_math<std::uint16_t>(r); register_math<std::uint32_t>(r); register_math<std::uint64_t>(r);
    register_math<std::int8_t>(r); register_math<std::int16_t>(r); register_math<std::int32_t>(r); register_math<std::int64_t>(r);
    register_math<float>(r); register_math<double>(r); register_math<std::complex<float>>(r); register_math<std::complex<double>>(r);
    register_io<float>(r); register_io<std::complex<float>>(r); register_io<std::int32_t>(r);
    r.insert<fir_filter<float>>(named<float>("gr::filter::fir_filter"));
    r.insert<fir_filter<double>>(named<double>("gr::filter::fir_filter")); // FP64 kernel behind the seam (csrc/f64.hip)
    r.insert<fir_filter<std::complex<float>>>(named<std::complex<float>>("gr::filter::fir_filter"));
    r.insert<complex_fir_filter<std::complex<float>>>(named<std::complex<float>>("gr::filter::complex_fir_filter")); // complex taps (no reference block)
    r.insert<rational_resampler<float>>(named<float>("gr::filter::rational_resampler")); // rate L / M (RATIONAL_RESAMPLER.md; no reference block)
    r.insert<rational_resampler<std::complex<float>>>(named<std::complex<float>>("gr::filter::rational_resampler"));
    r.insert<iir_filter<float, IIRForm::DF_I>>(named<float>("gr::filter::iir_filter", ", gr::filter::IIRForm::DF_I"));
    r.insert<iir_filter<float, IIRForm::DF_II>>(named<float>("gr::filter::iir_filter", ", gr::filter::IIRForm::DF_II"));
    r.insert<iir_filter<float, IIRForm::DF_I_TRANSPOSED>>(named<float>("gr::filter::iir_filter", ", gr::filter::IIRForm::DF_I_TRANSPOSED"));
    r.insert<iir_filter<float, IIRForm::DF_II_TRANSPOSED>>(named<float>("gr::filter::iir_filter", ", gr::filter::IIRForm::DF_II_TRANSPOSED"));
    r.insert<iir_filter<double, IIRForm::DF_I>>(named<double>("gr::filter::iir_filter", ", gr::filter::IIRForm::DF_I"));
    r.insert<iir_filter<double, IIRForm::DF_II>>(named<double>("gr::filter::iir_filter", ", gr::filter::IIRForm::DF_II"));
    r.insert<iir_filter<double, IIRForm::DF_I_TRANSPOSED>>(named<double>("gr::filter::iir_filter", ", gr::filter::IIRForm::DF_I_TRANSPOSED"));
    r.insert<iir_filter<double, IIRForm::DF_II_TRANSPOSED>>(named<double>("gr::filter::iir_filter", ", gr::filter::IIRForm::DF_II_TRANSPOSED"));
    r.insert<BasicFilter<float>>(named<float>("gr::filter::BasicFilter"));
    r.insert<BasicDecimatingFilter<float>>(named<float>("gr::filter::BasicFilterProto", ", gr::Resampling<1, 1, false>"));
    r.insert<gr::blocks::math::Rotator<std::complex<float>>>(named<std::complex<float>>("gr::blocks::math::Rotator"));
    r.insert<gr::blocks::math::Rotator<std::complex<double>>>(named<std::complex<double>>("gr::blocks::math::Rotator"));
    r.insert<FrequencyEstimatorTimeDomain<float>>(named<float>("gr::filter::FrequencyEstimatorTimeDomain")); // FrequencyEstimator.hpp:25-26, 181-182 (float only)
    r.insert<FrequencyEstimatorTimeDomainDecimating<float>>(named<float>("gr::filter::FrequencyEstimatorTimeDomainDecimating"));
    r.insert<FrequencyEstimatorFrequencyDomain<float>>(named<float>("gr::filter::FrequencyEstimatorFrequencyDomain"));
    r.insert<FrequencyEstimatorFrequencyDomainDecimating<float>>(named<float>("gr::filter::FrequencyEstimatorFrequencyDomainDecimating"));
    r.insert<IQDemodulatorDecimating<float>>(named<float>("gr::filter::IQDemodulator", ", gr::Resampling<1024U, 1U, false>")); // FrequencyEstimator.hpp:385
    r.insert<IQDemodulatorDecimating<double>>(named<double>("gr::filter::IQDemodulator", ", gr::Resampling<1024U, 1U, false>"));
    r.insert<gr::electrical::SinglePhasePowerMetrics<float>>(named<float>("gr::electrical::SinglePhasePowerMetrics")); // PowerEstimators.hpp:18-19
    r.insert<gr::electrical::ThreePhasePowerMetrics<float>>(named<float>("gr::electrical::ThreePhasePowerMetrics"));
    register_power_quality<float>(r); register_power_quality<double>(r);
    register_schmitt<std::int16_t>(r); register_schmitt<std::int32_t>(r); register_schmitt<float>(r); register_schmitt<double>(r);
    r.insert<SvdDenoiser<float>>(named<float>("gr::filter::SvdDenoiser")); // SvdDenoiser.hpp:12
    r.insert<SvdDenoiser<double>>(named<double>("gr::filter::SvdDenoiser"));
    r.insert<SvdDenoiser<std::complex<float>>>(named<std::complex<float>>("gr::filter::SvdDenoiser"));
    r.insert<SvdDenoiser<std::complex<double>>>(named<std::complex<double>>("gr::filter::SvdDenoiser"));
    r.insert<SavitzkyGolayFilter<float>>(named<float>("gr::filter::SavitzkyGolayFilter")); // SavitzkyGolayFilter.hpp:17, 87
    r.insert<SavitzkyGolayFilter<double>>(named<double>("gr::filter::SavitzkyGolayFilter"));
    r.insert<SavitzkyGolayDataSetFilter<float>>(named<float>("gr::filter::SavitzkyGolayDataSetFilter"));
    r.insert<SavitzkyGolayDataSetFilter<double>>(named<double>("gr::filter::SavitzkyGolayDataSetFilter"));
    register_signal_generator<float>(r); register_signal_generator<double>(r); register_signal_generator<std::complex<float>>(r); register_signal_generator<std::int16_t>(r);
    r.insert<gr::blocks::fft::FFT<double, gr::DataSet<double>>>(named<double>("gr::blocks::fft::FFT"));
    r.insert<gr::blocks::fft::FFT<float>>(named<float>("gr::blocks::fft::FFT"));
    r.insert<gr::blocks::fft::FFT<std::complex<float>>>(named<std::complex<float>>("gr::blocks::fft::FFT"));
    r.insert<gr::blocks::fft::PowerSpectrum<std::complex<float>>>(named<std::complex<float>>("gr::blocks::fft::PowerSpectrum"));
    r.insert<gr::blocks::fft::PfbPowerSpectrum<std::complex<float>>>(named<std::complex<float>>("gr::blocks::fft::PfbPowerSpectrum")); // polyphase filter bank (PFB.md; no reference block)
    r.insert<gr::blocks::fft::PfbChannelizer<std::complex<float>>>(named<std::complex<float>>("gr::blocks::fft::PfbChannelizer"));
    r.insert<gr::blocks::fft::InverseFFT<std::complex<float>>>(named<std::complex<float>>("gr::blocks::fft::InverseFFT")); // inverse transform and synthesis bank (INVERSE_FFT.md)
    r.insert<gr::blocks::fft::InverseFFT<float>>(named<float>("gr::blocks::fft::InverseFFT"));
    r.insert<gr::blocks::fft::PfbSynthesizer<std::complex<float>>>(named<std::complex<float>>("gr::blocks::fft::PfbSynthesizer"));
    r.insert<gr::blocks::fft::SpectrumIntegrator<float>>(named<float>("gr::blocks::fft::SpectrumIntegrator")); // SPECTRUM_INTEGRATOR.md; no reference block
    r.insert<gr::blocks::fft::CrossSpectrum<float>>(named<float>("gr::blocks::fft::CrossSpectrum")); // CROSS_SPECTRUM.md; no reference block
    r.insert<gr::blocks::fft::Beamformer<float>>(named<float>("gr::blocks::fft::Beamformer")); // BEAMFORMER.md; no reference block
    r.insert<gr::blocks::fft::AdaptiveWeights<float>>(named<float>("gr::blocks::fft::AdaptiveWeights")); // ADAPTIVE_WEIGHTS.md; no reference block
    r.insert<gr::hip::OnDevice<fir_filter<float>>>(named<float>("gr::hip::OnDevice<gr::filter::fir_filter", ">"));
    r.insert<gr::hip::OnDevice<fir_filter<std::complex<float>>>>(named<std::complex<float>>("gr::hip::OnDevice<gr::filter::fir_filter", ">"));
    r.insert<gr::hip::OnDevice<gr::blocks::fft::PowerSpectrum<std::complex<float>>>>(named<std::complex<float>>("gr::hip::OnDevice<gr::blocks::fft::PowerSpectrum", ">"));
    gr4hip_register_converters_0(r); gr4hip_register_converters_1(r); gr4hip_register_converters_2(r); gr4hip_register_converters_3(r);
    gr4hip_register_converters_4(r); gr4hip_register_converters_5(r); gr4hip_register_converters_6(r); gr4hip_register_converters_7(r);
    gr4hip_register_converters_8(r); gr4hip_register_converters_9(r); gr4hip_register_converters_10(r); gr4hip_register_converters_11(r);
    gr::hip::register_provider(); // edges with EdgeParameters{.domain = "gpu:hip:i"} get pinned pages once the plugin is loaded
    return true;
}();
} // namespace
