// gr4/blocks.hpp -- block definitions on the hot path, written against gr4/core.hpp in the reference's block style.
//
// Each block states the reference block it mirrors (settings names, port names, semantics, error behaviour).  The processOne /
// processBulk bodies are the host ("compute_domain = host") path used by BASELINE configs[0] (CPU scheduler plumbing); with
// compute_domain = "gpu:hip[:i]" the work loop dispatches to gr::hip::Kernel<Block> (gr4/hip.hpp) instead.
#pragma once
#include <bit>
#include <cmath>
#include <numbers>

#include "../../../../include/gr4hip.h" // host-side design functions only (gr4hip_fir_design / gr4hip_iir_design / gr4hip_window_create: no device needed)
#include "converter_ops.hpp"
#include "electrical_ops.hpp"
#include "core.hpp"

namespace gr::testing {

// settable-values source with a sample budget: the role of TagSource<T> (blocks/testing/.../TagMonitors.hpp:134-293) without tags
template <typename T>
struct VectorSource : Block<VectorSource<T>> {
    PortOut<T>     out;
    std::vector<T> values{};      // repeated cyclically when shorter than n_samples_max
    Size_t         n_samples_max = 0; // 0: exactly values.size() samples
    std::size_t    _produced     = 0;
    std::vector<Tag> _tags{};     // tags to emit, ascending index (TagSource::_tags)
    GR_MAKE_REFLECTABLE(VectorSource, out, values, n_samples_max);

    work::Result customWork(std::size_t requested) {
        const std::size_t total = n_samples_max ? n_samples_max : values.size();
        if (_produced >= total) return {requested, 0, work::Status::DONE};
        if (!out.connected()) return {requested, 0, work::Status::ERROR};
        const std::size_t n = std::min({total - _produced, out.buffer->free_space(), requested});
        if (n == 0) return {requested, 0, work::Status::INSUFFICIENT_OUTPUT_ITEMS};
        auto span = out.buffer->write_span(n);
        if (values.empty()) std::fill(span.begin(), span.end(), T{});
        else
            for (std::size_t i = 0; i < n;) { // whole runs of the cyclic pattern at a time
                const std::size_t at = (_produced + i) % values.size(), run = std::min(n - i, values.size() - at);
                std::copy_n(values.begin() + static_cast<std::ptrdiff_t>(at), run, span.begin() + static_cast<std::ptrdiff_t>(i));
                i += run;
            }
        for (const Tag& t : _tags)
            if (t.index >= _produced && t.index < _produced + n) out.buffer->publishTag(t.map, t.index - _produced);
        out.buffer->publish(n);
        _produced += n;
        return {requested, n, work::Status::OK};
    }
};

// records everything it receives: TagSink<T> (TagMonitors.hpp:391-479) without tags
template <typename T>
struct VectorSink : Block<VectorSink<T>> {
    PortIn<T>      in;
    Size_t         n_samples_expected = 0;
    std::vector<T> _samples;
    std::vector<Tag> _tags; // received tags with their absolute sample index (TagSink::_tags)
    GR_MAKE_REFLECTABLE(VectorSink, in, n_samples_expected);

    work::Result customWork(std::size_t requested) {
        if (!in.connected()) return {requested, 0, work::Status::ERROR};
        const std::size_t n = std::min(in.buffer->available(), requested);
        if (n == 0) return {requested, 0, in.buffer->done() ? work::Status::DONE : work::Status::INSUFFICIENT_INPUT_ITEMS};
        auto span = in.buffer->read_span(n);
        for (const Tag& t : in.buffer->tags)
            if (t.index < in.buffer->read_pos + n) _tags.push_back(t);
        _samples.insert(_samples.end(), span.begin(), span.end());
        in.buffer->consume(n);
        return {requested, n, work::Status::OK};
    }
};

// NullSink<T> / CountingSink<T> (blocks/testing/.../NullSources.hpp): consumes and counts
template <typename T>
struct NullSink : Block<NullSink<T>> {
    PortIn<T>   in;
    std::size_t _count = 0;
    GR_MAKE_REFLECTABLE(NullSink, in);
    work::Result customWork(std::size_t requested) {
        if (!in.connected()) return {requested, 0, work::Status::ERROR};
        const std::size_t n = std::min(in.buffer->available(), requested);
        if (n == 0) return {requested, 0, in.buffer->done() ? work::Status::DONE : work::Status::INSUFFICIENT_INPUT_ITEMS};
        in.buffer->consume(n);
        _count += n;
        return {requested, n, work::Status::OK};
    }
};
} // namespace gr::testing

namespace gr::basic {
namespace signal_generator {
enum class Type : int { Const, Sin, Cos, Square, Saw, Triangle, FastSin, FastCos, UniformNoise, TriangularNoise, GaussianNoise }; // SignalGeneratorCore.hpp:16
inline bool gr_enum_parse(Type& d, std::string_view s) {
    return gr::detail::enum_from_names(d, s, std::array<std::string_view, 11>{"Const", "Sin", "Cos", "Square", "Saw", "Triangle", "FastSin", "FastCos", "UniformNoise", "TriangularNoise", "GaussianNoise"});
}

// xoshiro256++ with the reference's float conversions (algorithm/.../rng/Xoshiro256pp.hpp:22-96: splitmix64 seeding :33-39, next :41-52, 24 / 53 mantissa
// bits -> [0, 1) :55-61) and its Marsaglia-polar Gaussian with the cached second variate (GaussianNoise.hpp:33-55)
template <typename F>
struct Noise {
    std::uint64_t s[4]{};
    F             spare{};
    bool          has_spare = false;
    void          seed(std::uint64_t v) {
        for (auto& w : s) { // splitmix64
            v += 0x9e3779b97f4a7c15ULL;
            std::uint64_t z = v;
            z               = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
            z               = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
            w               = z ^ (z >> 31);
        }
        has_spare = false;
    }
    static constexpr std::uint64_t rotl(std::uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    std::uint64_t next() {
        const std::uint64_t r = rotl(s[0] + s[3], 23) + s[0], t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return r;
    }
    F u01() {
        if constexpr (std::is_same_v<F, float>) return static_cast<F>(next() >> 40) * F(0x1.0p-24);
        else return static_cast<F>(next() >> 11) * F(0x1.0p-53);
    }
    F um11() { return F(2) * u01() - F(1); }
    F triangular() { const F a = u01(), b = u01(); return a + b - F(1); }
    F gauss() {
        if (has_spare) { has_spare = false; return spare; }
        F u, v, q;
        do { u = um11(); v = um11(); q = u * u + v * v; } while (q >= F(1) || q == F(0));
        const F f = std::sqrt(F(-2) * std::log(q) / q);
        spare     = v * f;
        has_spare = true;
        return u * f;
    }
};
} // namespace signal_generator

// gr::basic::SignalGenerator<T> (blocks/basic/.../SignalGenerator.hpp:25-87) over SignalGeneratorCore<T> (algorithm/.../signal/SignalGeneratorCore.hpp:72-147),
// free-running with a sample budget instead of the wall-clock pacing.  All eleven signal types, sample by sample as the block does (generateSample):
//   tones (ToneGenerator.hpp): time accumulates by 1 / sample_rate in the compute type F (double for scalar T, the base type for complex T); Sin / Cos by
//   std::sin / std::cos of 2 pi f t + phase, FastSin / FastCos by a phasor rotated once per sample and renormalised every 65536 samples, Square / Saw /
//   Triangle from the cycle count f t + phase / 2 pi; frequency <= 0 turns every tone into Const; complex output = the analytic signal for the four
//   sinusoids (offset on the real part), {value, 0} otherwise
//   noise (NoiseGenerator.hpp): xoshiro256++ seeded with `seed`; Uniform [-1, 1), Triangular u1 + u2 - 1, Gaussian by Marsaglia's polar method; complex:
//   independent components (offset on the real part), Gaussian components scaled by 1 / sqrt 2
//   integer T: truncation, clamped to the type's range (clampToInt, SignalGeneratorCore.hpp:47-58)
template <typename T>
struct SignalGenerator : Block<SignalGenerator<T>> {
    using F = std::conditional_t<std::is_same_v<T, std::complex<float>>, float, double>;
    PortOut<T>             out;
    signal_generator::Type signal_type = signal_generator::Type::Sin;
    float                  sample_rate = 1000.f, frequency = 1.f, amplitude = 1.f, offset = 0.f, phase = 0.f;
    std::uint64_t          seed          = 0;
    Size_t                 n_samples_max = 0;
    std::size_t            _n            = 0;
    GR_MAKE_REFLECTABLE(SignalGenerator, out, signal_type, sample_rate, frequency, amplitude, offset, phase, seed, n_samples_max);

    // ---- the core's state
    signal_generator::Type     _type = signal_generator::Type::Sin;
    F                          _t = 0, _tick = 0, _omega = 0, _cycles0 = 0, _f = 1, _a = 1, _o = 0, _ph = 0;
    std::complex<F>            _phasor{1, 0}, _rot{1, 0};
    std::size_t                _count = 0;
    signal_generator::Noise<F> _noise;
    bool                       _configured = false;
    bool                       _device_configure = false, _device_reset = false; // compute_domain gpu:hip: what the device handle has not been told yet
    std::size_t                _device_calls = 0;

    void configure() {
        using signal_generator::Type;
        constexpr F pi2 = F(2) * std::numbers::pi_v<F>;
        _f = static_cast<F>(frequency); _a = static_cast<F>(amplitude); _o = static_cast<F>(offset); _ph = static_cast<F>(phase);
        _tick    = F(1) / static_cast<F>(sample_rate);
        _type    = signal_type;
        if (static_cast<int>(_type) <= static_cast<int>(Type::FastCos) && _f <= F(0)) _type = Type::Const;
        _omega   = pi2 * _f;
        _cycles0 = _ph / pi2;
        _rot     = {std::cos(pi2 * _f * _tick), std::sin(pi2 * _f * _tick)};
        _phasor  = {std::cos(_ph), std::sin(_ph)};
        _count   = 0;
        _noise.seed(seed);
        _configured = true;
        _device_configure = true;
    }
    void settingsChanged(const property_map&, const property_map&) { configure(); } // (the time base keeps running across a settings change, as upstream)
    void reset() { _t = 0; configure(); _device_reset = true; }
    [[nodiscard]] gr4hip_siggen_params params() const {
        int dtype = GR4HIP_F64;
        if constexpr (std::is_same_v<T, float>) dtype = GR4HIP_F32;
        else if constexpr (std::is_same_v<T, std::complex<float>>) dtype = GR4HIP_C32;
        else if constexpr (std::is_same_v<T, std::int16_t>) dtype = GR4HIP_I16;
        else if constexpr (!std::is_same_v<T, double>) dtype = -1; // no device implementation: gr4hip_siggen_check refuses it
        return gr4hip_siggen_params{dtype, static_cast<int>(signal_type), sample_rate, frequency, amplitude, offset, phase, seed};
    }

    [[nodiscard]] F tone() const {
        using signal_generator::Type;
        const F theta = _omega * _t + _ph, cycle = _f * _t + _cycles0;
        switch (_type) {
        case Type::Sin: return _a * std::sin(theta) + _o;
        case Type::Cos: return _a * std::cos(theta) + _o;
        case Type::FastSin: return _a * _phasor.imag() + _o;
        case Type::FastCos: return _a * _phasor.real() + _o;
        case Type::Square: return (cycle - std::floor(cycle) < F(0.5)) ? _a + _o : -_a + _o;
        case Type::Saw: return _a * (F(2) * (cycle - std::floor(cycle + F(0.5)))) + _o;
        case Type::Triangle: return _a * (F(4) * std::abs(cycle - std::floor(cycle + F(0.75)) + F(0.25)) - F(1)) + _o;
        default: return _a + _o;
        }
    }
    void advance() {
        using signal_generator::Type;
        _t += _tick;
        if (_type == Type::FastSin || _type == Type::FastCos) {
            _phasor *= _rot;
            if ((++_count & 0xFFFF) == 0) { const F inv = F(1) / std::abs(_phasor); _phasor = {_phasor.real() * inv, _phasor.imag() * inv}; }
        }
    }
    [[nodiscard]] F noise() {
        using signal_generator::Type;
        return _type == Type::UniformNoise ? _noise.um11() : _type == Type::TriangularNoise ? _noise.triangular() : _noise.gauss();
    }
    [[nodiscard]] T generateSample() {
        using signal_generator::Type;
        if (!_configured) configure();
        const bool is_tone = static_cast<int>(_type) <= static_cast<int>(Type::FastCos);
        if constexpr (gr::detail::is_complex<T>::value) {
            T r;
            if (is_tone) {
                const F theta = _omega * _t + _ph;
                switch (_type) {
                case Type::Sin: r = T(_a * std::sin(theta) + _o, -_a * std::cos(theta)); break;
                case Type::Cos: r = T(_a * std::cos(theta) + _o, _a * std::sin(theta)); break;
                case Type::FastSin: r = T(_a * _phasor.imag() + _o, -_a * _phasor.real()); break;
                case Type::FastCos: r = T(_a * _phasor.real() + _o, _a * _phasor.imag()); break;
                default: r = T(tone(), F(0)); break;
                }
                advance();
            } else if (_type == Type::GaussianNoise) {
                constexpr F scale = F(1) / std::numbers::sqrt2_v<F>;
                const F     g1 = _noise.gauss() * scale, g2 = _noise.gauss() * scale;
                r = T(_a * g1 + _o, _a * g2);
            } else {
                const F n1 = noise(), n2 = noise();
                r = T(_a * n1 + _o, _a * n2);
            }
            return r;
        } else {
            F raw;
            if (is_tone) { raw = tone(); advance(); }
            else raw = _a * noise() + _o;
            if constexpr (std::is_integral_v<T>) {
                if (raw >= static_cast<F>(std::numeric_limits<T>::max())) return std::numeric_limits<T>::max();
                if (raw <= static_cast<F>(std::numeric_limits<T>::min())) return std::numeric_limits<T>::min();
                return static_cast<T>(raw);
            } else {
                return static_cast<T>(raw);
            }
        }
    }

    work::Result customWork(std::size_t requested) {
        if (n_samples_max && _n >= n_samples_max) return {requested, 0, work::Status::DONE};
        if (!out.connected()) return {requested, 0, work::Status::ERROR};
        std::size_t n = std::min(out.buffer->free_space(), requested);
        if (n_samples_max) n = std::min<std::size_t>(n, n_samples_max - _n);
        if (n == 0) return {requested, 0, work::Status::INSUFFICIENT_OUTPUT_ITEMS};
        auto span = out.buffer->write_span(n);
        if (this->_domain.is_device()) { // the chunk is generated in HBM (gr4hip_siggen_process, gr4/hip.hpp) and copied to this edge: never a silent host fallback
            if constexpr (hip::HasKernel<SignalGenerator>) {
                if (hip::Kernel<SignalGenerator>::generate(*this, span.data(), n) != work::Status::OK) return {requested, 0, work::Status::ERROR};
            } else {
                this->_log("SignalGenerator: compute_domain '" + this->compute_domain + "' needs gr4/hip.hpp");
                return {requested, 0, work::Status::ERROR};
            }
        } else {
            for (std::size_t i = 0; i < n; ++i) span[i] = generateSample();
        }
        out.buffer->publish(n);
        _n += n;
        return {requested, n, work::Status::OK};
    }
};
} // namespace gr::basic

namespace gr::filter {

// gr::filter::fir_filter<T> (blocks/filter/.../time_domain_filter.hpp:22-48): setting `b`, y[n] = sum_k b[k] x[n-k], zero initial
// history.  T = float / double as registered upstream, plus std::complex<float> (complex data, real taps).
template <typename T>
struct fir_filter : Block<fir_filter<T>> {
    using tap_type = std::conditional_t<detail::is_complex<T>::value, float, T>;
    PortIn<T>             in;
    PortOut<T>            out;
    Tensor<tap_type>      b{tap_type(1)}; // feedforward coefficients: the reference's settings type (time_domain_filter.hpp:32); a std::vector in a property_map is accepted
    std::vector<T>        _history = std::vector<T>(32, T{}); // newest first, like HistoryBuffer{32}
    GR_MAKE_REFLECTABLE(fir_filter, in, out, b);

    void settingsChanged(const property_map& /*oldSettings*/, const property_map& newSettings) {
        if (newSettings.contains("b") && b.size() > _history.size()) { // the reference replaces the HistoryBuffer only when it must grow (:38-42)
            std::size_t cap = 1;
            while (cap < b.size()) cap <<= 1;
            _history.assign(cap, T{});
        }
    }
    [[nodiscard]] T processOne(T input) noexcept {
        std::move_backward(_history.begin(), _history.end() - 1, _history.end());
        _history[0] = input;
        T acc{};
        for (std::size_t k = 0; k < b.size(); ++k) acc += b[k] * _history[k];
        return acc;
    }
};

enum class IIRForm { DF_I, DF_II, DF_I_TRANSPOSED, DF_II_TRANSPOSED }; // time_domain_filter.hpp:50-55

// gr::filter::iir_filter<T, form> (time_domain_filter.hpp:62-122); a[0] is assumed to be 1
template <typename T, IIRForm form = IIRForm::DF_II>
struct iir_filter : Block<iir_filter<T, form>> {
    PortIn<T>      in;
    PortOut<T>     out;
    Tensor<T>      b{T(1)}, a{T(1)}; // time_domain_filter.hpp:73-74
    std::vector<T> _x = std::vector<T>(32, T{}), _y = std::vector<T>(32, T{});
    GR_MAKE_REFLECTABLE(iir_filter, in, out, b, a);

    static void push(std::vector<T>& h, T v) {
        std::move_backward(h.begin(), h.end() - 1, h.end());
        h[0] = v;
    }
    static T dot(const Tensor<T>& c, std::size_t first, const std::vector<T>& h) {
        T acc{};
        for (std::size_t k = first; k < c.size(); ++k) acc += c[k] * h[k - first];
        return acc;
    }
    void settingsChanged(const property_map&, const property_map&) {
        const std::size_t n = std::max(a.size(), b.size());
        if (n >= _x.size()) { _x.assign(2 * n, T{}); _y.assign(2 * n, T{}); }
    }
    [[nodiscard]] T processOne(T input) noexcept {
        if constexpr (form == IIRForm::DF_I) {
            push(_x, input);
            const T o = dot(b, 0, _x) - dot(a, 1, _y);
            push(_y, o);
            return o;
        } else if constexpr (form == IIRForm::DF_II) {
            const T w = input - dot(a, 1, _x);
            push(_x, w);
            return dot(b, 0, _x);
        } else if constexpr (form == IIRForm::DF_I_TRANSPOSED) {
            const T v0 = input - dot(a, 1, _y);
            push(_y, v0);
            return dot(b, 0, _y);
        } else {
            const T o = b[0] * input + dot(b, 1, _x) - dot(a, 1, _y);
            push(_x, input);
            push(_y, o);
            return o;
        }
    }
};

// gr::filter::Decimator<T> (time_domain_filter.hpp:215-245): keep every decim-th sample
template <typename T>
struct Decimator : Block<Decimator<T>, Resampling<1, 1, false>> {
    PortIn<T>  in;
    PortOut<T> out;
    Size_t     decim = 1;
    GR_MAKE_REFLECTABLE(Decimator, in, out, decim);
    void settingsChanged(const property_map&, const property_map&) { this->input_chunk_size = decim; }
    [[nodiscard]] work::Status processBulk(std::span<const T> input, std::span<T> output) noexcept {
        std::size_t o = 0;
        for (std::size_t i = 0; i < input.size(); ++i)
            if (i % decim == 0) output[o++] = input[i];
        return work::Status::OK;
    }
};

// ---- BasicFilterProto<T, Args...> (time_domain_filter.hpp:126-210): FIR / IIR by specification, optionally decimating
enum class FilterType { FIR, IIR };                                   // time_domain_filter.hpp:127
enum class Type { LOWPASS, HIGHPASS, BANDPASS, BANDSTOP };            // filter::Type (FilterTool.hpp:64) == gr4hip_filter_response
namespace iir { enum class Design { BUTTERWORTH, BESSEL, CHEBYSHEV1, CHEBYSHEV2 }; // FilterTool.hpp:425-430 == gr4hip_iir_design_t
inline bool gr_enum_parse(Design& d, std::string_view s) { return gr::detail::enum_from_names(d, s, std::array<std::string_view, 4>{"BUTTERWORTH", "BESSEL", "CHEBYSHEV1", "CHEBYSHEV2"}); }
}
inline bool gr_enum_parse(FilterType& d, std::string_view s) { return gr::detail::enum_from_names(d, s, std::array<std::string_view, 2>{"FIR", "IIR"}); }
inline bool gr_enum_parse(Type& d, std::string_view s) { return gr::detail::enum_from_names(d, s, std::array<std::string_view, 4>{"LOWPASS", "HIGHPASS", "BANDPASS", "BANDSTOP"}); }

// FrequencyEstimatorTimeDomain<float, Args...> / FrequencyEstimatorFrequencyDomain<float, Args...> (blocks/filter/.../FrequencyEstimator.hpp:30-351): the settings
// and their checks (settingsChanged :62-69, :222-229).  Device-only: the estimates are computed behind compute_domain gpu:hip (gr4hip_freqest_*, gr4/hip.hpp); the
// host processBulk refuses loudly (work::Status::ERROR).  One output per input chunk: 1 without resampling (processOne), 10 for ...Decimating (Resampling<10U>, :179), N for the
// frequency-domain decimating form (initialiseFFT sets input_chunk_size = N, :231-242).
inline void frequency_estimator_check(float fs, float fmin, float fexp, float fmax) { // (:63-66)
    if (fmin < 0.f || fmax >= fs / 2.f || fexp < 0.f || fexp >= fs / 2.f)
        throw std::invalid_argument("Ill-formed block parameters: f_min < f_expected < f_max < sample_rate/2 (Nyquist limit) violated");
}

template <typename T, typename... Args>
    requires std::floating_point<T>
struct FrequencyEstimatorTimeDomain : Block<FrequencyEstimatorTimeDomain<T, Args...>, Args...> {
    using TParent = Block<FrequencyEstimatorTimeDomain<T, Args...>, Args...>;
    PortIn<T>  in;
    PortOut<T> out;
    float      sample_rate = 1e3f, f_min = 40.f, f_expected = 50.f, f_max = 60.f; // (:46-51)
    Size_t     n_periods = 4U;
    T          epsilon   = T(1e-8);
    GR_MAKE_REFLECTABLE(FrequencyEstimatorTimeDomain, in, out, sample_rate, f_expected, f_min, f_max, n_periods, epsilon);
    void settingsChanged(const property_map&, const property_map&) { frequency_estimator_check(sample_rate, f_min, f_expected, f_max); }
    [[nodiscard]] std::size_t chunk() const { return TParent::ResamplingControl::kEnabled ? std::max<std::size_t>(1, this->input_chunk_size) : 1; }
    work::Status processBulk(std::span<const T>, std::span<T>) { // (the graph ends with ERROR: no numbers come out of the host path)
        std::fprintf(stderr, "FrequencyEstimatorTimeDomain: device-only block, needs compute_domain gpu:hip\n");
        return work::Status::ERROR;
    }
};
template <typename T>
using FrequencyEstimatorTimeDomainDecimating = FrequencyEstimatorTimeDomain<T, Resampling<10U>>;

template <typename T, typename... Args>
    requires std::floating_point<T>
struct FrequencyEstimatorFrequencyDomain : Block<FrequencyEstimatorFrequencyDomain<T, Args...>, Args...> {
    using TParent = Block<FrequencyEstimatorFrequencyDomain<T, Args...>, Args...>;
    PortIn<T>  in;
    PortOut<T> out;
    float      sample_rate = 1e3f, f_min = 40.f, f_expected = 50.f, f_max = 60.f; // (:202-207)
    Size_t     min_fft_size = 256U;
    T          epsilon      = T(1e-8);
    GR_MAKE_REFLECTABLE(FrequencyEstimatorFrequencyDomain, in, out, sample_rate, f_expected, f_min, f_max, min_fft_size, epsilon);
    void settingsChanged(const property_map&, const property_map&) {
        frequency_estimator_check(sample_rate, f_min, f_expected, f_max);
        if constexpr (TParent::ResamplingControl::kEnabled && !TParent::ResamplingControl::kIsConst) { // initialiseFFT (:231-242): the chunk is N
            gr4hip_freqest_params p{sample_rate, f_min, f_expected, f_max, static_cast<float>(epsilon), 1, min_fft_size, 1};
            std::size_t N = 0;
            if (gr4hip_freqest_geometry(GR4HIP_FREQEST_FREQUENCY_DOMAIN, &p, &N, nullptr, nullptr) != GR4HIP_OK) throw std::invalid_argument(std::string("FrequencyEstimatorFrequencyDomain: ") + gr4hip_last_error());
            this->input_chunk_size = static_cast<Size_t>(N);
        }
    }
    [[nodiscard]] std::size_t chunk() const { return TParent::ResamplingControl::kEnabled ? std::max<std::size_t>(1, this->input_chunk_size) : 1; }
    work::Status processBulk(std::span<const T>, std::span<T>) { // (the graph ends with ERROR: no numbers come out of the host path)
        std::fprintf(stderr, "FrequencyEstimatorFrequencyDomain: device-only block, needs compute_domain gpu:hip\n");
        return work::Status::ERROR;
    }
};
// the registered decimating form says Resampling<10U>, but initialiseFFT overrides the chunk with N
template <typename T>
using FrequencyEstimatorFrequencyDomainDecimating = FrequencyEstimatorFrequencyDomain<T, Resampling<10U>>;

// IQDemodulator<T, Args...> (blocks/filter/.../FrequencyEstimator.hpp:356-653): a lock-in amplifier with two inputs (ref, resp) and three outputs (amplitude,
// phase, frequency), one output per input chunk.  Device-only: computed behind compute_domain gpu:hip (gr4hip_iqdemod_*, gr4/hip.hpp); off the device the work
// loop refuses loudly (deviceOnly: work::Status::ERROR).  A settings update that names sample_rate, f_high_pass, f_low_pass or derivative_method re-initialises
// the filters (settingsChanged, :454-466); with Derivative<M, true> an update that names derivative_method throws (:455-459).
enum class PhaseUnit : int { Radians = 0, Degrees = 1 };
enum class DerivativeMethod : int { SymmetricDifference = 0, SavitzkyGolay5 = 1, SavitzkyGolay7 = 2 };
inline bool gr_enum_parse(PhaseUnit& d, std::string_view s) { return gr::detail::enum_from_names(d, s, std::array<std::string_view, 2>{"Radians", "Degrees"}); }
inline bool gr_enum_parse(DerivativeMethod& d, std::string_view s) {
    return gr::detail::enum_from_names(d, s, std::array<std::string_view, 3>{"SymmetricDifference", "SavitzkyGolay5", "SavitzkyGolay7"});
}
template <DerivativeMethod method = DerivativeMethod::SymmetricDifference, bool isConst = false>
struct Derivative {
    static constexpr DerivativeMethod kMethod  = method;
    static constexpr bool             kIsConst = isConst;
};
namespace detail {
template <typename T>
struct is_derivative : std::false_type {};
template <DerivativeMethod M, bool C>
struct is_derivative<Derivative<M, C>> : std::true_type {};
template <typename... Args>
struct find_derivative {
    using type = Derivative<>;
};
template <typename A, typename... R>
struct find_derivative<A, R...> {
    using type = std::conditional_t<is_derivative<A>::value, A, typename find_derivative<R...>::type>;
};
} // namespace detail

template <typename T, typename... Args>
    requires std::floating_point<T>
struct IQDemodulator : Block<IQDemodulator<T, Args...>, Args...> {
    using TParent           = Block<IQDemodulator<T, Args...>, Args...>;
    using DerivativeControl = typename detail::find_derivative<Args...>::type;
    PortIn<T>        ref, resp;
    PortOut<T>       amplitude, phase, frequency;
    float            sample_rate = 62.5e6f, f_high_pass = 100.f, f_low_pass = 10000.f; // (:423-429)
    PhaseUnit        phase_unit        = PhaseUnit::Radians;
    bool             invert_phase      = false;
    DerivativeMethod derivative_method = DerivativeControl::kMethod;
    T                epsilon           = T(1e-12);
    bool             _filters_changed  = false; // an update named a filter key since the device handle last took the settings
    GR_MAKE_REFLECTABLE(IQDemodulator, ref, resp, amplitude, phase, frequency, sample_rate, f_high_pass, f_low_pass, phase_unit, invert_phase, derivative_method, epsilon);
    void settingsChanged(const property_map&, const property_map& newSettings) {
        if constexpr (DerivativeControl::kIsConst) {
            if (newSettings.contains("derivative_method")) throw std::invalid_argument("derivative_method is compile-time fixed and cannot be changed at runtime");
        }
        if (newSettings.contains("sample_rate") || newSettings.contains("f_high_pass") || newSettings.contains("f_low_pass") || newSettings.contains("derivative_method")) {
            if (f_high_pass <= 0.f || f_low_pass <= 0.f || f_high_pass >= f_low_pass || f_low_pass >= sample_rate / 2.f)
                throw std::invalid_argument("invalid filter frequencies: 0 < f_hp < f_lp < fs/2 violated");
            _filters_changed = true;
        }
    }
    [[nodiscard]] std::size_t chunk() const { return TParent::ResamplingControl::kEnabled ? std::max<std::size_t>(1, this->input_chunk_size) : 1; }
    work::Status deviceOnly() { // (the graph ends with ERROR: no numbers come out of the host path)
        std::fprintf(stderr, "IQDemodulator: device-only block, needs compute_domain gpu:hip\n");
        this->_log("IQDemodulator: device-only block, needs compute_domain gpu:hip");
        return work::Status::ERROR;
    }
};
template <typename T>
using IQDemodulatorDecimating = IQDemodulator<T, Resampling<1024U, 1U, false>>;
template <typename T, DerivativeMethod M>
using IQDemodulatorFixed = IQDemodulator<T, Resampling<1024U, 1U, false>, Derivative<M, true>>;

GR_REGISTER_BLOCK(gr::filter::SvdDenoiser, [T], [ float, double, std::complex<float>, std::complex<double> ])
// SvdDenoiser<T> (blocks/filter/.../SvdDenoiser.hpp:14-91): Hankel-SVD low-rank denoising, one output per input.  Members, names, defaults and the reflected set
// are the reference's (:34-53).  Device-only: the windows are decomposed behind compute_domain gpu:hip (gr4hip_svddenoise_*, gr4/hip.hpp, SVD_DENOISER.md); off
// the device the work loop refuses loudly.  Any update that names one of the seven settings is setParameters (:76-86), which resets the stream's history; what
// gr4hip_svddenoise_check refuses is refused here, and a window beyond the device kernel's limits fails the work loop (GR4HIP_UNSUPPORTED), never a host path.
template <typename T>
    requires(std::floating_point<T> || std::is_same_v<T, std::complex<float>> || std::is_same_v<T, std::complex<double>>)
struct SvdDenoiser : Block<SvdDenoiser<T>> {
    using RealT = std::conditional_t<std::is_same_v<T, float> || std::is_same_v<T, std::complex<float>>, float, double>;

    PortIn<T>  in;
    PortOut<T> out;

    Annotated<gr::Size_t, "window size", Doc<"analysis window size (samples)">>                   window_size = 64U;
    Annotated<gr::Size_t, "Hankel rows", Doc<"number of Hankel matrix rows (0 = window_size/2)">> hankel_rows = 0U;
    Annotated<gr::Size_t, "max rank", Doc<"maximum singular values to keep (max = no limit)">>    max_rank    = std::numeric_limits<gr::Size_t>::max();
    Annotated<RealT, "relative threshold", Doc<"minimum ratio sigma_i/sigma_0 to keep">, Unit<"ratio">>             relative_threshold = std::numeric_limits<RealT>::epsilon();
    Annotated<RealT, "absolute threshold", Doc<"minimum absolute value of sigma_i to keep">>                        absolute_threshold = std::numeric_limits<RealT>::epsilon();
    Annotated<RealT, "energy fraction", Doc<"fraction of total energy to retain (1.0 = all)">, Unit<"ratio">>       energy_fraction    = RealT{1};
    Annotated<RealT, "hop fraction", Doc<"SVD recomputation interval as fraction of window_size">, Unit<"ratio">>   hop_fraction       = RealT{0.25};

    GR_MAKE_REFLECTABLE(SvdDenoiser, in, out, window_size, hankel_rows, max_rank, relative_threshold, absolute_threshold, energy_fraction, hop_fraction);

    bool        _parameters_changed = false; // an update named a setting since the device handle last took them: setParameters, a reset (:76-86)
    std::size_t _device_calls       = 0;     // chunks handed to the device

    void settingsChanged(const property_map&, const property_map& newSettings) {
        if (newSettings.contains("window_size") || newSettings.contains("hankel_rows") || newSettings.contains("max_rank") || newSettings.contains("relative_threshold") ||
            newSettings.contains("absolute_threshold") || newSettings.contains("energy_fraction") || newSettings.contains("hop_fraction")) {
            // what gr4hip_svddenoise_check refuses (include/gr4hip.h), said here so that a program that only holds the block needs no library
            const double rel = static_cast<double>(relative_threshold.value), ab = static_cast<double>(absolute_threshold.value);
            const double ef = static_cast<double>(energy_fraction.value), hf = static_cast<double>(hop_fraction.value);
            const std::size_t W = std::max<std::size_t>(window_size.value, 2);
            if (!(std::isfinite(rel) && rel >= 0.0 && std::isfinite(ab) && ab >= 0.0 && std::isfinite(ef) && std::isfinite(hf) && hf >= 0.0 && hf <= 1.0 && hankel_rows.value <= W))
                throw std::invalid_argument("SvdDenoiser: thresholds must be finite and not negative, energy_fraction finite, hop_fraction in [0, 1], hankel_rows <= window_size");
            _parameters_changed = true;
        }
    }
    [[nodiscard]] gr4hip_svddenoise_params params() const {
        constexpr int dtype = std::is_same_v<T, float> ? GR4HIP_F32 : std::is_same_v<T, double> ? GR4HIP_F64 : std::is_same_v<T, std::complex<float>> ? GR4HIP_C32 : GR4HIP_C64;
        return {dtype, static_cast<std::size_t>(window_size.value), static_cast<std::size_t>(hankel_rows.value), static_cast<std::uint64_t>(max_rank.value),
                static_cast<double>(relative_threshold.value), static_cast<double>(absolute_threshold.value), static_cast<double>(energy_fraction.value),
                static_cast<double>(hop_fraction.value)};
    }
    work::Status processBulk(std::span<const T>, std::span<T>) { // (the graph ends with ERROR: nothing comes out of the host path)
        std::fprintf(stderr, "SvdDenoiser: device-only block, needs compute_domain gpu:hip\n");
        this->_log("SvdDenoiser: device-only block, needs compute_domain gpu:hip");
        return work::Status::ERROR;
    }
};

// ---- Savitzky-Golay (blocks/filter/.../SavitzkyGolayFilter.hpp:17-164 over algorithm/filter/SavitzkyGolay.hpp).  Members, names, defaults and the reflected sets are
// the reference's.  The coefficients come from gr4hip_savgol_design (host code of libgr4hip.so, like the filter design behind BasicFilter: the float design keeps
// the reference's truncated pseudo-inverse, SAVITZKY_GOLAY.md); the host bodies are the reference's plain loops in T, the device paths are in gr4/hip.hpp.
namespace savitzky_golay {
template <typename T>
[[nodiscard]] inline std::vector<T> design(std::size_t window_size, std::size_t poly_order, std::size_t deriv_order, T delta, bool causal) { // computeCoefficients<T> (:93-151)
    std::vector<T> c(std::max<std::size_t>(window_size, 1));
    const int      rc = gr4hip_savgol_design(std::is_same_v<T, float> ? GR4HIP_F32 : GR4HIP_F64, window_size, poly_order, deriv_order, static_cast<double>(delta),
                                             causal ? GR4HIP_SAVGOL_CAUSAL : GR4HIP_SAVGOL_CENTRED, c.data(), nullptr);
    if (rc != GR4HIP_OK) throw std::invalid_argument(std::string("Savitzky-Golay design: ") + gr4hip_last_error());
    return c;
}
[[nodiscard]] constexpr std::size_t reflectIndex(std::ptrdiff_t i, std::size_t N) noexcept { // (:51-64)
    if (N == 0) return 0;
    if (i < 0) i = -i - 1;
    const auto period = static_cast<std::ptrdiff_t>(2 * N);
    i %= period;
    if (i >= static_cast<std::ptrdiff_t>(N)) i = period - i - 1;
    return static_cast<std::size_t>(i);
}
[[nodiscard]] constexpr std::size_t replicateIndex(std::ptrdiff_t i, std::size_t N) noexcept { // (:66-77)
    if (N == 0 || i < 0) return 0;
    return i >= static_cast<std::ptrdiff_t>(N) ? N - 1 : static_cast<std::size_t>(i);
}
template <typename T>
inline void apply(std::span<const T> in, std::span<T> out, std::span<const T> coeffs, bool replicate) { // apply (:156-172), Centred
    const std::size_t N = in.size(), W = coeffs.size();
    if (N == 0 || W == 0 || out.size() < N) return;
    const auto D = static_cast<std::ptrdiff_t>((W - 1) / 2);
    for (std::size_t n = 0; n < N; ++n) {
        T acc{0};
        for (std::size_t k = 0; k < W; ++k) {
            const auto idx = static_cast<std::ptrdiff_t>(n) + static_cast<std::ptrdiff_t>(k) - D;
            acc += coeffs[k] * in[replicate ? replicateIndex(idx, N) : reflectIndex(idx, N)];
        }
        out[n] = acc;
    }
}
template <typename T>
inline void applyZeroPhase(std::span<const T> in, std::span<T> out, std::span<const T> coeffs, bool replicate) { // (:177-193)
    const std::size_t N = in.size();
    if (N == 0 || coeffs.empty() || out.size() < N) return;
    std::vector<T> temp(N), temp2(N);
    apply<T>(in, temp, coeffs, replicate);
    std::reverse(temp.begin(), temp.end());
    apply<T>(std::span<const T>(temp), temp2, coeffs, replicate);
    std::reverse(temp2.begin(), temp2.end());
    std::copy(temp2.begin(), temp2.end(), out.begin());
}
} // namespace savitzky_golay

GR_REGISTER_BLOCK(gr::filter::SavitzkyGolayFilter, [T], [ float, double ])
// SavitzkyGolayFilter<T> (:17-81): y[n] = sum_k c[k] x[n - (W - 1) + k] over a history of zeros (SavitzkyGolay.hpp:226-233, BoundaryPolicy::Default with value 0).
// Any update that names one of the five settings is setParameters (:67-76, SavitzkyGolay.hpp:253-260): new coefficients AND an empty history.
template <typename T>
    requires std::floating_point<T>
struct SavitzkyGolayFilter : Block<SavitzkyGolayFilter<T>> {
    PortIn<T>  in;
    PortOut<T> out;

    Annotated<gr::Size_t, "window size", Doc<"filter window size (samples, must be >= poly_order+1)">> window_size = 11U;
    Annotated<gr::Size_t, "polynomial order", Doc<"order of fitting polynomial">>                      poly_order  = 4U;
    Annotated<gr::Size_t, "derivative order", Doc<"derivative order (0=smooth, 1=1st deriv, ...)">>    deriv_order = 0U;
    Annotated<float, "sample rate", Doc<"input sample rate for derivative scaling">, Unit<"Hz">>       sample_rate = 1.0f;
    Annotated<std::string, "alignment", Doc<"Centred or Causal">>                                      alignment   = std::string("Centred");

    GR_MAKE_REFLECTABLE(SavitzkyGolayFilter, in, out, window_size, poly_order, deriv_order, sample_rate, alignment);

    std::vector<T> _coeffs, _history;           // the history oldest first, as HistoryBuffer::push_back leaves it
    bool           _parameters_changed = false; // an update named a setting since the device stage was made: setParameters, i.e. a reset

    [[nodiscard]] bool causal() const { return alignment.value == "Causal"; } // anything else is Centred (:53-55)
    [[nodiscard]] T    delta() const {                                        // (:49-52)
        const T sampleRateT = static_cast<T>(sample_rate.value);
        return sampleRateT > T{0} ? T{1} / sampleRateT : T{1};
    }
    [[nodiscard]] std::vector<T> designCoefficients() const { return savitzky_golay::design<T>(window_size.value, poly_order.value, deriv_order.value, delta(), causal()); }
    void start() { // (:60-65)
        _coeffs = designCoefficients();
        _history.assign(_coeffs.size(), T{0});
    }
    void settingsChanged(const property_map&, const property_map& newSettings) {
        if (newSettings.contains("window_size") || newSettings.contains("poly_order") || newSettings.contains("deriv_order") || newSettings.contains("sample_rate") ||
            newSettings.contains("alignment")) {
            _parameters_changed = true;
            _coeffs.clear(); // designed at the next sample (the host body) or stage (the device path): a program that only holds the block needs no library
        }
    }
    void reset() { _history.assign(_history.size(), T{0}); } // (:78)
    [[nodiscard]] T processOne(T input) {
        if (_coeffs.empty()) start();
        std::move(_history.begin() + 1, _history.end(), _history.begin());
        _history.back() = input;
        T acc{0};
        for (std::size_t k = 0; k < _coeffs.size(); ++k) acc += _history[k] * _coeffs[k];
        return acc;
    }
};

GR_REGISTER_BLOCK(gr::filter::SavitzkyGolayDataSetFilter, [T], [ float, double ])
// SavitzkyGolayDataSetFilter<T> (:87-164): zero-phase filtering of the whole flat signal_values as ONE sequence (:154-161), everything else of the DataSet passed
// through; an empty signal_values comes back unchanged (:150-152).  Always Centred with delta 1 (:121-130).
template <typename T>
    requires std::floating_point<T>
struct SavitzkyGolayDataSetFilter : Block<SavitzkyGolayDataSetFilter<T>> {
    PortIn<DataSet<T>>  in;
    PortOut<DataSet<T>> out;

    Annotated<gr::Size_t, "window size", Doc<"filter window size (samples, must be >= poly_order+1)">> window_size     = 11U;
    Annotated<gr::Size_t, "polynomial order", Doc<"order of fitting polynomial">>                      poly_order      = 4U;
    Annotated<gr::Size_t, "derivative order", Doc<"derivative order (0=smooth, 1=1st deriv, ...)>">>   deriv_order     = 0U;
    Annotated<std::string, "boundary policy", Doc<"Reflect or Replicate">>                             boundary_policy = std::string("Reflect");

    GR_MAKE_REFLECTABLE(SavitzkyGolayDataSetFilter, in, out, window_size, poly_order, deriv_order, boundary_policy);

    std::vector<T> _coeffs;
    bool           _parameters_changed = false;

    [[nodiscard]] bool replicate() const { return boundary_policy.value == "Replicate"; } // anything else is Reflect (:126-128)
    void               start() { _coeffs = savitzky_golay::design<T>(window_size.value, poly_order.value, deriv_order.value, T{1}, false); } // (:132-140)
    void               settingsChanged(const property_map&, const property_map& newSettings) {
        if (newSettings.contains("window_size") || newSettings.contains("poly_order") || newSettings.contains("deriv_order") || newSettings.contains("boundary_policy")) {
            _parameters_changed = true;
            _coeffs.clear();
        }
    }
    [[nodiscard]] gr4hip_savgol_zp_params params() const {
        return {std::is_same_v<T, float> ? GR4HIP_F32 : GR4HIP_F64, static_cast<std::size_t>(window_size.value), static_cast<std::size_t>(poly_order.value),
                static_cast<std::size_t>(deriv_order.value), replicate() ? GR4HIP_SAVGOL_REPLICATE : GR4HIP_SAVGOL_REFLECT};
    }
    [[nodiscard]] DataSet<T> processOne(DataSet<T> input) {
        if (input.signal_values.empty()) return input;
        if (_coeffs.empty()) start();
        std::vector<T> filtered(input.signal_values.size());
        savitzky_golay::applyZeroPhase<T>(std::span<const T>(input.signal_values), std::span<T>(filtered), std::span<const T>(_coeffs), replicate());
        input.signal_values = std::move(filtered);
        return input;
    }
};
} // namespace gr::filter
namespace gr::electrical {
namespace detail {
template <typename P>
std::span<typename P::value_type> electrical_out_span(P& port, std::size_t n, std::vector<typename P::value_type>& scratch) { // an unconnected port computes into scratch
    if (port.connected()) return port.buffer->write_span(n);
    scratch.resize(n);
    return scratch;
}
} // namespace detail
GR_REGISTER_BLOCK("gr::electrical::ThreePhasePowerMetrics", gr::electrical::PowerMetrics, ([T], 3UZ), [ float ])
GR_REGISTER_BLOCK("gr::electrical::SinglePhasePowerMetrics", gr::electrical::PowerMetrics, ([T], 1UZ), [ float ])
// PowerMetrics<T, nPhases> (blocks/electrical/.../PowerEstimators.hpp:21-131): per phase a voltage and a current input; active, reactive and apparent power and
// the two RMS values, one output per chunk of `decimate` inputs.  Members, names and the reflected set are the reference's (:36-51: high_pass and low_pass are
// public but not reflected).  Device-only: computed behind compute_domain gpu:hip (gr4hip_powermetrics_*, gr4/hip.hpp); off the device the work loop refuses
// loudly (deviceOnly: work::Status::ERROR).  Every settings update rebuilds the filters (:95) and sets input_chunk_size = decimate (:79-81).
template <typename T, std::size_t nPhases>
    requires std::floating_point<T>
struct PowerMetrics : Block<PowerMetrics<T, nPhases>, Resampling<100U, 1U, false>> {
    using TParent = Block<PowerMetrics<T, nPhases>, Resampling<100U, 1U, false>>;
    std::vector<PortIn<T>>  U{nPhases};
    std::vector<PortIn<T>>  I{nPhases};
    std::vector<PortOut<T>> P{nPhases};     // active power (in-phase)
    std::vector<PortOut<T>> Q{nPhases};     // reactive power
    std::vector<PortOut<T>> S{nPhases};     // apparent power
    std::vector<PortOut<T>> U_rms{nPhases};
    std::vector<PortOut<T>> I_rms{nPhases};
    float      sample_rate = 10000.f, high_pass = 2.f, low_pass = 90.f; // (:46-48)
    gr::Size_t decimate    = 100U;                                      // (:49)
    gr::Size_t _decimate_in_force = 100U; // the last accepted value: a refused update leaves the block as it was
    GR_MAKE_REFLECTABLE(PowerMetrics, U, I, P, Q, S, U_rms, I_rms, sample_rate, decimate);
    void settingsChanged(const property_map&, const property_map&) {
        if (decimate == 0U) {
            decimate = _decimate_in_force;
            throw std::invalid_argument("decimate must be at least 1");
        }
        _decimate_in_force     = decimate;
        this->input_chunk_size = decimate; // initFilters (:79-81); the device handle rebuilds its filters on the new settings generation
    }
    work::Status deviceOnly() { // (the graph ends with ERROR: no numbers come out of the host path)
        std::fprintf(stderr, "PowerMetrics: device-only block, needs compute_domain gpu:hip\n");
        this->_log("PowerMetrics: device-only block, needs compute_domain gpu:hip");
        return work::Status::ERROR;
    }
};
template <typename T>
using ThreePhasePowerMetrics = PowerMetrics<T, 3U>;
template <typename T>
using SinglePhasePowerMetrics = PowerMetrics<T, 1U>;

GR_REGISTER_BLOCK("gr::electrical::SinglePhasePowerFactorCalculator", gr::electrical::PowerFactor, ([T], 1UZ), [ float, double ])
GR_REGISTER_BLOCK("gr::electrical::ThreePhasePowerFactorCalculator", gr::electrical::PowerFactor, ([T], 3UZ), [ float, double ])
// PowerFactor<T, nPhases> (blocks/electrical/.../PowerEstimators.hpp:144-182): per phase cos(phi) = P / S clamped to [-1, 1] and phi = acos of it.  Ports and names
// are the reference's.  The arithmetic is gr4/electrical_ops.hpp, the device kernels' own (csrc/electrical.hip): host and device agree bit for bit on
// power_factor; phase is std::acos in T here, like the reference (POWER_QUALITY.md).  The gr::UncertainValue<T> instantiations are left out, as for PowerMetrics.
template <typename T, std::size_t nPhases>
    requires std::floating_point<T>
struct PowerFactor : Block<PowerFactor<T, nPhases>> {
    std::vector<PortIn<T>>  P{nPhases}; // active power
    std::vector<PortIn<T>>  S{nPhases}; // apparent power
    std::vector<PortOut<T>> power_factor{nPhases};
    std::vector<PortOut<T>> phase{nPhases};
    GR_MAKE_REFLECTABLE(PowerFactor, P, S, power_factor, phase);
    work::Status processBulk(std::span<const std::span<const T>> pIn, std::span<const std::span<const T>> sIn, std::span<const std::span<T>> powerFactorOut,
                             std::span<const std::span<T>> phaseAngle) { // (:161-181)
        namespace ops = gr4::electrical_ops;
        for (std::size_t phaseIdx = 0; phaseIdx < nPhases; ++phaseIdx) {
            for (std::size_t n = 0; n < pIn[phaseIdx].size(); ++n) {
                const T cos_phi             = ops::power_factor<T>(pIn[phaseIdx][n], sIn[phaseIdx][n]);
                powerFactorOut[phaseIdx][n] = cos_phi;
                phaseAngle[phaseIdx][n]     = ops::acos_of(cos_phi);
            }
        }
        return work::Status::OK;
    }
    work::Status hostWork(std::size_t nIn, std::size_t nOut) {
        std::vector<std::span<const T>> p, s;
        std::vector<std::span<T>>       f, a;
        std::vector<std::vector<T>>     scratch(2 * nPhases);
        for (std::size_t k = 0; k < nPhases; ++k) {
            p.push_back(P[k].buffer->read_span(nIn));
            s.push_back(S[k].buffer->read_span(nIn));
            f.push_back(detail::electrical_out_span(power_factor[k], nOut, scratch[2 * k]));
            a.push_back(detail::electrical_out_span(phase[k], nOut, scratch[2 * k + 1]));
        }
        return processBulk(p, s, f, a);
    }
};
template <typename T>
using SinglePhasePowerFactorCalculator = PowerFactor<T, 1>;
template <typename T>
using ThreePhasePowerFactorCalculator = PowerFactor<T, 3>;

GR_REGISTER_BLOCK("gr::electrical::TwoPhaseSystemUnbalanceCalculator", gr::electrical::SystemUnbalance, ([T], 2UZ), [ float, double ])
GR_REGISTER_BLOCK("gr::electrical::ThreePhaseSystemUnbalanceCalculator", gr::electrical::SystemUnbalance, ([T], 3UZ), [ float, double ])
// SystemUnbalance<T, nPhases> (:193-257): the total active power and the voltage and current unbalance (largest deviation from the phases' average, in percent of
// it) of a multi-phase system.  Ports and names are the reference's; the arithmetic is gr4/electrical_ops.hpp, which keeps the reference's two different
// reductions (std::transform_reduce / std::max for the voltage, std::max_element for the current): host and device agree bit for bit on all three outputs.
template <typename T, std::size_t nPhases>
    requires(std::floating_point<T> && (nPhases > 1)) // unbalance calculation requires at least two phases
struct SystemUnbalance : Block<SystemUnbalance<T, nPhases>> {
    std::vector<PortIn<T>> voltage_rms_inputs{nPhases};  // U_rms_in
    std::vector<PortIn<T>> current_rms_inputs{nPhases};  // I_rms_in
    std::vector<PortIn<T>> active_power_inputs{nPhases}; // P_in
    PortOut<T>             total_active_power_output;    // P_total_out
    PortOut<T>             voltage_unbalance_output;     // U_unbalance_out
    PortOut<T>             current_unbalance_output;     // I_unbalance_out
    GR_MAKE_REFLECTABLE(SystemUnbalance, voltage_rms_inputs, current_rms_inputs, active_power_inputs, total_active_power_output, voltage_unbalance_output, current_unbalance_output);
    work::Status processBulk(std::span<const std::span<const T>> rmsUIn, std::span<const std::span<const T>> rmsIIn, std::span<const std::span<const T>> PIn,
                             std::span<T> totalP, std::span<T> unbalancedU, std::span<T> unbalancedI) { // (:217-256)
        namespace ops = gr4::electrical_ops;
        constexpr int N = static_cast<int>(nPhases);
        for (std::size_t n = 0; n < rmsUIn[0].size(); ++n) {
            totalP[n]      = ops::sum_of<T>([&](int i) { return PIn[static_cast<std::size_t>(i)][n]; }, N);
            unbalancedU[n] = ops::voltage_unbalance<T>([&](int i) { return rmsUIn[static_cast<std::size_t>(i)][n]; }, N);
            unbalancedI[n] = ops::current_unbalance<T>([&](int i) { return rmsIIn[static_cast<std::size_t>(i)][n]; }, N);
        }
        return work::Status::OK;
    }
    work::Status hostWork(std::size_t nIn, std::size_t nOut) {
        std::vector<std::span<const T>> u, c, p;
        std::vector<T>                  s0, s1, s2;
        for (std::size_t k = 0; k < nPhases; ++k) {
            u.push_back(voltage_rms_inputs[k].buffer->read_span(nIn));
            c.push_back(current_rms_inputs[k].buffer->read_span(nIn));
            p.push_back(active_power_inputs[k].buffer->read_span(nIn));
        }
        return processBulk(u, c, p, detail::electrical_out_span(total_active_power_output, nOut, s0), detail::electrical_out_span(voltage_unbalance_output, nOut, s1),
                           detail::electrical_out_span(current_unbalance_output, nOut, s2));
    }
};
template <typename T>
using TwoPhaseSystemUnbalanceCalculator = SystemUnbalance<T, 2>;
template <typename T>
using ThreePhaseSystemUnbalanceCalculator = SystemUnbalance<T, 3>;
} // namespace gr::electrical
namespace gr::trigger {
enum class InterpolationMethod : int { NO_INTERPOLATION = 0, BASIC_LINEAR_INTERPOLATION = 1, LINEAR_INTERPOLATION = 2, POLYNOMIAL_INTERPOLATION = 3 }; // SchmittTrigger.hpp:17-22
enum class EdgeDetection : int { NONE = 0, RISING = 1, FALLING = 2 };                                                                                // (:24)
} // namespace gr::trigger
namespace gr::blocks::basic {
GR_REGISTER_BLOCK("gr::blocks::basic::SchmittTriggerNoInterpolation", gr::blocks::basic::SchmittTrigger, ([T], gr::trigger::InterpolationMethod::NO_INTERPOLATION), [ std::int16_t, std::int32_t, float, double ])
GR_REGISTER_BLOCK("gr::blocks::basic::SchmittTriggerBasic", gr::blocks::basic::SchmittTrigger, ([T], gr::trigger::InterpolationMethod::BASIC_LINEAR_INTERPOLATION), [ std::int16_t, std::int32_t, float, double ])
GR_REGISTER_BLOCK("gr::blocks::basic::SchmittTrigger", gr::blocks::basic::SchmittTrigger, ([T], gr::trigger::InterpolationMethod::LINEAR_INTERPOLATION), [ std::int16_t, std::int32_t, float, double ])
// SchmittTrigger<T, Method> (blocks/basic/.../Trigger.hpp:16-164): passes its samples through and publishes a tag {trigger_name, trigger_time,
// trigger_time_error, trigger_offset, context} for every detected edge whose name is not empty.  Members, names and the reflected set are the reference's (:47-62).
// Device-only: the detector (gr::trigger::SchmittTrigger<T, Method, 32>, algorithm/.../SchmittTrigger.hpp) runs behind compute_domain gpu:hip (gr4hip_schmitt_*,
// gr4/hip.hpp); off the device the work loop refuses loudly.  SchmittTriggerPolynomial (:14) is not provided: the device has no Savitzky-Golay design.
// _period and _now follow :68-74 and :141: sample_rate sets _period = uint64(1e6f / sample_rate), trigger_time sets _now = trigger_time + uint64(1e6f trigger_offset),
// every sample adds _period; offset / threshold by settings reset the detector (:76-80).  start() / reset() (:83-89) read the wall clock into _now; this layer has
// no lifecycle calls, so _now counts from 0 until trigger_time is set.
// DEVIATIONS from the reference's processBulk (:91-163), stated here and in SCHMITT_TRIGGER.md:
//   - the reference publishes up to an interpolated edge position and returns (:133-136), so the samples between that position and the detecting sample go
//     through its detector a second time, and _now advances twice for them.  The device block feeds every sample to the detector exactly once and advances _now
//     once per sample.  For NO_INTERPOLATION (edge position = detecting sample) the tag streams are identical; for the linear methods the device's tags are
//     those of the detector class fed once.
//   - several edges of one chunk are published together, where the reference returns after each.
//   - an edge whose position sample + lastEdgeIdx lies in front of the chunk -- in front of what has been published -- is dropped, as the reference drops
//     edgePosition < 0 (:146), and counted in _dropped_edges; the reference's second limit, edgePosition < nProcess, holds likewise.
//   - the reference holds back the last N_HISTORY samples of a chunk (:93-98); the device handle carries the history across calls, so every sample is passed on.
//   - trigger_time = _now(sample) - int64(relOffset) in signed arithmetic (the reference converts a negative float to uint64_t, :126, which is undefined).
//   - forward_tag forwards the chunk's input tags the way this layer's work loop does for every block (the "gr:" keys, at the chunk's first sample).
template <typename T, gr::trigger::InterpolationMethod Method>
    requires(std::is_same_v<T, std::int16_t> || std::is_same_v<T, std::int32_t> || std::is_same_v<T, float> || std::is_same_v<T, double>)
struct SchmittTrigger : Block<SchmittTrigger<T, Method>, NoTagPropagation> {
    using value_t = T;
    template <typename U, gr::fixed_string description = "", typename... Arguments>
    using A = gr::Annotated<U, description, Arguments...>;
    constexpr static std::size_t                 N_HISTORY = 32;
    constexpr static trigger::InterpolationMethod kMethod   = Method;

    PortIn<T>  in;
    PortOut<T> out;

    A<value_t, "offset", Doc<"trigger offset">, Visible>                                                                         offset{value_t(0)};
    A<value_t, "threshold", Doc<"trigger threshold">, Visible>                                                                   threshold{value_t(1)};
    A<std::string, "rising trigger", Doc<"trigger name generated on detected rising edge (N.B. \"\" omits trigger)">, Visible>   trigger_name_rising_edge{std::string("RISING")};
    A<std::string, "falling trigger", Doc<"trigger name generated on detected falling edge (N.B. \"\" omits trigger)">, Visible> trigger_name_falling_edge{std::string("FALLING")};
    A<float, "avg. sample rate", Visible>                                                                                        sample_rate = 1.f;

    A<bool, "forward tags ", Doc<"false: emit only tags for detected edges">>                                                  forward_tag{true};
    A<std::string, "trigger name", Doc<"last trigger used to synchronise time">>                                               trigger_name{std::string()};
    A<std::uint64_t, "trigger time", Doc<"last trigger UTC time used for synchronisation (then sample counting)">, Unit<"ns">> trigger_time{0U};
    A<float, "trigger offset", Doc<"last trigger offset time used for synchronisation (then sample counting)">, Unit<"s">>     trigger_offset{0.0f};
    std::string                                                                                                                context = "";

    GR_MAKE_REFLECTABLE(SchmittTrigger, in, out, offset, threshold, trigger_name_rising_edge, trigger_name_falling_edge, sample_rate, forward_tag, trigger_name, trigger_time, trigger_offset, context);

    std::uint64_t _period{1U};
    std::uint64_t _now{0U};
    bool          _detector_changed = false; // offset / threshold named by an update since the device handle last took them: the detector is reset (:76-80)
    std::size_t   _dropped_edges    = 0;     // edges whose position fell outside the chunk (:146)
    std::size_t   _device_calls     = 0;     // chunks handed to the device

    void settingsChanged(const property_map&, const property_map& newSettings) {
        if (newSettings.contains("sample_rate")) _period = static_cast<std::uint64_t>(1e6f / sample_rate.value);
        if (newSettings.contains("trigger_time")) _now = trigger_time.value + static_cast<std::uint64_t>(1e6f * trigger_offset.value);
        if (newSettings.contains("offset") || newSettings.contains("threshold")) {
            // what gr4hip_schmitt_check refuses (include/gr4hip.h), said here so that a program that only holds the block needs no library
            const double o = static_cast<double>(offset.value), t = static_cast<double>(threshold.value);
            bool         ok = std::isfinite(o) && std::isfinite(t) && t >= 0.0;
            if constexpr (std::is_integral_v<T>) ok = ok && o + t <= static_cast<double>(std::numeric_limits<T>::max()) && o - t >= static_cast<double>(std::numeric_limits<T>::min());
            if (!ok) throw std::invalid_argument("SchmittTrigger: threshold must be finite and not negative, and offset +- threshold must stay in the sample type's range");
            _detector_changed = true;
        }
    }
    [[nodiscard]] gr4hip_schmitt_params params() const {
        constexpr int dtype = std::is_same_v<T, std::int16_t> ? GR4HIP_I16 : std::is_same_v<T, std::int32_t> ? GR4HIP_I32 : std::is_same_v<T, float> ? GR4HIP_F32 : GR4HIP_F64;
        return {static_cast<double>(offset.value), static_cast<double>(threshold.value), static_cast<int>(Method), dtype};
    }
    work::Status processBulk(std::span<const T>, std::span<T>) { // (the graph ends with ERROR: nothing comes out of the host path)
        std::fprintf(stderr, "SchmittTrigger: device-only block, needs compute_domain gpu:hip\n");
        this->_log("SchmittTrigger: device-only block, needs compute_domain gpu:hip");
        return work::Status::ERROR;
    }
};
template <typename T>
using SchmittTriggerNoInterpolation = SchmittTrigger<T, trigger::InterpolationMethod::NO_INTERPOLATION>;
template <typename T>
using SchmittTriggerBasic = SchmittTrigger<T, trigger::InterpolationMethod::BASIC_LINEAR_INTERPOLATION>;
template <typename T>
using SchmittTriggerLinear = SchmittTrigger<T, trigger::InterpolationMethod::LINEAR_INTERPOLATION>;
} // namespace gr::blocks::basic
namespace gr::algorithm::window {
enum class Type : int { None, Rectangular, Hamming, Hann, HannExp, Blackman, Nuttall, BlackmanHarris, BlackmanNuttall, FlatTop, Exponential, Kaiser }; // window.hpp:35 == GR4HIP_WIN_*
inline constexpr std::array<std::string_view, 12> TypeList{"None", "Rectangular", "Hamming", "Hann", "HannExp", "Blackman", "Nuttall", "BlackmanHarris", "BlackmanNuttall", "FlatTop", "Exponential", "Kaiser"};
inline bool gr_enum_parse(Type& d, std::string_view s) { return gr::detail::enum_from_names(d, s, TypeList); }
// window::create (window.hpp:69-183) through the library's host-side restatement
template <typename T>
std::vector<T> create(Type type, std::size_t n, float beta = 1.6f) {
    if constexpr (std::is_same_v<T, double>) { // create<double>: evaluated in double
        std::vector<double> w(n);
        if (n && gr4hip_window_create_f64(static_cast<int>(type), w.data(), n, static_cast<double>(beta)) != GR4HIP_OK) throw std::invalid_argument(std::string("window::create: ") + gr4hip_last_error());
        return w;
    } else {
        std::vector<float> w(n);
        if (n && gr4hip_window_create(static_cast<int>(type), w.data(), n, beta) != GR4HIP_OK) throw std::invalid_argument(std::string("window::create: ") + gr4hip_last_error());
        return std::vector<T>(w.begin(), w.end());
    }
}
} // namespace gr::algorithm::window
namespace gr::filter {

// designed coefficients: FIR = one section with a = {1}; IIR = biquad (or first-order) sections, applied as a cascade of DF_II sections
// (Filter<T>::processOne folds over the sections, FilterTool.hpp:223-247; DF_II is the float default :220)
struct DesignedFilter {
    bool                            fir = true;
    std::vector<float>              taps;     // FIR
    std::vector<std::array<float, 3>> b, a;   // IIR sections (zero padded to order 2)
};
inline DesignedFilter designFilter(FilterType ft, Type response, std::size_t order, double fLow, double fHigh, double fs, iir::Design iirDesign, algorithm::window::Type firWindow) {
    gr4hip_filter_params p;
    gr4hip_filter_params_default(&p);
    p.order = order; p.f_low = fLow; p.f_high = fHigh; p.fs = fs;
    DesignedFilter d;
    d.fir = ft == FilterType::FIR;
    const auto fail = [](const char* what) { throw std::invalid_argument(std::string(what) + ": " + gr4hip_last_error()); };
    if (d.fir) {
        std::size_t n = 0;
        if (gr4hip_fir_design(static_cast<int>(response), &p, static_cast<int>(firWindow), nullptr, 0, &n) != GR4HIP_OK) fail("fir::designFilter");
        d.taps.resize(n);
        if (gr4hip_fir_design(static_cast<int>(response), &p, static_cast<int>(firWindow), d.taps.data(), n, &n) != GR4HIP_OK) fail("fir::designFilter");
    } else {
        std::size_t        cap = 2 * order + 2, n = 0;
        std::vector<float> fb(3 * cap), fa(3 * cap);
        if (gr4hip_iir_design(static_cast<int>(response), &p, static_cast<int>(iirDesign), fb.data(), fa.data(), cap, &n) != GR4HIP_OK) fail("iir::designFilter");
        for (std::size_t s = 0; s < n; ++s) {
            d.b.push_back({fb[3 * s], fb[3 * s + 1], fb[3 * s + 2]});
            d.a.push_back({fa[3 * s], fa[3 * s + 1], fa[3 * s + 2]});
        }
    }
    return d;
}

template <typename T, typename... Args>
struct BasicFilterProto : Block<BasicFilterProto<T, Args...>, Args...> {
    using TParent = Block<BasicFilterProto<T, Args...>, Args...>;
    PortIn<T>  in;
    PortOut<T> out;
    Annotated<FilterType, "filter_type">                  filter_type     = FilterType::IIR;
    Annotated<Type, "filter_response">                    filter_response = Type::LOWPASS;
    Annotated<Size_t, "filter_order">                     filter_order{3};
    Annotated<float, "f_low">                             f_low{0.1f};
    Annotated<float, "f_high">                            f_high{0.2f};
    Annotated<float, "sample rate">                       sample_rate{1.0f};
    Annotated<Size_t, "decimation factor">                decimate{1U};
    Annotated<iir::Design, "iir_design_method">           iir_design_method = iir::Design::BUTTERWORTH;
    Annotated<algorithm::window::Type, "fir_design_method"> fir_design_method = algorithm::window::Type::Kaiser;
    GR_MAKE_REFLECTABLE(BasicFilterProto, in, out, filter_type, filter_response, filter_order, f_low, f_high, sample_rate, decimate, iir_design_method, fir_design_method);

    DesignedFilter              _design;
    std::vector<T>              _fir_hist;             // newest first
    std::vector<std::array<T, 2>> _w;                  // DF_II state per section
    bool                        _designed = false;

    void settingsChanged(const property_map&, const property_map&) { designFilter(); }
    void designFilter() { // time_domain_filter.hpp:163-182
        if constexpr (!TParent::ResamplingControl::kIsConst) this->input_chunk_size = decimate;
        _design = gr::filter::designFilter(filter_type, filter_response, filter_order, static_cast<double>(f_low.value), static_cast<double>(f_high.value), static_cast<double>(sample_rate.value), iir_design_method, fir_design_method);
        _fir_hist.assign(_design.taps.size(), T{});
        _w.assign(_design.b.size(), std::array<T, 2>{});
        _designed = true;
    }
    [[nodiscard]] T filterOne(T x) noexcept {
        if (_design.fir) {
            if (_fir_hist.empty()) return T{};
            std::move_backward(_fir_hist.begin(), _fir_hist.end() - 1, _fir_hist.end());
            _fir_hist[0] = x;
            T acc{};
            for (std::size_t k = 0; k < _fir_hist.size(); ++k) acc += static_cast<T>(_design.taps[k]) * _fir_hist[k];
            return acc;
        }
        for (std::size_t s = 0; s < _w.size(); ++s) { // DF_II section (FilterTool.hpp:127-135)
            const auto& b = _design.b[s];
            const auto& a = _design.a[s];
            const T w0 = x - static_cast<T>(a[1]) * _w[s][0] - static_cast<T>(a[2]) * _w[s][1];
            x          = static_cast<T>(b[0]) * w0 + static_cast<T>(b[1]) * _w[s][0] + static_cast<T>(b[2]) * _w[s][1];
            _w[s][1]   = _w[s][0];
            _w[s][0]   = w0;
        }
        return x;
    }
    [[nodiscard]] T processOne(T input) noexcept
    requires(TParent::ResamplingControl::kIsConst)
    {
        if (!_designed) designFilter();
        return filterOne(input);
    }
    [[nodiscard]] work::Status processBulk(std::span<const T> input, std::span<T> output) noexcept
    requires(!TParent::ResamplingControl::kIsConst)
    { // full-rate filter, keep the samples with i % decimate == 0 (time_domain_filter.hpp:190-204)
        if (!_designed) designFilter();
        std::size_t o = 0;
        for (std::size_t i = 0; i < input.size(); ++i) {
            const T y = filterOne(input[i]);
            if (i % decimate == 0) output[o++] = y;
        }
        return work::Status::OK;
    }
};
template <typename T> using BasicFilter           = BasicFilterProto<T>;
template <typename T> using BasicDecimatingFilter = BasicFilterProto<T, Resampling<1, 1, false>>;

// ---- interpolating FIR (BASELINE.json north_star).  The reference has no such block, only the rate declaration it would carry --
// Resampling<1, L> (annotated.hpp:121-128; chunk bookkeeping Block.hpp:1576-1636) -- so this follows fir_filter's shape (settings `b`, plus `interpolate`)
// and SURVEY.md Appendix A's definition: zero-stuff by L, fir_filter's sum at the output rate, gain L.  Host body: the polyphase form
// y[m L + p] = L sum_q b[q L + p] x[m - q]; output_chunk_size = interpolate, so gr:sample_rate is forwarded times L (Block.hpp:1088-1099).
template <typename T>
struct fir_interpolator : Block<fir_interpolator<T>, Resampling<1, 1, false>> {
    PortIn<T>          in;
    PortOut<T>         out;
    std::vector<float> b{1.f};
    Size_t             interpolate = 1;
    GR_MAKE_REFLECTABLE(fir_interpolator, in, out, b, interpolate);
    std::vector<T> _hist; // newest first, ceil(K / L) input samples

    void settingsChanged(const property_map&, const property_map&) {
        if (interpolate == 0) throw std::invalid_argument("fir_interpolator: interpolate must be >= 1");
        this->output_chunk_size = interpolate;
        const std::size_t kp = (b.size() + interpolate - 1) / interpolate;
        if (kp > _hist.size()) _hist.assign(kp, T{}); // like fir_filter: the history is replaced only when it must grow
    }
    [[nodiscard]] work::Status processBulk(std::span<const T> input, std::span<T> output) noexcept {
        const std::size_t L = interpolate, K = b.size(), kp = (K + L - 1) / L;
        if (_hist.size() < kp) _hist.assign(kp, T{});
        for (std::size_t m = 0; m < input.size(); ++m) {
            std::move_backward(_hist.begin(), _hist.end() - 1, _hist.end());
            _hist[0] = input[m];
            for (std::size_t p = 0; p < L; ++p) {
                T acc{};
                for (std::size_t q = 0; q * L + p < K; ++q) acc += static_cast<T>(b[q * L + p]) * _hist[q];
                output[m * L + p] = static_cast<T>(static_cast<float>(L)) * acc;
            }
        }
        return work::Status::OK;
    }
};

// ---- rational resampler, rate interpolate / decimate (RATIONAL_RESAMPLER.md).  The reference has the rate machinery (Resampling<inputChunk, outputChunk>,
// annotated.hpp:121-128; gr:sample_rate rescaling Block.hpp:1088-1099) and no such block, so like fir_interpolator this is the project's: zero-stuff by L,
// fir_filter's sum with gain L, keep every M-th sample.  Host body: the evaluated form of include/gr4hip.h -- output c L + p is
// sum_{q < Kp} (float(L) b[q L + (p M) mod L]) x[c M + floor(p M / L) - q] in float32, q ascending, one fmaf per term, the zero-padded terms included.
// input_chunk_size = decimate, output_chunk_size = interpolate: a work() call consumes whole cycles and gr:sample_rate is forwarded times L / M.
// New taps keep the carried inputs (unless more are needed); another L or M clears them.
template <typename T>
struct rational_resampler : Block<rational_resampler<T>, Resampling<1, 1, false>> {
    PortIn<T>          in;
    PortOut<T>         out;
    std::vector<float> b{1.f};
    Size_t             interpolate = 1;
    Size_t             decimate    = 1;
    GR_MAKE_REFLECTABLE(rational_resampler, in, out, b, interpolate, decimate);
    std::vector<T>     _hist; // the last samples in stream order, at least Kp - 1 of them
    std::vector<T>     _work;
    std::vector<float> _w;    // [Kp][L], q-major: float(L) b[q L + phi_p]
    std::size_t        _L = 0, _M = 0;

    void settingsChanged(const property_map&, const property_map&) {
        if (b.empty()) throw std::invalid_argument("rational_resampler: need at least one tap");
        if (interpolate == 0 || decimate == 0) throw std::invalid_argument("rational_resampler: interpolate and decimate must be >= 1");
        this->input_chunk_size  = decimate;
        this->output_chunk_size = interpolate;
        const std::size_t L = interpolate, M = decimate, K = b.size(), kp = (K + L - 1) / L;
        if (L != _L || M != _M) reset(); // another rate: the carried inputs belong to the old one
        _L = L;
        _M = M;
        if (kp > _hist.size()) _hist.assign(std::max<std::size_t>(32, std::bit_ceil(kp)), T{}); // the device handle's rule: capacity max(32, bit_ceil(Kp)), replaced only when it must grow
        _w.assign(kp * L, 0.f);
        for (std::size_t p = 0; p < L; ++p) {
            const std::size_t phi = p * M % L;
            for (std::size_t q = 0; q * L + phi < K; ++q) _w[q * L + p] = static_cast<float>(L) * b[q * L + phi];
        }
    }
    void reset() { std::fill(_hist.begin(), _hist.end(), T{}); }
    [[nodiscard]] std::size_t branchLength() const { return (b.size() + interpolate - 1) / std::max<std::size_t>(1, interpolate); }
    [[nodiscard]] work::Status processBulk(std::span<const T> input, std::span<T> output) noexcept {
        if (_L == 0) settingsChanged({}, {});
        const std::size_t L = _L, M = _M, kp = _w.size() / L, H = _hist.size(), cycles = input.size() / M;
        _work.resize(H + input.size());
        std::copy(_hist.begin(), _hist.end(), _work.begin());
        std::copy(input.begin(), input.end(), _work.begin() + static_cast<std::ptrdiff_t>(H));
        for (std::size_t c = 0; c < cycles; ++c)
            for (std::size_t p = 0; p < L; ++p) {
                const T* top = _work.data() + H + c * M + p * M / L; // x[c M + o_p]
                if constexpr (std::is_same_v<T, std::complex<float>>) {
                    float re = 0.f, im = 0.f;
                    for (std::size_t q = 0; q < kp; ++q) { re = std::fmaf(_w[q * L + p], (top - q)->real(), re); im = std::fmaf(_w[q * L + p], (top - q)->imag(), im); }
                    output[c * L + p] = T(re, im);
                } else {
                    T acc{};
                    for (std::size_t q = 0; q < kp; ++q) acc = std::fma(static_cast<T>(_w[q * L + p]), *(top - q), acc);
                    output[c * L + p] = acc;
                }
            }
        std::copy(_work.end() - static_cast<std::ptrdiff_t>(H), _work.end(), _hist.begin());
        return work::Status::OK;
    }
};

// ---- complex-tap FIR for complex streams, direct and decimating (SURVEY.md Appendix A's "complex-tap variant"; COMPLEX_FIR.md).  The reference's fir_filter is
// `requires std::floating_point<T>`, so like fir_interpolator this is the project's block: y[n] = sum_k b[k] x[n - k] with complex b, output m = y[m decimate].
// Settings: the taps as two float vectors of equal length (pmt has no complex vector), and `decimate`; input_chunk_size = decimate, so gr:sample_rate is
// forwarded divided by it (Block.hpp:1088-1099).  Host body: the sum in fir_filter's order, every complex product as four real products.
template <typename T>
    requires std::is_same_v<T, std::complex<float>>
struct complex_fir_filter : Block<complex_fir_filter<T>, Resampling<1, 1, false>> {
    PortIn<T>          in;
    PortOut<T>         out;
    std::vector<float> b_real{1.f};
    std::vector<float> b_imag{0.f};
    Size_t             decimate = 1;
    GR_MAKE_REFLECTABLE(complex_fir_filter, in, out, b_real, b_imag, decimate);
    std::vector<T> _hist; // newest first, K samples

    void settingsChanged(const property_map&, const property_map&) {
        if (b_real.size() != b_imag.size()) throw std::invalid_argument("complex_fir_filter: b_real and b_imag must have the same length");
        if (b_real.empty()) throw std::invalid_argument("complex_fir_filter: need at least one tap");
        if (decimate == 0) throw std::invalid_argument("complex_fir_filter: decimate must be >= 1");
        this->input_chunk_size = decimate;
        if (b_real.size() > _hist.size()) _hist.assign(b_real.size(), T{}); // like fir_filter: the history is replaced only when it must grow
    }
    void reset() { std::fill(_hist.begin(), _hist.end(), T{}); }
    [[nodiscard]] std::vector<float> interleavedTaps() const {
        std::vector<float> t(2 * b_real.size());
        for (std::size_t k = 0; k < b_real.size(); ++k) { t[2 * k] = b_real[k]; t[2 * k + 1] = k < b_imag.size() ? b_imag[k] : 0.f; }
        return t;
    }
    [[nodiscard]] work::Status processBulk(std::span<const T> input, std::span<T> output) noexcept {
        const std::size_t K = std::min(b_real.size(), b_imag.size()), D = std::max<std::size_t>(1, decimate);
        if (_hist.size() < K) _hist.assign(K, T{});
        std::size_t o = 0;
        for (std::size_t i = 0; i < input.size(); ++i) {
            std::move_backward(_hist.begin(), _hist.end() - 1, _hist.end());
            _hist[0] = input[i];
            if (i % D != 0) continue;
            float re = 0.f, im = 0.f;
            for (std::size_t k = 0; k < K; ++k) {
                const float xr = _hist[k].real(), xi = _hist[k].imag();
                re += b_real[k] * xr - b_imag[k] * xi;
                im += b_real[k] * xi + b_imag[k] * xr;
            }
            output[o++] = T(re, im);
        }
        return work::Status::OK;
    }
};
} // namespace gr::filter

namespace gr::blocks::math {
// MathOpImpl<T, op> (blocks/math/.../Math.hpp:30-57): out = in (op) value, default value 1
template <typename T, typename op>
struct MathOpImpl : Block<MathOpImpl<T, op>> {
    PortIn<T>  in;
    PortOut<T> out;
    T          value = T(1);
    GR_MAKE_REFLECTABLE(MathOpImpl, in, out, value);
    [[nodiscard]] constexpr T processOne(const T& a) const noexcept { return static_cast<T>(op()(a, value)); }
};
template <typename T> using AddConst      = MathOpImpl<T, std::plus<T>>;
template <typename T> using SubtractConst = MathOpImpl<T, std::minus<T>>;
template <typename T> using MultiplyConst = MathOpImpl<T, std::multiplies<T>>;
template <typename T> using DivideConst   = MathOpImpl<T, std::divides<T>>;

// MathOpMultiPortImpl<T, op> (Math.hpp:73-108): left fold over n_inputs (1..32) streams
template <typename T, typename op>
struct MathOpMultiPortImpl : Block<MathOpMultiPortImpl<T, op>> {
    std::vector<PortIn<T>> in;
    PortOut<T>             out;
    Size_t                 n_inputs = 0;
    GR_MAKE_REFLECTABLE(MathOpMultiPortImpl, in, out, n_inputs);
    void settingsChanged(const property_map&, const property_map& newSettings) {
        if (newSettings.contains("n_inputs")) {
            if (n_inputs < 1 || n_inputs > 32) throw std::invalid_argument("n_inputs must be in [1, 32]"); // Limits<1U, 32U> (Math.hpp:90)
            in.resize(n_inputs);
        }
    }
    work::Status processBulk(std::span<const std::span<const T>> ins, std::span<T> sout) const {
        std::copy(ins[0].begin(), ins[0].end(), sout.begin());
        for (std::size_t n = 1; n < ins.size(); ++n)
            std::transform(sout.begin(), sout.end(), ins[n].begin(), sout.begin(), [](T x, T y) { return static_cast<T>(op{}(x, y)); });
        return work::Status::OK;
    }
};
template <typename T> using Add      = MathOpMultiPortImpl<T, std::plus<T>>;
template <typename T> using Subtract = MathOpMultiPortImpl<T, std::minus<T>>;
template <typename T> using Multiply = MathOpMultiPortImpl<T, std::multiplies<T>>;
template <typename T> using Divide   = MathOpMultiPortImpl<T, std::divides<T>>;

// Rotator<std::complex<T>> (blocks/math/.../Rotator.hpp:16-63): XOR settings frequency_shift / phase_increment
template <typename T>
struct Rotator : Block<Rotator<T>> {
    using value_type = typename T::value_type;
    PortIn<T>  in;
    PortOut<T> out;
    float      sample_rate = 1.f, frequency_shift = 0.f;
    value_type phase_increment{0}, initial_phase{0};
    value_type _accumulated_phase{0};
    GR_MAKE_REFLECTABLE(Rotator, in, out, sample_rate, frequency_shift, initial_phase, phase_increment);
    void settingsChanged(const property_map&, const property_map& n) {
        const bool f = n.contains("frequency_shift"), p = n.contains("phase_increment");
        if (f && p) throw std::invalid_argument("cannot set both 'frequency_shift' and 'phase_increment' in new setting (XOR)");
        if (f) phase_increment = value_type(2) * static_cast<value_type>(std::numbers::pi_v<float> * frequency_shift / sample_rate);
        else if (p) frequency_shift = static_cast<float>(phase_increment / (value_type(2) * std::numbers::pi_v<value_type>)) * sample_rate;
        _accumulated_phase = initial_phase;
    }
    [[nodiscard]] T processOne(const T& x) noexcept {
        _accumulated_phase += phase_increment;
        if (_accumulated_phase > value_type(2) * std::numbers::pi_v<value_type>) _accumulated_phase -= value_type(2) * std::numbers::pi_v<value_type>;
        else if (_accumulated_phase < value_type(0)) _accumulated_phase += value_type(2) * std::numbers::pi_v<value_type>;
        return x * T(std::cos(_accumulated_phase), std::sin(_accumulated_phase));
    }
};
} // namespace gr::blocks::math

namespace gr::blocks::fft {
// Streaming |FFT|^2: one frame of fftSize complex samples in, fftSize floats (natural bin order) out.  The streaming counterpart of
// blocks::fft::FFT<T> (blocks/fourier/.../fft.hpp:31-251), which emits a DataSet per frame: mag2[(k + N/2) mod N] equals
// (DataSet magnitude[k] * N/2)^2.  Settings follow the FFT block: fftSize, window ("None" or "Hann").
template <typename T>
struct PowerSpectrum : Block<PowerSpectrum<T>, Resampling<1024, 1024, false>> {
    using value_type = typename T::value_type;
    PortIn<T>           in;
    PortOut<value_type> out;
    Size_t              fftSize = 1024;
    std::string         window  = "None";
    std::vector<value_type> _window;
    GR_MAKE_REFLECTABLE(PowerSpectrum, in, out, fftSize, window);

    void settingsChanged(const property_map&, const property_map&) {
        if (fftSize < 2 || (fftSize & (fftSize - 1))) throw std::invalid_argument("fftSize must be a power of two");
        this->input_chunk_size = this->output_chunk_size = fftSize; // fft.hpp:131-134: exactly whole frames
        _window.assign(fftSize, value_type(1));
        if (window == "Hann")
            for (std::size_t i = 0; i < fftSize; ++i) _window[i] = value_type(.5) - value_type(.5) * std::cos(value_type(2) * std::numbers::pi_v<value_type> / value_type(fftSize - 1) * value_type(i));
        else if (window != "None" && window != "Rectangular") _window.clear(); // the other ten windows exist on the device path only (gr4hip_window_create)
    }
    // host path: iterative radix-2 in double (plumbing only)
    work::Status processBulk(std::span<const T> input, std::span<value_type> output) {
        const std::size_t N = fftSize;
        if (_window.size() != N) settingsChanged({}, {});
        if (_window.size() != N) throw std::invalid_argument("PowerSpectrum: the host path implements None, Rectangular and Hann; window '" + window + "' needs compute_domain gpu:hip");
        std::vector<std::complex<double>> v(N);
        for (std::size_t f = 0; f + N <= input.size(); f += N) {
            for (std::size_t i = 0, j = 0; i < N; ++i) {
                v[j] = std::complex<double>(input[f + i]) * static_cast<double>(_window[i]);
                std::size_t m = N >> 1;
                while (m >= 1 && (j & m)) { j ^= m; m >>= 1; }
                j |= m;
            }
            for (std::size_t len = 2; len <= N; len <<= 1)
                for (std::size_t k = 0; k < N; k += len)
                    for (std::size_t n = 0; n < len / 2; ++n) {
                        const auto w = std::polar(1.0, -2.0 * std::numbers::pi * static_cast<double>(n) / static_cast<double>(len));
                        const auto t = v[k + n + len / 2] * w;
                        v[k + n + len / 2] = v[k + n] - t;
                        v[k + n] += t;
                    }
            for (std::size_t i = 0; i < N; ++i) output[f + i] = static_cast<value_type>(std::norm(v[i]));
        }
        return work::Status::OK;
    }
};

// ---- polyphase filter bank in front of the transform (critically sampled analysis bank; PFB.md -- the reference has no polyphase form, the definition is the
// project's):  frame m = DFT_N( u_m ),  u_m[i] = sum_{k < P} h[k N + i] x[(m - P + 1 + k) N + i],  N = fftSize, P = taps_per_channel, zero initial history.
// PfbPowerSpectrum emits |X|^2 (float), PfbChannelizer the spectrum itself (complex, frame-major: fftSize bins per frame), both in natural bin order.
// Settings: fftSize, taps_per_channel, taps (P N values; empty = the windowed-sinc prototype of gr4hip_pfb_design with `window`), window.
// Host body: the float32 sums of the definition (k ascending from 0, one fma per term and component) and PowerSpectrum's float64 radix-2 transform (plumbing).
namespace detail {
struct PfbCore {
    std::vector<float>               h;    // the prototype in use, P N values
    std::vector<std::complex<float>> hist; // the last (P - 1) N samples
    std::size_t                      N = 0, P = 0;

    // throws on every bad setting; a change of N or P clears the history, new taps alone keep it
    void configure(std::size_t fftSize, std::size_t tapsPerChannel, const std::vector<float>& taps, const std::string& window) {
        if (fftSize < 2 || (fftSize & (fftSize - 1))) throw std::invalid_argument("fftSize must be a power of two");
        if (tapsPerChannel < 1 || tapsPerChannel > 32) throw std::invalid_argument("taps_per_channel must be in [1, 32]");
        if (!taps.empty() && taps.size() != fftSize * tapsPerChannel) throw std::invalid_argument("taps: need taps_per_channel * fftSize values (or none: designed)");
        std::vector<float> next(taps);
        if (next.empty()) {
            gr::algorithm::window::Type type{};
            if (!gr_enum_parse(type, std::string_view(window))) throw std::invalid_argument("unknown window '" + window + "'");
            next.resize(fftSize * tapsPerChannel);
            if (gr4hip_pfb_design(next.data(), fftSize, tapsPerChannel, static_cast<int>(type), 1.6f) != GR4HIP_OK) throw std::invalid_argument(std::string("pfb design: ") + gr4hip_last_error());
        }
        h = std::move(next);
        if (fftSize != N || tapsPerChannel != P) hist.assign((tapsPerChannel - 1) * fftSize, {});
        N = fftSize;
        P = tapsPerChannel;
    }
    void reset() { std::fill(hist.begin(), hist.end(), std::complex<float>{}); }

    // whole frames of `input` -> emit(frame index, bin, X)
    template <typename Emit>
    void process(std::span<const std::complex<float>> input, Emit&& emit) {
        const std::size_t                 M = input.size() / N, H = (P - 1) * N;
        std::vector<std::complex<double>> v(N);
        const auto sample = [&](std::ptrdiff_t n) { return n < 0 ? hist[H - static_cast<std::size_t>(-n)] : input[static_cast<std::size_t>(n)]; }; // n relative to the call
        for (std::size_t m = 0; m < M; ++m) {
            for (std::size_t i = 0, j = 0; i < N; ++i) {
                float re = 0.f, im = 0.f;
                for (std::size_t k = 0; k < P; ++k) {
                    const auto s = sample(static_cast<std::ptrdiff_t>((m + k) * N + i) - static_cast<std::ptrdiff_t>(H));
                    re = std::fma(h[k * N + i], s.real(), re);
                    im = std::fma(h[k * N + i], s.imag(), im);
                }
                v[j] = std::complex<double>(re, im);
                std::size_t b = N >> 1;
                while (b >= 1 && (j & b)) { j ^= b; b >>= 1; }
                j |= b;
            }
            for (std::size_t len = 2; len <= N; len <<= 1)
                for (std::size_t k = 0; k < N; k += len)
                    for (std::size_t n = 0; n < len / 2; ++n) {
                        const auto w = std::polar(1.0, -2.0 * std::numbers::pi * static_cast<double>(n) / static_cast<double>(len));
                        const auto t = v[k + n + len / 2] * w;
                        v[k + n + len / 2] = v[k + n] - t;
                        v[k + n] += t;
                    }
            for (std::size_t c = 0; c < N; ++c) emit(m, c, v[c]);
        }
        // the last (P - 1) N samples of history + input
        if (H) {
            std::vector<std::complex<float>> next(H);
            const std::ptrdiff_t             n0 = static_cast<std::ptrdiff_t>(M * N) - static_cast<std::ptrdiff_t>(H);
            for (std::size_t j = 0; j < H; ++j) next[j] = sample(n0 + static_cast<std::ptrdiff_t>(j));
            hist = std::move(next);
        }
    }
};
} // namespace detail

template <typename T>
    requires std::is_same_v<T, std::complex<float>>
struct PfbPowerSpectrum : Block<PfbPowerSpectrum<T>, Resampling<1024, 1024, false>> {
    PortIn<T>          in;
    PortOut<float>     out;
    Size_t             fftSize          = 1024;
    Size_t             taps_per_channel = 4;
    std::vector<float> taps;
    std::string        window = "Hamming";
    GR_MAKE_REFLECTABLE(PfbPowerSpectrum, in, out, fftSize, taps_per_channel, taps, window);
    detail::PfbCore _core;

    void settingsChanged(const property_map&, const property_map&) {
        _core.configure(fftSize, taps_per_channel, taps, window);
        this->input_chunk_size = this->output_chunk_size = fftSize; // whole frames
    }
    void reset() { _core.reset(); }
    work::Status processBulk(std::span<const T> input, std::span<float> output) {
        if (_core.N != fftSize) settingsChanged({}, {});
        _core.process(input, [&](std::size_t m, std::size_t c, const std::complex<double>& X) { output[m * _core.N + c] = static_cast<float>(std::norm(X)); });
        return work::Status::OK;
    }
};

template <typename T>
    requires std::is_same_v<T, std::complex<float>>
struct PfbChannelizer : Block<PfbChannelizer<T>, Resampling<1024, 1024, false>> {
    PortIn<T>          in;
    PortOut<T>         out;
    Size_t             fftSize          = 1024;
    Size_t             taps_per_channel = 4;
    std::vector<float> taps;
    std::string        window = "Hamming";
    GR_MAKE_REFLECTABLE(PfbChannelizer, in, out, fftSize, taps_per_channel, taps, window);
    detail::PfbCore _core;

    void settingsChanged(const property_map&, const property_map&) {
        _core.configure(fftSize, taps_per_channel, taps, window);
        this->input_chunk_size = this->output_chunk_size = fftSize;
    }
    void reset() { _core.reset(); }
    work::Status processBulk(std::span<const T> input, std::span<T> output) {
        if (_core.N != fftSize) settingsChanged({}, {});
        _core.process(input, [&](std::size_t m, std::size_t c, const std::complex<double>& X) { output[m * _core.N + c] = static_cast<T>(X); });
        return work::Status::OK;
    }
};

// ---- inverse transform and polyphase synthesis bank (INVERSE_FFT.md): frames of fftSize complex bins in natural order (what PfbChannelizer emits) -> samples.
//   InverseFFT<complex<float>>:  x[n] = sum_k X[k] e^{+2 pi i k n / N}, unnormalised like algorithm::FFT's Direction::Backward (algorithm/.../fourier/fft.hpp:260-314)
//   InverseFFT<float>:           the packed complex-to-real form (fft.hpp:277-283): bins 0 .. N/2 of each frame, the imaginary parts of bins 0 and N/2 ignored
//   PfbSynthesizer:              v_m = the transform of frame m, y[m N + i] = sum_{k < P} g[k N + i] v_{m - k}[i]  (the project's own definition)
// Settings: fftSize, window (a synthesis window on the samples; the bank: the prototype's design window), scale (times 1 / fftSize, before the window).
// Host bodies, the definition written plainly: a float64 transform rounded to float, then float multiplies (scale, window) / std::fmaf sums (k ascending from 0).
namespace detail {
// in-place unnormalised inverse DFT (e^{+...}) of a power-of-two frame in float64
inline void inverse_dft64(std::vector<std::complex<double>>& v) {
    const std::size_t N = v.size();
    for (std::size_t i = 0, j = 0; i < N; ++i) {
        if (i < j) std::swap(v[i], v[j]);
        std::size_t b = N >> 1;
        while (b >= 1 && (j & b)) { j ^= b; b >>= 1; }
        j |= b;
    }
    for (std::size_t len = 2; len <= N; len <<= 1)
        for (std::size_t k = 0; k < N; k += len)
            for (std::size_t n = 0; n < len / 2; ++n) {
                const auto w = std::polar(1.0, 2.0 * std::numbers::pi * static_cast<double>(n) / static_cast<double>(len));
                const auto t = v[k + n + len / 2] * w;
                v[k + n + len / 2] = v[k + n] - t;
                v[k + n] += t;
            }
}
inline void check_inverse_size(std::size_t fftSize) {
    if (fftSize < 2 || (fftSize & (fftSize - 1)) || fftSize > 8192) throw std::invalid_argument("fftSize must be a power of two in [2, 8192]");
}
// the float window of gr4hip_window_create (host code of the library); "None" / "Rectangular": empty = no multiply
inline std::vector<float> synthesis_window(const std::string& window, std::size_t n) {
    gr::algorithm::window::Type type{};
    if (!gr_enum_parse(type, std::string_view(window))) throw std::invalid_argument("unknown window '" + window + "'");
    if (type == gr::algorithm::window::Type::None || type == gr::algorithm::window::Type::Rectangular) return {};
    std::vector<float> w(n);
    if (gr4hip_window_create(static_cast<int>(type), w.data(), n, 1.6f) != GR4HIP_OK) throw std::invalid_argument(std::string("window: ") + gr4hip_last_error());
    return w;
}
} // namespace detail

template <typename T>
    requires(std::is_same_v<T, std::complex<float>> || std::is_same_v<T, float>)
struct InverseFFT : Block<InverseFFT<T>, Resampling<1024, 1024, false>> {
    PortIn<std::complex<float>> in;
    PortOut<T>                  out;
    Size_t                      fftSize = 1024;
    std::string                 window  = "None";
    bool                        scale   = false;
    GR_MAKE_REFLECTABLE(InverseFFT, in, out, fftSize, window, scale);
    std::vector<float> _window;
    std::size_t        _n = 0;

    void settingsChanged(const property_map&, const property_map&) {
        detail::check_inverse_size(fftSize);
        _window = detail::synthesis_window(window, fftSize);
        _n      = fftSize;
        this->input_chunk_size = this->output_chunk_size = fftSize; // whole frames
    }
    work::Status processBulk(std::span<const std::complex<float>> input, std::span<T> output) {
        if (_n != fftSize) settingsChanged({}, {});
        const std::size_t                 N = _n;
        const float                       s = scale ? 1.f / static_cast<float>(N) : 1.f;
        std::vector<std::complex<double>> v(N);
        for (std::size_t f = 0; f + N <= input.size(); f += N) {
            for (std::size_t k = 0; k < N; ++k) v[k] = std::complex<double>(input[f + k]);
            if constexpr (std::is_same_v<T, float>) { // the Hermitian expansion of bins 0 .. N/2
                v[0] = v[0].real();
                v[N / 2] = v[N / 2].real();
                for (std::size_t k = 1; k < N / 2; ++k) v[N - k] = std::conj(v[k]);
            }
            detail::inverse_dft64(v);
            for (std::size_t n = 0; n < N; ++n) {
                std::complex<float> y(static_cast<float>(v[n].real()) * s, static_cast<float>(v[n].imag()) * s);
                if (!_window.empty()) y = std::complex<float>(y.real() * _window[n], y.imag() * _window[n]);
                if constexpr (std::is_same_v<T, float>) output[f + n] = y.real();
                else output[f + n] = y;
            }
        }
        return work::Status::OK;
    }
};

template <typename T>
    requires std::is_same_v<T, std::complex<float>>
struct PfbSynthesizer : Block<PfbSynthesizer<T>, Resampling<1024, 1024, false>> {
    PortIn<T>          in;
    PortOut<T>         out;
    Size_t             fftSize          = 1024;
    Size_t             taps_per_channel = 4;
    std::vector<float> taps;
    std::string        window = "Hamming";
    bool               scale  = false;
    GR_MAKE_REFLECTABLE(PfbSynthesizer, in, out, fftSize, taps_per_channel, taps, window, scale);
    std::vector<float> _g;    // the prototype in use, P N values
    std::vector<T>     _hist; // the last P - 1 transformed frames, oldest first
    std::size_t        _N = 0, _P = 0;

    // throws on every bad setting; a change of fftSize or taps_per_channel clears the history, new taps alone keep it
    void settingsChanged(const property_map&, const property_map&) {
        detail::check_inverse_size(fftSize);
        if (taps_per_channel < 1 || taps_per_channel > 32) throw std::invalid_argument("taps_per_channel must be in [1, 32]");
        if (!taps.empty() && taps.size() != fftSize * taps_per_channel) throw std::invalid_argument("taps: need taps_per_channel * fftSize values (or none: designed)");
        std::vector<float> next(taps);
        if (next.empty()) {
            gr::algorithm::window::Type type{};
            if (!gr_enum_parse(type, std::string_view(window))) throw std::invalid_argument("unknown window '" + window + "'");
            next.resize(fftSize * taps_per_channel);
            if (gr4hip_pfb_design(next.data(), fftSize, taps_per_channel, static_cast<int>(type), 1.6f) != GR4HIP_OK) throw std::invalid_argument(std::string("pfb design: ") + gr4hip_last_error());
        }
        _g = std::move(next);
        if (fftSize != _N || taps_per_channel != _P) _hist.assign((taps_per_channel - 1) * fftSize, T{});
        _N = fftSize;
        _P = taps_per_channel;
        this->input_chunk_size = this->output_chunk_size = fftSize;
    }
    void reset() { std::fill(_hist.begin(), _hist.end(), T{}); }
    work::Status processBulk(std::span<const T> input, std::span<T> output) {
        if (_N != fftSize) settingsChanged({}, {});
        const std::size_t                 N = _N, P = _P, M = input.size() / N, H = (P - 1) * N;
        const float                       s = scale ? 1.f / static_cast<float>(N) : 1.f;
        std::vector<T>                    v(H + M * N); // the history, then the call's transformed frames
        std::vector<std::complex<double>> w(N);
        std::copy(_hist.begin(), _hist.end(), v.begin());
        for (std::size_t m = 0; m < M; ++m) {
            for (std::size_t c = 0; c < N; ++c) w[c] = std::complex<double>(input[m * N + c]);
            detail::inverse_dft64(w);
            for (std::size_t i = 0; i < N; ++i) v[H + m * N + i] = T(static_cast<float>(w[i].real()) * s, static_cast<float>(w[i].imag()) * s);
        }
        for (std::size_t m = 0; m < M; ++m)
            for (std::size_t i = 0; i < N; ++i) {
                float re = 0.f, im = 0.f;
                for (std::size_t k = 0; k < P; ++k) {
                    const T& q = v[H + m * N + i - k * N]; // frame m - k
                    re = std::fmaf(_g[k * N + i], q.real(), re);
                    im = std::fmaf(_g[k * N + i], q.imag(), im);
                }
                output[m * N + i] = T(re, im);
            }
        _hist.assign(v.end() - static_cast<std::ptrdiff_t>(H), v.end());
        return work::Status::OK;
    }
};

// ---- spectrum integrator behind a power spectrum (SPECTRUM_INTEGRATOR.md -- the reference has no such block, the definition is the project's): the sum (mean:
// the mean) of n_integrate consecutive frames of vector_size values, one frame out per n_integrate frames in.  One fixed order of additions, on the host as on
// the device: float32 sums over leaves of gr4hip_specint_leaf() = 32 frames counted from the integration's start, the leaves into a float64 sum in ascending
// order, one rounding to float32 (mean: after the division by n_integrate in float64).
// A work() call consumes whole integrations (input_chunk_size = n_integrate * vector_size), so gr:sample_rate is forwarded divided by n_integrate by the
// Resampling bookkeeping and nothing is carried between calls.  LIMIT: n_integrate * vector_size samples must fit the input edge.  A longer integration is two
// integrators in a row (A = A1 A2) -- which is ANOTHER order of additions (float32 leaves of the first, rounded to float32, then summed again), not this
// definition with a larger A.
template <typename T>
    requires std::is_same_v<T, float>
struct SpectrumIntegrator : Block<SpectrumIntegrator<T>, Resampling<1024, 1024, false>> {
    PortIn<T>  in;
    PortOut<T> out;
    Size_t     vector_size = 1024;
    Size_t     n_integrate = 1;
    bool       mean        = false;
    GR_MAKE_REFLECTABLE(SpectrumIntegrator, in, out, vector_size, n_integrate, mean);
    std::vector<double> _acc;
    std::vector<float>  _leaf;

    void settingsChanged(const property_map&, const property_map&) {
        if (vector_size < 2) throw std::invalid_argument("SpectrumIntegrator: vector_size must be >= 2");
        if (n_integrate == 0) throw std::invalid_argument("SpectrumIntegrator: n_integrate must be >= 1");
        this->input_chunk_size  = n_integrate * vector_size;
        this->output_chunk_size = vector_size;
    }
    [[nodiscard]] work::Status processBulk(std::span<const T> input, std::span<T> output) {
        if (this->input_chunk_size != n_integrate * vector_size) settingsChanged({}, {});
        const std::size_t N = vector_size, A = n_integrate, B = gr4hip_specint_leaf();
        _acc.resize(N);
        _leaf.resize(N);
        for (std::size_t q = 0; (q + 1) * A * N <= input.size(); ++q) {
            std::fill(_acc.begin(), _acc.end(), 0.0);
            for (std::size_t s = 0; s < A; s += B) {
                std::fill(_leaf.begin(), _leaf.end(), 0.f);
                for (std::size_t f = s; f < std::min(s + B, A); ++f)
                    for (std::size_t c = 0; c < N; ++c) _leaf[c] = _leaf[c] + input[(q * A + f) * N + c];
                for (std::size_t c = 0; c < N; ++c) _acc[c] = _acc[c] + static_cast<double>(_leaf[c]);
            }
            for (std::size_t c = 0; c < N; ++c) output[q * N + c] = static_cast<float>(mean ? _acc[c] / static_cast<double>(A) : _acc[c]);
        }
        return work::Status::OK;
    }
};

// ---- cross-spectrum correlator behind n_inputs spectra (CROSS_SPECTRUM.md -- the reference has no such block, the definition is the project's): the averaged
// cross-spectral matrix V_ij[c] = sum_m X_i[m][c] conj(X_j[m][c]) over n_integrate frames of vector_size bins, baselines j <= i packed p = i (i + 1) / 2 + j, one
// matrix [P][vector_size] out per n_integrate frames in on every input.  One fixed order of operations, on the host as on the device: per pair and bin a float32
// fma chain over leaves of gr4hip_xcorr_leaf() = 64 frames counted from the integration's start
//     re = fmaf(xr_i, xr_j, re);  re = fmaf(xi_i, xi_j, re);  im = fmaf(xi_i, xr_j, im);  im = fmaf(-xr_i, xi_j, im);
// the leaves into float64 sums in ascending order, one rounding to float32 (mean: after the division by n_integrate in float64); the imaginary part of the
// diagonal is +0.  A work() call consumes whole integrations (input_chunk_size = n_integrate * vector_size per input, output_chunk_size = P * vector_size), so
// gr:sample_rate is forwarded scaled by P / n_integrate by the Resampling bookkeeping and nothing is carried between calls.
template <typename T>
    requires std::is_same_v<T, float>
struct CrossSpectrum : Block<CrossSpectrum<T>, Resampling<1024, 3072, false>> {
    std::vector<PortIn<std::complex<T>>> in{2};
    PortOut<std::complex<T>>             out;
    Size_t                               n_inputs    = 2;
    Size_t                               vector_size = 1024;
    Size_t                               n_integrate = 1;
    bool                                 mean        = false;
    GR_MAKE_REFLECTABLE(CrossSpectrum, in, out, n_inputs, vector_size, n_integrate, mean);
    std::vector<double> _acc;
    std::vector<float>  _leaf;

    [[nodiscard]] std::size_t nBaselines() const { return static_cast<std::size_t>(n_inputs) * (n_inputs + 1) / 2; }

    void settingsChanged(const property_map&, const property_map&) {
        if (n_inputs < 2 || n_inputs > 32) throw std::invalid_argument("CrossSpectrum: n_inputs must be in [2, 32]");
        if (vector_size < 2) throw std::invalid_argument("CrossSpectrum: vector_size must be >= 2");
        if (n_integrate == 0) throw std::invalid_argument("CrossSpectrum: n_integrate must be >= 1");
        if (in.size() != n_inputs) in.resize(n_inputs);
        this->input_chunk_size  = n_integrate * vector_size;
        this->output_chunk_size = nBaselines() * vector_size;
    }
    [[nodiscard]] work::Status processBulk(std::span<const std::span<const std::complex<T>>> ins, std::span<std::complex<T>> output) {
        if (this->input_chunk_size != n_integrate * vector_size || this->output_chunk_size != nBaselines() * vector_size) settingsChanged({}, {});
        const std::size_t S = ins.size(), N = vector_size, A = n_integrate, B = gr4hip_xcorr_leaf(), P = S * (S + 1) / 2;
        _acc.resize(2 * N);
        _leaf.resize(2 * N);
        for (std::size_t q = 0; (q + 1) * A * N <= ins[0].size(); ++q) {
            for (std::size_t i = 0, p = 0; i < S; ++i) {
                for (std::size_t j = 0; j <= i; ++j, ++p) {
                    std::fill(_acc.begin(), _acc.end(), 0.0);
                    for (std::size_t s = 0; s < A; s += B) {
                        std::fill(_leaf.begin(), _leaf.end(), 0.f);
                        for (std::size_t f = s; f < std::min(s + B, A); ++f) {
                            const std::complex<T>* xi = ins[i].data() + (q * A + f) * N;
                            const std::complex<T>* xj = ins[j].data() + (q * A + f) * N;
                            for (std::size_t c = 0; c < N; ++c) {
                                float re = _leaf[2 * c], im = _leaf[2 * c + 1];
                                re = std::fmaf(xi[c].real(), xj[c].real(), re);
                                re = std::fmaf(xi[c].imag(), xj[c].imag(), re);
                                im = std::fmaf(xi[c].imag(), xj[c].real(), im);
                                im = std::fmaf(-xi[c].real(), xj[c].imag(), im);
                                _leaf[2 * c] = re, _leaf[2 * c + 1] = im;
                            }
                        }
                        for (std::size_t c = 0; c < 2 * N; ++c) _acc[c] = _acc[c] + static_cast<double>(_leaf[c]);
                    }
                    for (std::size_t c = 0; c < N; ++c) {
                        const double re = mean ? _acc[2 * c] / static_cast<double>(A) : _acc[2 * c], im = mean ? _acc[2 * c + 1] / static_cast<double>(A) : _acc[2 * c + 1];
                        output[(q * P + p) * N + c] = std::complex<T>(static_cast<float>(re), i == j ? 0.f : static_cast<float>(im));
                    }
                }
            }
        }
        return work::Status::OK;
    }
};

// ---- beamformer behind n_inputs spectra (BEAMFORMER.md -- the reference has no such block, the definition is the project's): the per-bin weighted sum of the
// streams into n_beams beams, Y_b[f][c] = sum_s W[b][s][c] X_s[f][c], one frame [n_beams][vector_size] out per frame of vector_size bins in on every input.  One
// fixed order of operations, on the host as on the device: per beam, frame and bin a float32 fma chain over the streams in ascending order from re = im = +0
//     re = fmaf(wr_s, xr_s, re);  re = fmaf(-wi_s, xi_s, re);  im = fmaf(wi_s, xr_s, im);  im = fmaf(wr_s, xi_s, im);
// weights_real / weights_imag hold W[b][s][c], bin fastest (n_beams n_inputs vector_size values), or W[b][s] (n_beams n_inputs values: the same weight in every
// bin).  input_chunk_size = vector_size, output_chunk_size = n_beams * vector_size, so gr:sample_rate is forwarded scaled by n_beams by the Resampling
// bookkeeping and nothing is carried between calls.  Integrated power in a graph is Beamformer -> |.|^2 -> SpectrumIntegrator, from the existing blocks.
template <typename T>
    requires std::is_same_v<T, float>
struct Beamformer : Block<Beamformer<T>, Resampling<1024, 1024, false>> {
    std::vector<PortIn<std::complex<T>>> in{2};
    PortOut<std::complex<T>>             out;
    Size_t                               n_inputs    = 2;
    Size_t                               n_beams     = 1;
    Size_t                               vector_size = 1024;
    std::vector<float>                   weights_real{0.5f, 0.5f};
    std::vector<float>                   weights_imag{0.f, 0.f};
    GR_MAKE_REFLECTABLE(Beamformer, in, out, n_inputs, n_beams, vector_size, weights_real, weights_imag);

    // W[b][s][c] of either form
    [[nodiscard]] std::complex<T> weight(std::size_t b, std::size_t s, std::size_t c) const {
        const std::size_t S = n_inputs, N = vector_size, i = weights_real.size() == static_cast<std::size_t>(n_beams) * S ? b * S + s : (b * S + s) * N + c;
        return {weights_real[i], weights_imag[i]};
    }

    void settingsChanged(const property_map&, const property_map&) {
        if (n_inputs < 1 || n_inputs > 32) throw std::invalid_argument("Beamformer: n_inputs must be in [1, 32]");
        if (n_beams < 1 || n_beams > 32) throw std::invalid_argument("Beamformer: n_beams must be in [1, 32]");
        if (vector_size < 2) throw std::invalid_argument("Beamformer: vector_size must be >= 2");
        if (weights_real.size() != weights_imag.size()) throw std::invalid_argument("Beamformer: weights_real and weights_imag must have the same length");
        const std::size_t BS = static_cast<std::size_t>(n_beams) * n_inputs;
        if (weights_real.size() != BS && weights_real.size() != BS * vector_size) throw std::invalid_argument("Beamformer: need n_beams * n_inputs weights, or that times vector_size");
        if (in.size() != n_inputs) in.resize(n_inputs);
        this->input_chunk_size  = vector_size;
        this->output_chunk_size = n_beams * vector_size;
    }
    [[nodiscard]] work::Status processBulk(std::span<const std::span<const std::complex<T>>> ins, std::span<std::complex<T>> output) {
        if (this->input_chunk_size != vector_size || this->output_chunk_size != n_beams * vector_size) settingsChanged({}, {});
        const std::size_t S = ins.size(), B = n_beams, N = vector_size;
        for (std::size_t f = 0; (f + 1) * N <= ins[0].size(); ++f) {
            for (std::size_t b = 0; b < B; ++b) {
                for (std::size_t c = 0; c < N; ++c) {
                    float re = 0.f, im = 0.f;
                    for (std::size_t s = 0; s < S; ++s) {
                        const std::complex<T> w = weight(b, s, c), x = ins[s][f * N + c];
                        re = std::fmaf(w.real(), x.real(), re);
                        re = std::fmaf(-w.imag(), x.imag(), re);
                        im = std::fmaf(w.imag(), x.real(), im);
                        im = std::fmaf(w.real(), x.imag(), im);
                    }
                    output[(f * B + b) * N + c] = std::complex<T>(re, im);
                }
            }
        }
        return work::Status::OK;
    }
};

// ---- adaptive (MVDR / Capon) beamformer weights behind CrossSpectrum (ADAPTIVE_WEIGHTS.md -- the reference has no such block, the definition is the project's):
// per matrix [P][vector_size] in (what CrossSpectrum<float>::out emits, packed lower triangle p = i (i + 1) / 2 + j, j <= i) one set of weights
// [n_beams][n_inputs][vector_size] out, laid out as Beamformer's weights.  All arithmetic is double, on the host as on the device, per matrix and bin:
//     R_ij = V_ij (j < i),  R_ji = conj(V_ij),  R_ii = Re V_ii (the imaginary part is ignored)
//     lambda = loading * (sum_i R_ii) / S ;   R'_ii = R_ii + lambda
//     R' = L L^H   Cholesky, columns j ascending, every inner sum with k ascending:
//         s_j  = R'_jj - sum_{k<j} |L_jk|^2 ;   L_jj = sqrt(s_j)
//         L_ij = (R'_ij - sum_{k<j} L_ik conj(L_jk)) / L_jj            (i > j)
//     per beam b:   L y = a_b  (forward, k ascending) ;   d = sum_k |y_k|^2
//                   L^H u = y  (backward) ;   w = u / d
//     W[q][b][s][c] = conj(w_s)  rounded once to complex<float>
// and a pivot s_j that is not > 0 (NaN included) makes every weight of that matrix and bin a quiet NaN.  steering_real / steering_imag hold a[b][s][c], bin
// fastest (n_beams n_inputs vector_size values), or a[b][s] (the same vector in every bin).  input_chunk_size = P * vector_size, output_chunk_size =
// n_beams * n_inputs * vector_size, so gr:sample_rate is forwarded scaled by n_beams n_inputs / P by the Resampling bookkeeping and nothing is carried between
// calls.  LIMIT: P * vector_size samples must fit the input edge.  The Capon power is not a port: gr4hip_mvdr_process(d_power) has it.
template <typename T>
    requires std::is_same_v<T, float>
struct AdaptiveWeights : Block<AdaptiveWeights<T>, Resampling<3072, 2048, false>> {
    PortIn<std::complex<T>>  in;
    PortOut<std::complex<T>> out;
    Size_t                   n_inputs    = 2;
    Size_t                   n_beams     = 1;
    Size_t                   vector_size = 1024;
    std::vector<float>       steering_real{1.f, 1.f};
    std::vector<float>       steering_imag{0.f, 0.f};
    double                   loading = 0.0;
    GR_MAKE_REFLECTABLE(AdaptiveWeights, in, out, n_inputs, n_beams, vector_size, steering_real, steering_imag, loading);
    std::vector<std::complex<double>> _l, _y;

    [[nodiscard]] std::size_t nBaselines() const { return static_cast<std::size_t>(n_inputs) * (n_inputs + 1) / 2; }
    // a[b][s][c] of either form
    [[nodiscard]] std::complex<T> steer(std::size_t b, std::size_t s, std::size_t c) const {
        const std::size_t S = n_inputs, N = vector_size, i = steering_real.size() == static_cast<std::size_t>(n_beams) * S ? b * S + s : (b * S + s) * N + c;
        return {steering_real[i], steering_imag[i]};
    }

    void settingsChanged(const property_map&, const property_map&) {
        if (n_inputs < 2 || n_inputs > 32) throw std::invalid_argument("AdaptiveWeights: n_inputs must be in [2, 32]");
        if (n_beams < 1 || n_beams > 32) throw std::invalid_argument("AdaptiveWeights: n_beams must be in [1, 32]");
        if (vector_size < 2) throw std::invalid_argument("AdaptiveWeights: vector_size must be >= 2");
        if (!(loading >= 0.0) || !std::isfinite(loading)) throw std::invalid_argument("AdaptiveWeights: loading must be finite and >= 0");
        if (steering_real.size() != steering_imag.size()) throw std::invalid_argument("AdaptiveWeights: steering_real and steering_imag must have the same length");
        const std::size_t BS = static_cast<std::size_t>(n_beams) * n_inputs;
        if (steering_real.size() != BS && steering_real.size() != BS * vector_size) throw std::invalid_argument("AdaptiveWeights: need n_beams * n_inputs steering values, or that times vector_size");
        this->input_chunk_size  = nBaselines() * vector_size;
        this->output_chunk_size = BS * vector_size;
    }
    [[nodiscard]] work::Status processBulk(std::span<const std::complex<T>> input, std::span<std::complex<T>> output) {
        if (this->input_chunk_size != nBaselines() * vector_size || this->output_chunk_size != static_cast<std::size_t>(n_beams) * n_inputs * vector_size) settingsChanged({}, {});
        using Cd = std::complex<double>;
        const std::size_t S = n_inputs, B = n_beams, N = vector_size, P = nBaselines();
        const float       qnan = std::numeric_limits<float>::quiet_NaN();
        _l.resize(P);
        _y.resize(S);
        const auto tri = [](std::size_t i, std::size_t j) { return i * (i + 1) / 2 + j; };
        for (std::size_t q = 0; (q + 1) * P * N <= input.size(); ++q) {
            for (std::size_t c = 0; c < N; ++c) {
                double tr = 0.0;
                for (std::size_t i = 0; i < S; ++i) {
                    for (std::size_t j = 0; j < i; ++j) _l[tri(i, j)] = Cd(input[(q * P + tri(i, j)) * N + c]);
                    _l[tri(i, i)] = Cd(static_cast<double>(input[(q * P + tri(i, i)) * N + c].real()), 0.0);
                    tr            = tr + _l[tri(i, i)].real();
                }
                const double lambda = loading * tr / static_cast<double>(S);
                for (std::size_t i = 0; i < S; ++i) _l[tri(i, i)] = Cd(_l[tri(i, i)].real() + lambda, 0.0);
                bool ok = true;
                for (std::size_t j = 0; j < S; ++j) { // R' = L L^H in place
                    double sj = _l[tri(j, j)].real();
                    for (std::size_t k = 0; k < j; ++k) sj = sj - std::norm(_l[tri(j, k)]);
                    ok             = ok && (sj > 0.0);
                    const double d = std::sqrt(sj);
                    _l[tri(j, j)]  = Cd(d, 0.0);
                    for (std::size_t i = j + 1; i < S; ++i) {
                        Cd t = _l[tri(i, j)];
                        for (std::size_t k = 0; k < j; ++k) t = t - _l[tri(i, k)] * std::conj(_l[tri(j, k)]);
                        _l[tri(i, j)] = Cd(t.real() / d, t.imag() / d);
                    }
                }
                for (std::size_t b = 0; b < B; ++b) {
                    double d = 0.0;
                    for (std::size_t i = 0; i < S; ++i) { // L y = a_b
                        Cd t = Cd(steer(b, i, c));
                        for (std::size_t k = 0; k < i; ++k) t = t - _l[tri(i, k)] * _y[k];
                        const double lii = _l[tri(i, i)].real();
                        _y[i]            = Cd(t.real() / lii, t.imag() / lii);
                        d                = d + std::norm(_y[i]);
                    }
                    for (std::size_t i = S; i-- > 0;) { // L^H u = y, u over y
                        Cd t = _y[i];
                        for (std::size_t k = i + 1; k < S; ++k) t = t - std::conj(_l[tri(k, i)]) * _y[k];
                        const double lii = _l[tri(i, i)].real();
                        _y[i]            = Cd(t.real() / lii, t.imag() / lii);
                    }
                    for (std::size_t s = 0; s < S; ++s)
                        output[((q * B + b) * S + s) * N + c] = ok ? std::complex<T>(static_cast<float>(_y[s].real() / d), static_cast<float>(-(_y[s].imag() / d))) : std::complex<T>(qnan, qnan);
                }
            }
        }
        return work::Status::OK;
    }
};

// ---- gr::blocks::fft::FFT<T> (blocks/fourier/.../fft.hpp:31-251): one DataSet per frame of fftSize samples
// window (default Hann) -> unnormalised forward DFT -> magnitude (hypot 2/N [dB], fft-shifted) + phase (atan2 [unwrap][deg], shifted) + Re + Im,
// frequency axis, per-signal min/max.  T = std::complex<float> (N bins) or float (N/2 bins: fft.hpp:140-143, 221-227).
// The host body is a float64 DFT (radix-2 for powers of two, the defining sum otherwise) -- plumbing; the device path is gr4hip_fft_process.
template <typename T, typename U = DataSet<float>>
struct FFT : Block<FFT<T, U>, Resampling<1024, 1, false>> {
    using value_type                         = typename U::value_type;
    static constexpr bool computeFullSpectrum = gr::detail::is_complex<T>::value;
    PortIn<T>                         in;
    PortOut<U, RequiredSamples<1, 1>> out;
    Annotated<Size_t, "FFT size">           fftSize{1024U};
    Annotated<std::string, "window type">   window = std::string("Hann");
    Annotated<bool, "output in dB">         outputInDb{false};
    Annotated<bool, "output in deg">        outputInDeg{false};
    Annotated<bool, "unwrap phase">         unwrapPhase{false};
    Annotated<float, "sample rate">         sample_rate = 1.f;
    Annotated<std::string, "signal name">   signal_name = std::string("unknown signal");
    Annotated<std::string, "signal unit">   signal_unit = std::string("a.u.");
    Annotated<float, "signal min">          signal_min  = -std::numeric_limits<float>::max();
    Annotated<float, "signal max">          signal_max  = +std::numeric_limits<float>::max();
    GR_MAKE_REFLECTABLE(FFT, in, out, fftSize, window, outputInDb, outputInDeg, unwrapPhase, sample_rate, signal_name, signal_unit, signal_min, signal_max);

    gr::algorithm::window::Type       _windowType = gr::algorithm::window::Type::Hann;
    std::vector<value_type>           _window;
    std::vector<std::complex<value_type>> _outData;
    std::vector<value_type>           _magnitudeSpectrum, _phaseSpectrum;

    void settingsChanged(const property_map&, const property_map& newSettings) {
        if (!newSettings.contains("fftSize") && !newSettings.contains("window") && !_window.empty()) return; // fft.hpp:126-129
        in.max_samples = in.min_samples = fftSize;
        this->input_chunk_size          = fftSize;
        gr::algorithm::window::Type t   = _windowType;
        if (gr_enum_parse(t, std::string_view(window.value))) _windowType = t; // enum_cast(...).value_or(_windowType) (:138)
        _window = gr::algorithm::window::create<value_type>(_windowType, fftSize);
    }
    [[nodiscard]] std::size_t nBins() const { return computeFullSpectrum ? fftSize.value : fftSize.value / 2; }

    [[nodiscard]] work::Status processBulk(std::span<const T> input, std::span<U> output) {
        const std::size_t N = fftSize;
        if (_window.size() != N) settingsChanged({}, {{"fftSize", std::int64_t(N)}});
        for (std::size_t f = 0; f < output.size(); ++f) {
            std::vector<std::complex<double>> v(N);
            for (std::size_t i = 0; i < N; ++i) v[i] = std::complex<double>(input[f * N + i]) * static_cast<double>(_window[i]);
            dft(v);
            _outData.assign(N, {});
            for (std::size_t i = 0; i < N; ++i) _outData[i] = std::complex<value_type>(static_cast<value_type>(v[i].real()), static_cast<value_type>(v[i].imag()));
            const std::size_t M = nBins();
            _magnitudeSpectrum.assign(M, 0);
            _phaseSpectrum.assign(M, 0);
            for (std::size_t k = 0; k < M; ++k) { // fft_common.hpp:20-56, 91-123
                const value_type mag = std::hypot(_outData[k].real(), _outData[k].imag()) * value_type(2) / static_cast<value_type>(N);
                _magnitudeSpectrum[k] = !outputInDb ? mag : mag > value_type(0) ? value_type(20) * std::log10(mag) : std::numeric_limits<value_type>::lowest();
                _phaseSpectrum[k]     = std::atan2(_outData[k].imag(), _outData[k].real());
            }
            if (unwrapPhase) { // fft_common.hpp:71-89
                const value_type pi = std::numbers::pi_v<value_type>;
                value_type prev = _phaseSpectrum.front();
                for (std::size_t k = 1; k < M; ++k) {
                    value_type& cur = _phaseSpectrum[k];
                    while (cur - prev > pi) cur -= 2 * pi;
                    while (cur - prev < -pi) cur += 2 * pi;
                    prev = cur;
                }
            }
            if (outputInDeg) for (auto& ph : _phaseSpectrum) ph = ph * value_type(180) * std::numbers::inv_pi_v<value_type>;
            if (computeFullSpectrum) {
                std::rotate(_magnitudeSpectrum.begin(), _magnitudeSpectrum.begin() + static_cast<std::ptrdiff_t>(M / 2), _magnitudeSpectrum.end());
                std::rotate(_phaseSpectrum.begin(), _phaseSpectrum.begin() + static_cast<std::ptrdiff_t>(M / 2), _phaseSpectrum.end());
            }
            output[f] = createDataset();
        }
        return work::Status::OK;
    }

    // the descriptive part of the DataSet (everything but signal_values / signal_ranges), fft.hpp:173-250
    [[nodiscard]] U datasetSkeleton() const {
        U ds{};
        const std::size_t N = nBins();
        ds.extents    = {static_cast<std::int32_t>(N)};
        ds.axis_names = {"Frequency"};
        ds.axis_units = {"Hz"};
        ds.axis_values.assign(1, std::vector<value_type>(N));
        const value_type freqWidth = static_cast<value_type>(sample_rate.value) / static_cast<value_type>(fftSize.value);
        const value_type freqOffset = computeFullSpectrum ? static_cast<value_type>(N / 2) * freqWidth : value_type(0);
        for (std::size_t i = 0; i < N; ++i) ds.axis_values[0][i] = static_cast<value_type>(i) * freqWidth - freqOffset;
        const std::string& n = signal_name.value;
        ds.signal_names      = {"Magnitude(" + n + ")", "Phase(" + n + ")", "Re(FFT(" + n + "))", "Im(FFT(" + n + "))"};
        ds.signal_quantities = {"Magnitude(FFT)", "Phase(FFT)", "Re(FFT)", "Im(FFT)"};
        ds.signal_units      = {signal_unit.value + "/\u221aHz", "rad", "Re" + signal_unit.value, "Im" + signal_unit.value};
        ds.signal_values.assign(4 * N, 0);
        ds.signal_ranges.assign(4, {});
        typename decltype(ds.meta_information)::value_type meta{{"sample_rate", sample_rate.value}, {"window", window.value}, {"output_in_db", outputInDb.value},
            {"output_in_deg", outputInDeg.value}, {"unwrap_phase", unwrapPhase.value}, {"input_chunk_size", std::uint64_t(this->input_chunk_size)},
            {"output_chunk_size", std::uint64_t(this->output_chunk_size)}};
        ds.meta_information.assign(4, meta);
        return ds;
    }
    [[nodiscard]] U createDataset() const {
        U                 ds = datasetSkeleton();
        const std::size_t N  = nBins();
        std::copy_n(_magnitudeSpectrum.begin(), N, ds.signalValues(0).begin());
        std::copy_n(_phaseSpectrum.begin(), N, ds.signalValues(1).begin());
        const auto spec = std::span<const std::complex<value_type>>(_outData).last(N); // real input: the upper half (fft.hpp:221-227)
        for (std::size_t i = 0; i < N; ++i) {
            ds.signalValues(2)[i] = spec[i].real();
            ds.signalValues(3)[i] = spec[i].imag();
        }
        for (std::size_t i = 0; i < 4; ++i) {
            const auto sv       = ds.signalValues(i);
            const auto mm       = std::minmax_element(sv.begin(), sv.end());
            ds.signal_ranges[i] = {*mm.first, *mm.second};
        }
        return ds;
    }

private:
    static void dft(std::vector<std::complex<double>>& v) {
        const std::size_t N = v.size();
        if (N && !(N & (N - 1))) {
            for (std::size_t i = 1, j = 0; i < N; ++i) {
                std::size_t bit = N >> 1;
                for (; j & bit; bit >>= 1) j ^= bit;
                j ^= bit;
                if (i < j) std::swap(v[i], v[j]);
            }
            for (std::size_t len = 2; len <= N; len <<= 1)
                for (std::size_t k = 0; k < N; k += len)
                    for (std::size_t n = 0; n < len / 2; ++n) {
                        const auto w = std::polar(1.0, -2.0 * std::numbers::pi * static_cast<double>(n) / static_cast<double>(len));
                        const auto t = v[k + n + len / 2] * w;
                        v[k + n + len / 2] = v[k + n] - t;
                        v[k + n] += t;
                    }
            return;
        }
        std::vector<std::complex<double>> o(N);
        for (std::size_t k = 0; k < N; ++k)
            for (std::size_t n = 0; n < N; ++n) o[k] += v[n] * std::polar(1.0, -2.0 * std::numbers::pi * static_cast<double>((k * n) % N) / static_cast<double>(N));
        v = std::move(o);
    }
};
} // namespace gr::blocks::fft

// ---- the type-converter blocks (blocks/basic/.../ConverterBlocks.hpp:13-277) under the reference's names and port names.  The host bodies are the reference's
// expressions with the integer / cast rules of gr4/converter_ops.hpp where its C++ is undefined (CONVERTERS.md), the same header the device kernels use: the two
// domains of a block agree on every input.  Ports that are not called in / out go through hostWork() (the default work loop knows only that pair).
namespace gr::blocks::type::converter {
namespace ops = gr4::converter_ops;
namespace detail {
template <typename T> struct base_value { using type = T; };
template <typename T> struct base_value<std::complex<T>> { using type = T; };
template <typename T> using base_value_t = typename base_value<T>::type; // meta::fundamental_base_value_type_t
template <typename T> concept complex_like = gr::detail::is_complex<T>::value;
template <typename T> concept interleavable = std::floating_point<T> || std::is_same_v<T, std::int8_t> || std::is_same_v<T, std::int16_t>;

template <typename P>
std::span<typename P::value_type> out_span(P& port, std::size_t n, std::vector<typename P::value_type>& scratch) {
    if (port.connected()) return port.buffer->write_span(n);
    scratch.resize(n);
    return scratch;
}
template <typename B, typename PI, typename PO>
work::Status map11(B& b, PI& in, PO& out, std::size_t n) {
    std::vector<typename PO::value_type> s;
    const auto is = in.buffer->read_span(n);
    auto       os = out_span(out, n, s);
    for (std::size_t i = 0; i < n; ++i) os[i] = b.processOne(is[i]);
    return work::Status::OK;
}
template <typename B, typename PI, typename PO>
work::Status map12(B& b, PI& in, PO& out0, PO& out1, std::size_t n) {
    std::vector<typename PO::value_type> s0, s1;
    const auto is = in.buffer->read_span(n);
    auto       o0 = out_span(out0, n, s0), o1 = out_span(out1, n, s1);
    for (std::size_t i = 0; i < n; ++i) std::tie(o0[i], o1[i]) = b.processOne(is[i]);
    return work::Status::OK;
}
template <typename B, typename PI, typename PO>
work::Status map21(B& b, PI& in0, PI& in1, PO& out, std::size_t n) {
    std::vector<typename PO::value_type> s;
    const auto i0 = in0.buffer->read_span(n), i1 = in1.buffer->read_span(n);
    auto       os = out_span(out, n, s);
    for (std::size_t i = 0; i < n; ++i) os[i] = b.processOne(i0[i], i1[i]);
    return work::Status::OK;
}
} // namespace detail

GR_REGISTER_BLOCK(gr::blocks::type::converter::Convert, ([T], [U]), [ uint8_t, uint16_t, uint32_t, uint64_t, int8_t, int16_t, int32_t, int64_t, float, double ], [ uint8_t, uint16_t, uint32_t, uint64_t, int8_t, int16_t, int32_t, int64_t, float, double ])
template <typename T, typename R>
    requires std::is_arithmetic_v<T> && std::is_arithmetic_v<R>
struct Convert : Block<Convert<T, R>> { // (:15-33)
    PortIn<T>  in;
    PortOut<R> out;
    GR_MAKE_REFLECTABLE(Convert, in, out);
    static constexpr int kConvertKind = GR4HIP_CONVERT; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(out); }
    [[nodiscard]] constexpr R processOne(const T& input) const noexcept { return ops::cast<R>(input); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::ScalingConvert, ([T], [U]), [ uint8_t, uint16_t, uint32_t, uint64_t, int8_t, int16_t, int32_t, int64_t, float, double ], [ uint8_t, uint16_t, uint32_t, uint64_t, int8_t, int16_t, int32_t, int64_t, float, double ])
template <typename T, typename R>
    requires std::is_arithmetic_v<T> && std::is_arithmetic_v<R>
struct ScalingConvert : Block<ScalingConvert<T, R>> { // (:37-59): R output = R(input * scale), the product in the promoted type
    PortIn<T>  in;
    PortOut<R> out;
    T          scale = static_cast<T>(1);
    GR_MAKE_REFLECTABLE(ScalingConvert, in, out, scale);
    static constexpr int kConvertKind = GR4HIP_SCALING_CONVERT; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(out); }
    [[nodiscard]] constexpr R processOne(const T& input) const noexcept { return ops::cast<R>(ops::mul<T>(input, scale)); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::Abs, [T], [ uint8_t, uint16_t, uint32_t, uint64_t, int8_t, int16_t, int32_t, int64_t, float, double, std::complex<float>, std::complex<double> ])
template <typename T>
    requires std::is_arithmetic_v<T> || detail::complex_like<T>
struct Abs : Block<Abs<T>> { // (:63-81)
    using R = detail::base_value_t<T>;
    PortIn<T>  in;
    PortOut<R> abs;
    GR_MAKE_REFLECTABLE(Abs, in, abs);
    static constexpr int kConvertKind = GR4HIP_CONVERT_ABS; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(abs); }
    [[nodiscard]] R processOne(T input) const noexcept {
        if constexpr (std::is_integral_v<T>) return ops::abs_int<T>(input);
        else return static_cast<R>(std::abs(input));
    }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map11(*this, in, abs, nIn); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::Imag, [T], [ std::complex<float>, std::complex<double> ])
template <detail::complex_like T>
struct Imag : Block<Imag<T>> { // (:85-96)
    using R = detail::base_value_t<T>;
    PortIn<T>  in;
    PortOut<R> imag;
    GR_MAKE_REFLECTABLE(Imag, in, imag);
    static constexpr int kConvertKind = GR4HIP_CONVERT_IMAG; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(imag); }
    [[nodiscard]] constexpr R processOne(T input) const noexcept { return std::imag(input); }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map11(*this, in, imag, nIn); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::Real, [T], [ std::complex<float>, std::complex<double> ])
template <detail::complex_like T>
struct Real : Block<Real<T>> { // (:100-111)
    using R = detail::base_value_t<T>;
    PortIn<T>  in;
    PortOut<R> real;
    GR_MAKE_REFLECTABLE(Real, in, real);
    static constexpr int kConvertKind = GR4HIP_CONVERT_REAL; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(real); }
    [[nodiscard]] constexpr R processOne(T input) const noexcept { return std::real(input); }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map11(*this, in, real, nIn); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::Arg, [T], [ std::complex<float>, std::complex<double> ])
template <detail::complex_like T>
struct Arg : Block<Arg<T>> { // (:115-126)
    using R = detail::base_value_t<T>;
    PortIn<T>  in;
    PortOut<R> arg;
    GR_MAKE_REFLECTABLE(Arg, in, arg);
    static constexpr int kConvertKind = GR4HIP_CONVERT_ARG; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(arg); }
    [[nodiscard]] R processOne(T input) const noexcept { return std::arg(input); }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map11(*this, in, arg, nIn); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::RadiansToDegree, [T], [ float, double ])
template <std::floating_point T>
struct RadiansToDegree : Block<RadiansToDegree<T>> { // (:130-143): a division, then a multiplication
    PortIn<T>  rad;
    PortOut<T> deg;
    GR_MAKE_REFLECTABLE(RadiansToDegree, rad, deg);
    static constexpr int kConvertKind = GR4HIP_RADIANS_TO_DEGREE; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(rad); }
    auto outPorts() { return std::tie(deg); }
    [[nodiscard]] constexpr T processOne(const T& radians) const noexcept { return (radians / std::numbers::pi_v<T>)*static_cast<T>(180); }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map11(*this, rad, deg, nIn); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::DegreeToRadians, [T], [ float, double ])
template <std::floating_point T>
struct DegreeToRadians : Block<DegreeToRadians<T>> { // (:147-160)
    PortIn<T>  deg;
    PortOut<T> rad;
    GR_MAKE_REFLECTABLE(DegreeToRadians, deg, rad);
    static constexpr int kConvertKind = GR4HIP_DEGREE_TO_RADIANS; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(deg); }
    auto outPorts() { return std::tie(rad); }
    [[nodiscard]] constexpr T processOne(const T& degree) const noexcept { return (degree / static_cast<T>(180)) * std::numbers::pi_v<T>; }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map11(*this, deg, rad, nIn); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::ToRealImag, [T], [ std::complex<float>, std::complex<double> ])
template <detail::complex_like T>
struct ToRealImag : Block<ToRealImag<T>> { // (:164-178)
    using R = detail::base_value_t<T>;
    PortIn<T>  in;
    PortOut<R> real;
    PortOut<R> imag;
    GR_MAKE_REFLECTABLE(ToRealImag, in, real, imag);
    static constexpr int kConvertKind = GR4HIP_TO_REAL_IMAG; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(real, imag); }
    [[nodiscard]] constexpr std::tuple<R, R> processOne(T complexIn) const noexcept { return {std::real(complexIn), std::imag(complexIn)}; }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map12(*this, in, real, imag, nIn); }
};

// DEVIATION: the reference's registration macros of the next three blocks repeat the name ToRealImag (:180, :197, :215); each is registered under its own name here
GR_REGISTER_BLOCK(gr::blocks::type::converter::RealImagToComplex, [T], [ float, double ])
template <std::floating_point T>
struct RealImagToComplex : Block<RealImagToComplex<T>> { // (:182-195)
    using R = std::complex<T>;
    PortIn<T>  real;
    PortIn<T>  imag;
    PortOut<R> out;
    GR_MAKE_REFLECTABLE(RealImagToComplex, real, imag, out);
    static constexpr int kConvertKind = GR4HIP_REAL_IMAG_TO_COMPLEX; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(real, imag); }
    auto outPorts() { return std::tie(out); }
    [[nodiscard]] constexpr R processOne(T re, T im) const noexcept { return {re, im}; }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map21(*this, real, imag, out, nIn); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::ToMagPhase, [T], [ std::complex<float>, std::complex<double> ])
template <detail::complex_like T>
struct ToMagPhase : Block<ToMagPhase<T>> { // (:199-213)
    using R = detail::base_value_t<T>;
    PortIn<T>  in;
    PortOut<R> mag;
    PortOut<R> phase;
    GR_MAKE_REFLECTABLE(ToMagPhase, in, mag, phase);
    static constexpr int kConvertKind = GR4HIP_TO_MAG_PHASE; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(mag, phase); }
    [[nodiscard]] std::tuple<R, R> processOne(T complexIn) const noexcept { return {static_cast<R>(std::abs(complexIn)), static_cast<R>(std::arg(complexIn))}; }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map12(*this, in, mag, phase, nIn); }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::MagPhaseToComplex, [T], [ float, double ])
template <std::floating_point T>
struct MagPhaseToComplex : Block<MagPhaseToComplex<T>> { // (:217-231): {r cos theta, r sin theta} (std::polar's value without its precondition on r)
    using R = std::complex<T>;
    PortIn<T>  mag;
    PortIn<T>  phase;
    PortOut<R> out;
    GR_MAKE_REFLECTABLE(MagPhaseToComplex, mag, phase, out);
    static constexpr int kConvertKind = GR4HIP_MAG_PHASE_TO_COMPLEX; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(mag, phase); }
    auto outPorts() { return std::tie(out); }
    [[nodiscard]] R processOne(T r, T theta) const noexcept { return {r * std::cos(theta), r * std::sin(theta)}; }
    work::Status hostWork(std::size_t nIn, std::size_t) { return detail::map21(*this, mag, phase, out, nIn); }
};

// (the templates' constraint, wider than the reference's registration: the int8 / int16 variants are registered too -- the interleaved I/Q of an SDR or ADC)
GR_REGISTER_BLOCK(gr::blocks::type::converter::ComplexToInterleaved, ([T], [U]), [ std::complex<float>, std::complex<double> ], [ float, double, int8_t, int16_t ])
template <detail::complex_like T, detail::interleavable R>
struct ComplexToInterleaved : Block<ComplexToInterleaved<T, R>, Resampling<1U, 2U, true>> { // (:235-254)
    PortIn<T>  in;
    PortOut<R> interleaved;
    GR_MAKE_REFLECTABLE(ComplexToInterleaved, in, interleaved);
    static constexpr int kConvertKind = GR4HIP_COMPLEX_TO_INTERLEAVED; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(in); }
    auto outPorts() { return std::tie(interleaved); }
    [[nodiscard]] constexpr work::Status processBulk(std::span<const T> complexInput, std::span<R> interleavedOut) const noexcept {
        for (std::size_t i = 0; i < complexInput.size(); ++i) {
            interleavedOut[2 * i]     = ops::cast<R>(complexInput[i].real());
            interleavedOut[2 * i + 1] = ops::cast<R>(complexInput[i].imag());
        }
        return work::Status::OK;
    }
    work::Status hostWork(std::size_t nIn, std::size_t nOut) {
        std::vector<R> s;
        return processBulk(in.buffer->read_span(nIn), detail::out_span(interleaved, nOut, s));
    }
};

GR_REGISTER_BLOCK(gr::blocks::type::converter::InterleavedToComplex, ([T], [U]), [ float, double, int8_t, int16_t ], [ std::complex<float>, std::complex<double> ])
template <detail::interleavable T, detail::complex_like R>
struct InterleavedToComplex : Block<InterleavedToComplex<T, R>, Resampling<2U, 1U, true>> { // (:258-277)
    PortIn<T>  interleaved;
    PortOut<R> out;
    GR_MAKE_REFLECTABLE(InterleavedToComplex, interleaved, out);
    static constexpr int kConvertKind = GR4HIP_INTERLEAVED_TO_COMPLEX; // the device kernel family of this block (gr4/hip.hpp)
    auto inPorts() { return std::tie(interleaved); }
    auto outPorts() { return std::tie(out); }
    [[nodiscard]] constexpr work::Status processBulk(std::span<const T> interleavedInput, std::span<R> complexOut) const noexcept {
        for (std::size_t i = 0; i < complexOut.size(); ++i)
            complexOut[i] = R{static_cast<typename R::value_type>(interleavedInput[2 * i]), static_cast<typename R::value_type>(interleavedInput[2 * i + 1])};
        return work::Status::OK;
    }
    work::Status hostWork(std::size_t nIn, std::size_t nOut) {
        std::vector<R> s;
        return processBulk(interleaved.buffer->read_span(nIn), detail::out_span(out, nOut, s));
    }
};
} // namespace gr::blocks::type::converter
