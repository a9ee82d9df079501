// The type-converter mirror blocks (gr4/blocks.hpp, gr::blocks::type::converter), host domain.
//   test_host_converter <dir> [scale]
// reads <dir>/in0_<type>.bin and <dir>/in1_<type>.bin (raw samples; type = u8 ... f64, c32, c64) and writes each output port to
// <dir>/<Kind>_<in>_<out>_<port>.bin; tests/test_converter_host.py compares the files with tests/converter_oracle.py.
//   * every kind and registered type pair through the block's own processOne / processBulk (246 block types);
//   * every kind once more as a graph, VectorSource -> block -> VectorSink(s), with the ports under the reference's names: <dir>/graph_<Kind>_..., which must
//     equal the direct call's file.  (Only these: a work loop per block type costs a second of compile time each, and the loop is the same code for all.)
// ScalingConvert runs with `scale` (default 3).  Exit code 0: every block ran; 1: one did not.
//   test_host_converter --device <dir> <plugin.so>
// the same inputs on compute_domain gpu:hip:0:
//   * every kind as a graph through the device seam (Kernel<> of gr4/hip.hpp): <dir>/dev_<Kind>_...;
//   * the ingest graph VectorSource<int16> -> InterleavedToComplex<int16, complex<float>> -> MultiplyConst -> Rotator -> fir_filter (31 taps) -> sink planned by
//     hip::plan (the run takes the samples to HBM and back): converter, gain and rotator must be ONE stage, and the result must be within 1e-5 (relative to the
//     larger of the sample and the rms) of the same graph with converter, gain and rotator in the host domain;
//   * the narrowing graph PowerSpectrum (gpu) -> Convert<float, int16> (gpu) against PowerSpectrum (gpu) -> Convert (host), bit for bit;
//   * the plugin: every converter name of the reference's lists is registered, and ToMagPhase<complex<float32>> made by name with compute_domain gpu:hip:0 feeds
//     two sinks (<dir>/plugin_mag.bin, plugin_phase.bin).
// Exit code 0: all passed; 1: a comparison failed; 3: a device block reported work::Status::ERROR (what must happen without a GPU: never a host fallback).
#include <complex>
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
namespace cv = gr::blocks::type::converter;

template <typename T> constexpr const char* tname() {
    if constexpr (std::is_same_v<T, std::uint8_t>) return "u8"; else if constexpr (std::is_same_v<T, std::uint16_t>) return "u16";
    else if constexpr (std::is_same_v<T, std::uint32_t>) return "u32"; else if constexpr (std::is_same_v<T, std::uint64_t>) return "u64";
    else if constexpr (std::is_same_v<T, std::int8_t>) return "i8"; else if constexpr (std::is_same_v<T, std::int16_t>) return "i16";
    else if constexpr (std::is_same_v<T, std::int32_t>) return "i32"; else if constexpr (std::is_same_v<T, std::int64_t>) return "i64";
    else if constexpr (std::is_same_v<T, float>) return "f32"; else if constexpr (std::is_same_v<T, double>) return "f64";
    else if constexpr (std::is_same_v<T, std::complex<float>>) return "c32"; else return "c64";
}

static std::string g_dir;
static double      g_scale  = 3.0;
static int         g_errors = 0, g_graphs = 0, g_blocks = 0, g_failures = 0;
static std::string g_domain = "host", g_prefix = "graph_";

template <typename T>
static std::vector<T> load(int port) {
    std::ifstream  f(g_dir + "/in" + std::to_string(port) + "_" + tname<T>() + ".bin", std::ios::binary | std::ios::ate);
    std::vector<T> v;
    if (!f) { std::cerr << "missing input for " << tname<T>() << "\n"; ++g_errors; return v; }
    v.resize(static_cast<std::size_t>(f.tellg()) / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
    return v;
}
template <typename T>
static void store(const std::string& name, const std::vector<T>& v) {
    std::ofstream f(g_dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

// the block's own processOne / processBulk over the whole input
template <typename B, typename TI, typename TO>
static void direct(const char* kind, std::initializer_list<const char*> outs, const property_map& settings = {}) {
    ++g_blocks;
    B b;
    b.applySettings(settings);
    const std::vector<TI> x0 = load<TI>(0);
    const std::string     stem = std::string(kind) + "_" + tname<TI>() + "_" + tname<TO>() + "_";
    const char* const*    name = outs.begin();
    if constexpr (requires(std::span<const TI> i, std::span<TO> o) { b.processBulk(i, o); }) {
        constexpr std::size_t ic = B::ResamplingControl::kIn, oc = B::ResamplingControl::kOut;
        std::vector<TO>       y(x0.size() / ic * oc);
        if (b.processBulk(std::span<const TI>(x0.data(), x0.size() / ic * ic), std::span<TO>(y)) != work::Status::OK) ++g_errors;
        store(stem + name[0], y);
    } else if constexpr (requires(TI v) { { b.processOne(v, v) }; }) {
        const std::vector<TI> x1 = load<TI>(1);
        std::vector<TO>       y(std::min(x0.size(), x1.size()));
        for (std::size_t i = 0; i < y.size(); ++i) y[i] = b.processOne(x0[i], x1[i]);
        store(stem + name[0], y);
    } else if constexpr (requires(TI v) { { b.processOne(v) } -> std::convertible_to<TO>; }) {
        std::vector<TO> y(x0.size());
        for (std::size_t i = 0; i < y.size(); ++i) y[i] = b.processOne(x0[i]);
        store(stem + name[0], y);
    } else {
        std::vector<TO> y0(x0.size()), y1(x0.size());
        for (std::size_t i = 0; i < x0.size(); ++i) std::tie(y0[i], y1[i]) = b.processOne(x0[i]);
        store(stem + name[0], y0);
        store(stem + name[1], y1);
    }
}

// one block between sources and sinks; `ins` / `outs` are its port names in declaration order
template <typename B, typename TI, typename TO>
static void graph(const char* kind, std::initializer_list<const char*> ins, std::initializer_list<const char*> outs, const property_map& settings = {}) {
    ++g_graphs;
    Graph        g;
    property_map with_domain = settings;
    with_domain.insert_or_assign("compute_domain", g_domain);
    auto& blk = g.emplaceBlock<B>(with_domain);
    blk._log  = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    bool  ok  = true;
    int   p   = 0;
    for (const char* name : ins) {
        auto& src  = g.emplaceBlock<testing::VectorSource<TI>>();
        src.values = load<TI>(p++);
        ok         = ok && g.connect(src, "out", blk, name).has_value();
    }
    std::vector<testing::VectorSink<TO>*> sinks;
    for (const char* name : outs) {
        sinks.push_back(&g.emplaceBlock<testing::VectorSink<TO>>());
        ok = ok && g.connect(blk, name, *sinks.back(), "in").has_value();
    }
    if (!ok) { std::cerr << kind << ": connect failed\n"; ++g_errors; return; }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) { std::cerr << kind << "<" << tname<TI>() << ", " << tname<TO>() << ">: " << r.error().message << "\n"; ++g_errors; return; }
    std::size_t q = 0;
    for (const char* name : outs) store(g_prefix + kind + "_" + tname<TI>() + "_" + tname<TO>() + "_" + name, sinks[q++]->_samples);
}

template <typename T, typename R>
static void convert_pair() {
    direct<cv::Convert<T, R>, T, R>("Convert", {"out"});
    direct<cv::ScalingConvert<T, R>, T, R>("ScalingConvert", {"out"}, {{"scale", g_scale}});
}
template <typename T>
static void arithmetic_from() {
    convert_pair<T, std::uint8_t>(); convert_pair<T, std::uint16_t>(); convert_pair<T, std::uint32_t>(); convert_pair<T, std::uint64_t>();
    convert_pair<T, std::int8_t>(); convert_pair<T, std::int16_t>(); convert_pair<T, std::int32_t>(); convert_pair<T, std::int64_t>();
    convert_pair<T, float>(); convert_pair<T, double>();
    direct<cv::Abs<T>, T, T>("Abs", {"abs"});
}
template <typename F>
static void float_kinds() {
    using C = std::complex<F>;
    direct<cv::Abs<C>, C, F>("Abs", {"abs"});
    direct<cv::Real<C>, C, F>("Real", {"real"});
    direct<cv::Imag<C>, C, F>("Imag", {"imag"});
    direct<cv::Arg<C>, C, F>("Arg", {"arg"});
    direct<cv::RadiansToDegree<F>, F, F>("RadiansToDegree", {"deg"});
    direct<cv::DegreeToRadians<F>, F, F>("DegreeToRadians", {"rad"});
    direct<cv::ToRealImag<C>, C, F>("ToRealImag", {"real", "imag"});
    direct<cv::RealImagToComplex<F>, F, C>("RealImagToComplex", {"out"});
    direct<cv::ToMagPhase<C>, C, F>("ToMagPhase", {"mag", "phase"});
    direct<cv::MagPhaseToComplex<F>, F, C>("MagPhaseToComplex", {"out"});
    direct<cv::ComplexToInterleaved<C, float>, C, float>("ComplexToInterleaved", {"interleaved"});
    direct<cv::ComplexToInterleaved<C, double>, C, double>("ComplexToInterleaved", {"interleaved"});
    direct<cv::ComplexToInterleaved<C, std::int8_t>, C, std::int8_t>("ComplexToInterleaved", {"interleaved"});
    direct<cv::ComplexToInterleaved<C, std::int16_t>, C, std::int16_t>("ComplexToInterleaved", {"interleaved"});
    direct<cv::InterleavedToComplex<float, C>, float, C>("InterleavedToComplex", {"out"});
    direct<cv::InterleavedToComplex<double, C>, double, C>("InterleavedToComplex", {"out"});
    direct<cv::InterleavedToComplex<std::int8_t, C>, std::int8_t, C>("InterleavedToComplex", {"out"});
    direct<cv::InterleavedToComplex<std::int16_t, C>, std::int16_t, C>("InterleavedToComplex", {"out"});
}

static void every_kind_as_a_graph() {
    using C = std::complex<float>;
    graph<cv::Convert<float, std::int16_t>, float, std::int16_t>("Convert", {"in"}, {"out"});
    graph<cv::ScalingConvert<std::uint8_t, float>, std::uint8_t, float>("ScalingConvert", {"in"}, {"out"}, {{"scale", g_scale}});
    graph<cv::Abs<C>, C, float>("Abs", {"in"}, {"abs"});
    graph<cv::Real<C>, C, float>("Real", {"in"}, {"real"});
    graph<cv::Imag<C>, C, float>("Imag", {"in"}, {"imag"});
    graph<cv::Arg<C>, C, float>("Arg", {"in"}, {"arg"});
    graph<cv::RadiansToDegree<float>, float, float>("RadiansToDegree", {"rad"}, {"deg"});
    graph<cv::DegreeToRadians<double>, double, double>("DegreeToRadians", {"deg"}, {"rad"});
    graph<cv::ToRealImag<C>, C, float>("ToRealImag", {"in"}, {"real", "imag"});
    graph<cv::RealImagToComplex<float>, float, C>("RealImagToComplex", {"real", "imag"}, {"out"});
    graph<cv::ToMagPhase<C>, C, float>("ToMagPhase", {"in"}, {"mag", "phase"});
    graph<cv::MagPhaseToComplex<float>, float, C>("MagPhaseToComplex", {"mag", "phase"}, {"out"});
    graph<cv::ComplexToInterleaved<C, std::int16_t>, C, std::int16_t>("ComplexToInterleaved", {"in"}, {"interleaved"});
    graph<cv::InterleavedToComplex<std::int16_t, C>, std::int16_t, C>("InterleavedToComplex", {"interleaved"}, {"out"});
}

#define EXPECT(cond) do { if (!(cond)) { ++g_failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

// VectorSource<int16> -> InterleavedToComplex -> MultiplyConst -> Rotator -> fir_filter -> sink; `front`: the domain of converter, gain and rotator
static std::vector<std::complex<float>> ingest(const std::string& front, std::string* description) {
    using C = std::complex<float>;
    std::vector<double> taps(31);
    for (std::size_t k = 0; k < taps.size(); ++k) taps[k] = (0.54 - 0.46 * std::cos(2.0 * 3.14159265358979323846 * double(k) / 30.0)) / 16.0;
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<std::int16_t>>();
    src.values = load<std::int16_t>(0);
    src.values.resize(std::min<std::size_t>(src.values.size(), 8192) / 2 * 2);
    auto& conv = g.emplaceBlock<cv::InterleavedToComplex<std::int16_t, C>>({{"compute_domain", front}});
    auto& gain = g.emplaceBlock<blocks::math::MultiplyConst<C>>({{"value", C(1.f / 32768.f, 0.f)}, {"compute_domain", front}});
    auto& rot  = g.emplaceBlock<blocks::math::Rotator<C>>({{"phase_increment", 0.0078125}, {"compute_domain", front}}); // 2^-7: the host's float phase walk is exact
    auto& fir  = g.emplaceBlock<filter::fir_filter<C>>({{"b", taps}, {"compute_domain", std::string("gpu:hip:0")}});
    auto& sink = g.emplaceBlock<testing::VectorSink<C>>();
    for (auto* log : {&conv._log, &gain._log, &rot._log, &fir._log}) *log = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    if (!g.connect(src, "out", conv, "interleaved") || !g.connect(conv, "out", gain, "in") || !g.connect(gain, "out", rot, "in") || !g.connect(rot, "out", fir, "in") ||
        !g.connect(fir, "out", sink, "in")) { ++g_errors; return {}; }
    const auto runs = hip::plan(g);
    if (description) *description = runs.size() == 1 ? std::string(runs[0]->description()) : std::to_string(runs.size()) + " runs";
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) { std::cerr << "ingest graph (" << front << "): " << r.error().message << "\n"; ++g_errors; }
    return sink._samples;
}

static std::vector<std::int16_t> narrowing(const std::string& convert_domain) {
    using C = std::complex<float>;
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<C>>();
    src.values.resize(16 * 256);
    unsigned long long s = 12345;
    for (auto& v : src.values) { // a tone in noise: the spectrum spans int16's range and goes past it
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const float a = float((s >> 40) & 0xffff) / 65536.f - 0.5f;
        const auto  k = static_cast<double>(&v - src.values.data());
        v = C(3.f * float(std::cos(0.3 * k)) + a, 3.f * float(std::sin(0.3 * k)) - a);
    }
    auto& spec = g.emplaceBlock<blocks::fft::PowerSpectrum<C>>({{"fftSize", std::int64_t(256)}, {"window", std::string("Hann")}, {"compute_domain", std::string("gpu:hip:0")}});
    auto& conv = g.emplaceBlock<cv::Convert<float, std::int16_t>>({{"compute_domain", convert_domain}});
    auto& sink = g.emplaceBlock<testing::VectorSink<std::int16_t>>();
    spec._log = conv._log = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    if (!g.connect(src, "out", spec, "in") || !g.connect(spec, "out", conv, "in") || !g.connect(conv, "out", sink, "in")) { ++g_errors; return {}; }
    const auto runs = hip::plan(g);
    if (convert_domain != "host") EXPECT(runs.size() == 1 && runs[0]->description().find("convert_Convert_f32_i16") != std::string::npos);
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) { std::cerr << "narrowing graph (" << convert_domain << "): " << r.error().message << "\n"; ++g_errors; }
    return sink._samples;
}

// one block between a source and ONE sink on `out`; tags on the source (settings by tag)
template <typename B, typename TI, typename TO>
static std::vector<TO> one_sink(const std::string& domain, const char* in, const char* out, property_map settings, const std::vector<Tag>& tags, std::size_t* by_tag = nullptr) {
    Graph g;
    settings.insert_or_assign("compute_domain", domain);
    auto& blk  = g.emplaceBlock<B>(settings);
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& src  = g.emplaceBlock<testing::VectorSource<TI>>();
    src.values = load<TI>(0);
    src._tags  = tags;
    auto& sink = g.emplaceBlock<testing::VectorSink<TO>>();
    if (!g.connect(src, "out", blk, in) || !g.connect(blk, out, sink, "in")) { ++g_errors; return {}; }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) { std::cerr << "one_sink (" << domain << "): " << r.error().message << "\n"; ++g_errors; }
    if (by_tag) *by_tag = blk._settings_by_tag;
    return sink._samples;
}
// the seam's other two paths, device against the host block bit for bit (both kinds are exact arithmetic): ToRealImag with `imag` open -- a NULL pointer in the
// call, not copied back --, and ScalingConvert's scale changed by a settings tag in mid-stream
static void open_output_and_new_scale() {
    using C = std::complex<float>;
    const auto dr = one_sink<cv::ToRealImag<C>, C, float>("gpu:hip:0", "in", "real", {}, {}), hr = one_sink<cv::ToRealImag<C>, C, float>("host", "in", "real", {}, {});
    const bool same_r = !dr.empty() && dr.size() == hr.size() && std::memcmp(dr.data(), hr.data(), dr.size() * sizeof(float)) == 0;
    std::printf("ToRealImag with `imag` open: %zu samples, device == host: %s\n", dr.size(), same_r ? "bit for bit" : "FAILED");
    EXPECT(same_r);
    const std::size_t      n = load<std::uint8_t>(0).size(), at = n / 2;
    const std::vector<Tag> rescale{{at, {{"scale", 0.25}}}};
    std::size_t            by_tag[2] = {0, 0};
    const auto ds = one_sink<cv::ScalingConvert<std::uint8_t, float>, std::uint8_t, float>("gpu:hip:0", "in", "out", {{"scale", g_scale}}, rescale, &by_tag[0]);
    const auto hs = one_sink<cv::ScalingConvert<std::uint8_t, float>, std::uint8_t, float>("host", "in", "out", {{"scale", g_scale}}, rescale, &by_tag[1]);
    const auto h0 = one_sink<cv::ScalingConvert<std::uint8_t, float>, std::uint8_t, float>("host", "in", "out", {{"scale", g_scale}}, {});
    const bool same_s = ds.size() == n && hs.size() == n && std::memcmp(ds.data(), hs.data(), n * sizeof(float)) == 0;
    const bool stepped = h0.size() == n && std::equal(hs.begin(), hs.begin() + static_cast<std::ptrdiff_t>(at), h0.begin()) && !std::equal(hs.begin() + static_cast<std::ptrdiff_t>(at), hs.end(), h0.begin() + static_cast<std::ptrdiff_t>(at));
    std::printf("ScalingConvert scale by settings in mid-stream: %zu samples, device == host: %s\n", ds.size(), same_s && stepped ? "bit for bit" : "FAILED");
    EXPECT(same_s && stepped && by_tag[0] == 1 && by_tag[1] == 1);
}

static void plugin_checks(const char* path) {
    using namespace std::string_literals;
    PluginLoader loader;
    const auto   ok = loader.load(path);
    if (!ok) { std::cerr << ok.error().message << "\n"; ++g_failures; return; }
    const char* arith[] = {"uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64", "float32", "float64"};
    const std::string ns = "gr::blocks::type::converter::";
    std::size_t n = 0;
    const auto  have = [&](const std::string& name) { ++n; if (!loader.isBlockAvailable(name)) { ++g_failures; std::printf("FAILED: %s is not registered\n", name.c_str()); } };
    for (const char* t : arith) {
        for (const char* r : arith) { have(ns + "Convert<" + t + ", " + r + ">"); have(ns + "ScalingConvert<" + t + ", " + r + ">"); }
        have(ns + "Abs<" + t + ">");
    }
    for (const char* f : {"float32", "float64"}) {
        const std::string c = "complex<"s + f + ">";
        for (const char* k : {"Abs", "Real", "Imag", "Arg", "ToRealImag", "ToMagPhase"}) have(ns + k + "<" + c + ">");
        for (const char* k : {"RadiansToDegree", "DegreeToRadians", "RealImagToComplex", "MagPhaseToComplex"}) have(ns + k + "<" + f + ">");
        for (const char* r : {"float32", "float64", "int8", "int16"}) { have(ns + "ComplexToInterleaved<" + c + ", " + r + ">"); have(ns + "InterleavedToComplex<" + r + ", " + c + ">"); }
    }
    EXPECT(n == 246);
    EXPECT(!loader.isBlockAvailable(ns + "Convert<complex<float32>, float32>"));
    Graph g;
    auto& src = g.addBlock(loader.instantiate("gr::testing::VectorSource<complex<float32>>"));
    auto& tmp = g.addBlock(loader.instantiate(ns + "ToMagPhase<complex<float32>>", {{"compute_domain", "gpu:hip:0"s}}));
    auto& mag = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
    auto& ph  = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
    static_cast<testing::VectorSource<std::complex<float>>*>(src.raw())->values = load<std::complex<float>>(0);
    EXPECT(g.connect(src, "out"s, tmp, "in"s).has_value() && g.connect(tmp, "mag"s, mag, "in"s).has_value() && g.connect(tmp, "phase"s, ph, "in"s).has_value());
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) { std::cerr << "plugin graph: " << r.error().message << "\n"; ++g_errors; return; }
    store("plugin_mag", static_cast<testing::VectorSink<float>*>(mag.raw())->_samples);
    store("plugin_phase", static_cast<testing::VectorSink<float>*>(ph.raw())->_samples);
}

static int device_main(int argc, char** argv) {
    if (argc < 4) { std::cerr << "usage: test_host_converter --device <dir> <plugin.so>\n"; return 2; }
    g_dir    = argv[2];
    g_domain = "gpu:hip:0";
    g_prefix = "dev_";
    every_kind_as_a_graph();
    if (g_errors) return 3; // no device: fail loudly, never a host fallback
    std::string desc;
    const auto  dev  = ingest("gpu:hip:0", &desc);
    const auto  host = ingest("host", nullptr);
    std::printf("ingest run: %s\n", desc.c_str());
    EXPECT(desc == "convert_InterleavedToComplex_i16_c32[post: mul,rot] -> fir_c32");
    EXPECT(dev.size() == host.size() && !dev.empty());
    double rms = 0.0, worst = 0.0;
    for (const auto& v : host) rms += std::norm(v);
    rms = std::sqrt(rms / double(std::max<std::size_t>(1, host.size())));
    for (std::size_t i = 0; i < std::min(dev.size(), host.size()); ++i) worst = std::max(worst, double(std::abs(dev[i] - host[i])) / std::max(double(std::abs(host[i])), rms));
    std::printf("ingest graph: %zu samples, device front end vs host front end rel %.3e\n", dev.size(), worst);
    EXPECT(worst <= 1e-5);
    const auto nd = narrowing("gpu:hip:0"), nh = narrowing("host");
    const bool same = nd.size() == nh.size() && !nd.empty() && std::memcmp(nd.data(), nh.data(), nd.size() * sizeof(std::int16_t)) == 0;
    std::printf("narrowing graph: %zu samples, device Convert<float, int16> == host Convert: %s\n", nd.size(), same ? "bit for bit" : "FAILED");
    EXPECT(same);
    EXPECT(std::count(nd.begin(), nd.end(), std::int16_t(32767)) > 0 && std::count_if(nd.begin(), nd.end(), [](std::int16_t v) { return v > 0 && v < 32767; }) > 100);
    open_output_and_new_scale();
    plugin_checks(argv[3]);
    if (g_errors) { std::printf("FAILED: %d graphs did not run\n", g_errors); return 3; }
    if (!g_failures) std::printf("all converter device checks passed\n");
    return g_failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--device") return device_main(argc, argv);
    if (argc < 2) { std::cerr << "usage: test_host_converter <dir> [scale]\n"; return 2; }
    g_dir = argv[1];
    if (argc > 2) g_scale = std::stod(argv[2]);
    arithmetic_from<std::uint8_t>(); arithmetic_from<std::uint16_t>(); arithmetic_from<std::uint32_t>(); arithmetic_from<std::uint64_t>();
    arithmetic_from<std::int8_t>(); arithmetic_from<std::int16_t>(); arithmetic_from<std::int32_t>(); arithmetic_from<std::int64_t>();
    arithmetic_from<float>(); arithmetic_from<double>();
    float_kinds<float>();
    float_kinds<double>();
    every_kind_as_a_graph();
    std::printf("%d converter blocks, %d graphs, %d failed\n", g_blocks, g_graphs, g_errors);
    return g_errors ? 1 : 0;
}
