// SignalGenerator on the device, in graphs.
//   test_host_signal_generator [n_samples]
// Always (no device needed): gr4hip_siggen_check through the blocks' params(), the refusal of a bad setting by hip::SignalSource, the member names.
// Then, on compute_domain gpu:hip:0:
//   1. gr::basic::SignalGenerator<T> -> sink with compute_domain gpu:hip:0 against the same graph in the host domain, bit for bit (UniformNoise float,
//      TriangularNoise int16, Saw complex<float>: the types whose arithmetic has no library function in it);
//   2. hip::SignalSource<complex<float>> -> OnDevice<fir_filter> -> D2H -> sink against host SignalGenerator -> H2D -> OnDevice<fir_filter> -> D2H -> sink.
// Exit code 0: all passed; 1: a comparison failed; 3: a device block reported work::Status::ERROR (what must happen without a GPU: never a host fallback).
#include <cstdio>
#include <cstring>
#include <iostream>

#include <gr4/hip.hpp>

using namespace gr;
using namespace std::string_literals;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

template <typename T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

template <typename T>
static std::vector<T> run_generator(const std::string& type, const std::string& domain, std::size_t n, int& errors, std::size_t* device_calls = nullptr) {
    Graph g;
    auto& src  = g.emplaceBlock<basic::SignalGenerator<T>>({{"signal_type", type}, {"frequency", 37.5}, {"sample_rate", 1000.0}, {"phase", 0.3}, {"amplitude", 1.5}, {"offset", 0.25},
                                                            {"seed", std::int64_t(12345)}, {"n_samples_max", std::int64_t(n)}, {"compute_domain", domain}});
    src._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<T>>();
    if (!g.connect<"out", "in">(src, sink)) { ++errors; return {}; }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) { std::cerr << "generator graph (" << domain << "): " << r.error().message << "\n"; ++errors; }
    if (device_calls) *device_calls = src._device_calls;
    return sink._samples;
}

// the source driven by hand: n samples, new amplitude and seed through applySettings (the handle's configure), n samples, reset() (the handle's reset), n samples
template <typename T>
static std::vector<T> run_generator_in_parts(const std::string& domain, std::size_t n, int& errors, std::size_t* device_calls = nullptr) {
    Graph g;
    auto& src  = g.emplaceBlock<basic::SignalGenerator<T>>({{"signal_type", "UniformNoise"s}, {"sample_rate", 1000.0}, {"amplitude", 1.5}, {"offset", 0.25}, {"seed", std::int64_t(12345)},
                                                            {"n_samples_max", std::int64_t(3 * n)}, {"compute_domain", domain}});
    src._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<T>>();
    if (!g.connect<"out", "in">(src, sink)) { ++errors; return {}; }
    const auto part = [&] {
        if (const auto r = src.work(n); r.status != work::Status::OK || r.performed_work != n) ++errors;
        sink.work(std::numeric_limits<std::size_t>::max());
    };
    part();
    src.applySettings({{"amplitude", 0.5}, {"seed", std::int64_t(99)}});
    part();
    src.reset();
    part();
    if (device_calls) *device_calls = src._device_calls;
    return sink._samples;
}

static std::vector<std::complex<float>> run_filtered(bool device_source, std::size_t n, const std::vector<double>& taps, int& errors) {
    using T = std::complex<float>;
    const property_map settings{{"signal_type", "TriangularNoise"s}, {"amplitude", 1.5}, {"offset", 0.25}, {"seed", std::int64_t(777)}, {"n_samples_max", std::int64_t(n)}};
    Graph g;
    auto& fir  = g.emplaceBlock<hip::OnDevice<filter::fir_filter<T>>>({{"b", taps}});
    auto& d2h  = g.emplaceBlock<hip::D2H<T>>();
    auto& sink = g.emplaceBlock<testing::VectorSink<T>>();
    fir._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    bool ok = true;
    if (device_source) {
        auto& src = g.emplaceBlock<hip::SignalSource<T>>(settings);
        src._log  = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
        ok        = g.connect<"out", "in">(src, fir).has_value();
    } else {
        auto& src = g.emplaceBlock<basic::SignalGenerator<T>>(settings);
        auto& h2d = g.emplaceBlock<hip::H2D<T>>();
        ok        = g.connect<"out", "in">(src, h2d).has_value() && g.connect<"out", "in">(h2d, fir).has_value();
    }
    if (!ok || !g.connect<"out", "in">(fir, d2h) || !g.connect<"out", "in">(d2h, sink)) { ++errors; return {}; }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) { std::cerr << "filtered graph: " << r.error().message << "\n"; ++errors; }
    return sink._samples;
}

int main(int argc, char** argv) {
    const std::size_t n = argc > 1 ? std::stoul(argv[1]) : 200000;
    { // host side: what the blocks hand to the library
        basic::SignalGenerator<float> f;
        auto                          p = f.params();
        EXPECT(p.dtype == GR4HIP_F32 && p.signal_type == GR4HIP_SIGGEN_SIN && p.sample_rate == 1000.f && p.frequency == 1.f && p.amplitude == 1.f && p.seed == 0u);
        EXPECT(gr4hip_siggen_check(&p) == GR4HIP_OK);
        EXPECT(basic::SignalGenerator<std::int16_t>{}.params().dtype == GR4HIP_I16 && basic::SignalGenerator<std::complex<float>>{}.params().dtype == GR4HIP_C32);
        EXPECT(basic::SignalGenerator<double>{}.params().dtype == GR4HIP_F64);
        const auto bad = basic::SignalGenerator<std::int32_t>{}.params(); // registered upstream, no device implementation
        EXPECT(gr4hip_siggen_check(&bad) != GR4HIP_OK);
        hip::SignalSource<float> s;
        bool                     threw = false;
        try { s.applySettings({{"sample_rate", 0.0}}); } catch (const std::exception&) { threw = true; }
        EXPECT(threw);
        constexpr auto names = hip::SignalSource<float>::gr_member_names();
        EXPECT(names.size() == 10u && std::string_view(names[0]) == "out" && std::string_view(names[1]) == "signal_type" && std::string_view(names[8]) == "n_samples_max");
    }
    if (failures) return 1;

    int errors = 0;
    std::size_t calls = 0;
    const auto  dev_f = run_generator<float>("UniformNoise", "gpu:hip:0", n, errors, &calls);
    if (errors) return 3; // no device: fail loudly, never a host fallback
    const auto host_f = run_generator<float>("UniformNoise", "host", n, errors);
    const bool ok_f   = dev_f.size() == n && calls > 0 && same_bits(dev_f, host_f);
    std::printf("SignalGenerator<float> UniformNoise gpu:hip:0 == host domain: %s (%zu samples, %zu device calls)\n", ok_f ? "bit for bit" : "FAILED", dev_f.size(), calls);
    if (!ok_f) ++failures;
    const bool ok_i = same_bits(run_generator<std::int16_t>("TriangularNoise", "gpu:hip:0", n, errors), run_generator<std::int16_t>("TriangularNoise", "host", n, errors));
    std::printf("SignalGenerator<int16> TriangularNoise gpu:hip:0 == host domain: %s\n", ok_i ? "bit for bit" : "FAILED");
    if (!ok_i) ++failures;
    const bool ok_c = same_bits(run_generator<std::complex<float>>("Saw", "gpu:hip:0", n, errors), run_generator<std::complex<float>>("Saw", "host", n, errors));
    std::printf("SignalGenerator<complex<float>> Saw gpu:hip:0 == host domain: %s\n", ok_c ? "bit for bit" : "FAILED");
    if (!ok_c) ++failures;

    {
        const std::size_t m = 4096;
        std::size_t       part_calls = 0;
        const auto        dev_p  = run_generator_in_parts<float>("gpu:hip:0", m, errors, &part_calls);
        const auto        host_p = run_generator_in_parts<float>("host", m, errors);
        const bool        differ = host_p.size() == 3 * m && !std::equal(host_p.begin(), host_p.begin() + static_cast<std::ptrdiff_t>(m), host_p.begin() + static_cast<std::ptrdiff_t>(m));
        const bool        ok_p   = dev_p.size() == 3 * m && part_calls == 3 && differ && same_bits(dev_p, host_p);
        std::printf("SignalGenerator<float> new settings, then reset, between chunks, gpu:hip:0 == host domain: %s (%zu samples, %zu device calls)\n", ok_p ? "bit for bit" : "FAILED", dev_p.size(), part_calls);
        if (!ok_p) ++failures;
    }
    std::vector<double> taps(31); // (float32 products in a fixed order per output: the same bits however the two graphs cut the stream into chunks)
    for (std::size_t k = 0; k < taps.size(); ++k) taps[k] = (0.54 - 0.46 * std::cos(2.0 * 3.14159265358979323846 * double(k) / 30.0)) / 16.0;
    const auto from_device = run_filtered(true, n, taps, errors);
    const auto from_host   = run_filtered(false, n, taps, errors);
    const bool ok_g        = from_device.size() == n && same_bits(from_device, from_host);
    std::printf("hip::SignalSource<complex<float>> -> OnDevice<fir_filter> -> D2H == host SignalGenerator -> H2D -> OnDevice<fir_filter> -> D2H: %s (%zu samples)\n",
                ok_g ? "bit for bit" : "FAILED", from_device.size());
    if (!ok_g) ++failures;
    if (errors) { std::printf("FAILED: %d graphs did not run\n", errors); return 3; }
    if (!failures) std::printf("all signal generator graph checks passed\n");
    return failures ? 1 : 0;
}
