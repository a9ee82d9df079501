// FrequencyEstimator blocks through the plugin entry (Plugin.hpp:82-85), like test_host_plugin: this program links neither the plugin nor libgr4hip.so.
//   test_host_freq_est <libgr4hip_blocks.so> <compute_domain> [signal.f32 out_prefix]
// Always: the four registered names (FrequencyEstimator.hpp:25-26, 181-182; float only) instantiate, and ill-formed settings are refused.
// With a signal: source -> fir_filter<float32> {0.5, 0.5} -> FrequencyEstimatorFrequencyDomainDecimating<float32> (min_fft_size 4096) -> sink and
// source -> FrequencyEstimatorTimeDomain<float32> -> sink run on compute_domain; the outputs go to <out_prefix>_fd.f32 / _td.f32 (the Python side compares
// them with the oracle).  Exit code 3: the graph failed (a device domain without a device fails loudly, never a host fallback).
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/blocks.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s plugin.so compute_domain [signal.f32 out_prefix]\n", argv[0]); return 2; }
    const std::string domain = argv[2];
    PluginLoader loader;
    const auto ok = loader.load(argv[1]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    for (const char* n : {"gr::filter::FrequencyEstimatorTimeDomain<float32>", "gr::filter::FrequencyEstimatorTimeDomainDecimating<float32>",
                          "gr::filter::FrequencyEstimatorFrequencyDomain<float32>", "gr::filter::FrequencyEstimatorFrequencyDomainDecimating<float32>"}) {
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"compute_domain", domain}}) != nullptr);
    }
    EXPECT(!loader.isBlockAvailable("gr::filter::FrequencyEstimatorTimeDomain<float64>"));
    bool threw = false;
    try { (void)loader.instantiate("gr::filter::FrequencyEstimatorTimeDomain<float32>", {{"f_max", 600.f}}); } catch (const std::exception&) { threw = true; }
    EXPECT(threw); // settingsChanged: f_max >= sample_rate / 2
    {
        auto fd = loader.instantiate("gr::filter::FrequencyEstimatorFrequencyDomainDecimating<float32>", {{"min_fft_size", std::int64_t(4096)}, {"f_min", 45.f}, {"f_max", 55.f}});
        EXPECT(fd != nullptr && static_cast<filter::FrequencyEstimatorFrequencyDomainDecimating<float>*>(fd->raw())->input_chunk_size == 4096u); // initialiseFFT: chunk = N
        auto td = loader.instantiate("gr::filter::FrequencyEstimatorTimeDomainDecimating<float32>");
        EXPECT(td != nullptr && static_cast<filter::FrequencyEstimatorTimeDomainDecimating<float>*>(td->raw())->input_chunk_size == 10u);
    }
    if (argc >= 5) {
        std::ifstream     f(argv[3], std::ios::binary);
        std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        std::vector<float> x(raw.size() / 4);
        std::memcpy(x.data(), raw.data(), x.size() * 4);
        Graph g;
        const auto n = static_cast<std::int64_t>(x.size());
        auto& src  = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>", {{"n_samples_max", n}}));
        auto& fir  = g.addBlock(loader.instantiate("gr::filter::fir_filter<float32>", {{"b", std::vector<double>{0.5, 0.5}}, {"compute_domain", domain}}));
        auto& fd   = g.addBlock(loader.instantiate("gr::filter::FrequencyEstimatorFrequencyDomainDecimating<float32>",
                                                   {{"min_fft_size", std::int64_t(4096)}, {"f_min", 45.f}, {"f_max", 55.f}, {"compute_domain", domain}}));
        auto& fsnk = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
        auto& src2 = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>", {{"n_samples_max", n}}));
        auto& td   = g.addBlock(loader.instantiate("gr::filter::FrequencyEstimatorTimeDomain<float32>", {{"f_min", 45.f}, {"f_max", 55.f}, {"n_periods", std::int64_t(3)}, {"compute_domain", domain}}));
        auto& tsnk = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
        static_cast<testing::VectorSource<float>*>(src.raw())->values  = x;
        static_cast<testing::VectorSource<float>*>(src2.raw())->values = x;
        EXPECT(g.connect(src, "out"s, fir, "in"s).has_value() && g.connect(fir, "out"s, fd, "in"s).has_value() && g.connect(fd, "out"s, fsnk, "in"s).has_value());
        EXPECT(g.connect(src2, "out"s, td, "in"s).has_value() && g.connect(td, "out"s, tsnk, "in"s).has_value());
        EXPECT(fd.compute_domain().is_device() == (domain != "host"));
        auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
        if (!sched) return 1;
        sched->exchange(std::move(g));
        if (const auto r = sched->runAndWait(); !r) {
            std::fprintf(stderr, "estimator graph: %s\n", r.error().message.c_str());
            return 3;
        }
        for (const auto& [snk, suffix] : {std::pair{&fsnk, "_fd.f32"}, std::pair{&tsnk, "_td.f32"}}) {
            const auto&   y = static_cast<testing::VectorSink<float>*>(snk->raw())->_samples;
            std::ofstream o(std::string(argv[4]) + suffix, std::ios::binary);
            o.write(reinterpret_cast<const char*>(y.data()), static_cast<std::streamsize>(y.size() * 4));
            std::printf("%s: %zu outputs\n", suffix, y.size());
        }
    }
    if (failures) std::printf("host-freq-est: %d FAILURES\n", failures);
    else std::printf("host-freq-est: all checks passed (compute_domain %s)\n", domain.c_str());
    return failures ? 1 : 0;
}
