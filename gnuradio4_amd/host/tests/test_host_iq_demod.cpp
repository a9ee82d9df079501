// IQDemodulator through the plugin entry (Plugin.hpp:82-85), like test_host_freq_est: this program links neither the plugin nor libgr4hip.so.
//   test_host_iq_demod <libgr4hip_blocks.so> <compute_domain> [ref.f32 resp.f32 out_prefix]
// Always: the two registered names (FrequencyEstimator.hpp:385, float and double) instantiate, ill-formed settings are refused, and IQDemodulatorFixed refuses an
// update that names derivative_method (:455-459) while taking the others.  With signals: two sources -> IQDemodulator<float32> (chunk 1024) -> three sinks on
// compute_domain; the outputs go to <out_prefix>_amp.f32 / _phase.f32 / _freq.f32 (the Python side compares them with the oracle).  Exit code 3: the graph
// failed (a device domain without a device, or the host domain, fails loudly: there is no host arithmetic).  Then one chunk twice: every output connected, and
// `phase` alone (amplitude and frequency have no reader and are not copied to a port) -- the phase is the same value, bit for bit.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/blocks.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static std::vector<float> read_f32(const char* path) {
    std::ifstream      f(path, std::ios::binary);
    std::vector<char>  raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<float> x(raw.size() / 4);
    std::memcpy(x.data(), raw.data(), x.size() * 4);
    return x;
}

template <typename F>
static bool throws(F&& f) {
    try { f(); } catch (const std::exception&) { return true; }
    return false;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s plugin.so compute_domain [ref.f32 resp.f32 out_prefix]\n", argv[0]); return 2; }
    const std::string domain = argv[2];
    PluginLoader loader;
    const auto ok = loader.load(argv[1]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    const std::string f32 = "gr::filter::IQDemodulator<float32, gr::Resampling<1024U, 1U, false>>";
    const std::string f64 = "gr::filter::IQDemodulator<float64, gr::Resampling<1024U, 1U, false>>";
    for (const auto& n : {f32, f64}) {
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"compute_domain", domain}}) != nullptr);
    }
    EXPECT(throws([&] { (void)loader.instantiate(f32, {{"f_low_pass", 4e7f}}); }));   // f_lp >= fs / 2
    EXPECT(throws([&] { (void)loader.instantiate(f64, {{"f_high_pass", 2e4f}}); }));  // f_hp >= f_lp
    {
        auto b = loader.instantiate(f32, {{"derivative_method", std::int64_t(2)}, {"phase_unit", "Degrees"s}});
        auto* blk = b ? static_cast<filter::IQDemodulatorDecimating<float>*>(b->raw()) : nullptr;
        EXPECT(blk && blk->derivative_method == filter::DerivativeMethod::SavitzkyGolay7 && blk->phase_unit == filter::PhaseUnit::Degrees);
        EXPECT(blk && blk->input_chunk_size == 1024u);
    }
    {
        filter::IQDemodulatorFixed<float, filter::DerivativeMethod::SavitzkyGolay5> fixed;
        EXPECT(fixed.derivative_method == filter::DerivativeMethod::SavitzkyGolay5);
        EXPECT(throws([&] { fixed.applySettings({{"derivative_method", std::int64_t(0)}}); }));
        EXPECT(!throws([&] { fixed.applySettings({{"phase_unit", std::int64_t(1)}, {"f_low_pass", 5000.f}}); }));
        filter::IQDemodulatorDecimating<double> free;
        EXPECT(!throws([&] { free.applySettings({{"derivative_method", std::int64_t(1)}}); }));
        EXPECT(free._filters_changed);
    }
    if (argc >= 6) {
        const auto ref = read_f32(argv[3]), resp = read_f32(argv[4]);
        Graph      g;
        const auto n = static_cast<std::int64_t>(ref.size());
        auto& s1 = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>", {{"n_samples_max", n}}));
        auto& s2 = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>", {{"n_samples_max", n}}));
        auto& iq = g.addBlock(loader.instantiate(f32, {{"sample_rate", 62.5e6f}, {"derivative_method", std::int64_t(1)}, {"compute_domain", domain}}));
        auto& ka = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
        auto& kp = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
        auto& kf = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
        static_cast<testing::VectorSource<float>*>(s1.raw())->values = ref;
        static_cast<testing::VectorSource<float>*>(s2.raw())->values = resp;
        EXPECT(g.connect(s1, "out"s, iq, "ref"s).has_value() && g.connect(s2, "out"s, iq, "resp"s).has_value());
        EXPECT(g.connect(iq, "amplitude"s, ka, "in"s).has_value() && g.connect(iq, "phase"s, kp, "in"s).has_value() && g.connect(iq, "frequency"s, kf, "in"s).has_value());
        EXPECT(iq.compute_domain().is_device() == (domain != "host"));
        auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
        if (!sched) return 1;
        sched->exchange(std::move(g));
        if (const auto r = sched->runAndWait(); !r) {
            std::fprintf(stderr, "iq graph: %s\n", r.error().message.c_str());
            return 3;
        }
        for (const auto& [snk, suffix] : {std::pair{&ka, "_amp.f32"}, std::pair{&kp, "_phase.f32"}, std::pair{&kf, "_freq.f32"}}) {
            const auto&   y = static_cast<testing::VectorSink<float>*>(snk->raw())->_samples;
            std::ofstream o(std::string(argv[5]) + suffix, std::ios::binary);
            o.write(reinterpret_cast<const char*>(y.data()), static_cast<std::streamsize>(y.size() * 4));
            std::printf("%s: %zu outputs\n", suffix, y.size());
        }
    }
    if (argc >= 6) {
        const auto         ref = read_f32(argv[3]), resp = read_f32(argv[4]);
        std::vector<float> phase[2];
        for (int alone = 0; alone < 2 && ref.size() >= 1024 && resp.size() >= 1024; ++alone) {
            Graph g;
            auto& s1 = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>", {{"n_samples_max", std::int64_t(1024)}}));
            auto& s2 = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>", {{"n_samples_max", std::int64_t(1024)}}));
            auto& iq = g.addBlock(loader.instantiate(f32, {{"sample_rate", 62.5e6f}, {"derivative_method", std::int64_t(1)}, {"compute_domain", domain}}));
            auto& kp = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
            static_cast<testing::VectorSource<float>*>(s1.raw())->values.assign(ref.begin(), ref.begin() + 1024);
            static_cast<testing::VectorSource<float>*>(s2.raw())->values.assign(resp.begin(), resp.begin() + 1024);
            EXPECT(g.connect(s1, "out"s, iq, "ref"s).has_value() && g.connect(s2, "out"s, iq, "resp"s).has_value() && g.connect(iq, "phase"s, kp, "in"s).has_value());
            if (!alone) {
                auto& ka = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
                auto& kf = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
                EXPECT(g.connect(iq, "amplitude"s, ka, "in"s).has_value() && g.connect(iq, "frequency"s, kf, "in"s).has_value());
            }
            auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
            if (!sched) return 1;
            sched->exchange(std::move(g));
            if (const auto r = sched->runAndWait(); !r) {
                std::fprintf(stderr, "iq one-chunk graph: %s\n", r.error().message.c_str());
                return 3;
            }
            phase[alone] = static_cast<testing::VectorSink<float>*>(kp.raw())->_samples;
        }
        EXPECT(phase[0].size() == 1 && phase[1].size() == 1 && std::memcmp(phase[0].data(), phase[1].data(), sizeof(float)) == 0);
        // four chunks, invert_phase by a settings tag in front of the third: gr4hip_iqdemod_set_params on the live handle, which keeps its filters (no filter key is
        // named).  Against the same four chunks without the tag: the amplitude is the same bit for bit throughout, the phase up to the tag, and from the tag on it
        // is the other run's with the sign turned (the library negates the phase: an exact operation)
        std::vector<float> amp[2], ph[2];
        std::size_t        by_tag[2] = {0, 0};
        for (int inverted = 0; inverted < 2 && ref.size() >= 4096 && resp.size() >= 4096; ++inverted) {
            Graph g;
            auto& s1 = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>", {{"n_samples_max", std::int64_t(4096)}}));
            auto& s2 = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>", {{"n_samples_max", std::int64_t(4096)}}));
            auto& iq = g.addBlock(loader.instantiate(f32, {{"sample_rate", 62.5e6f}, {"derivative_method", std::int64_t(1)}, {"compute_domain", domain}}));
            auto& ka = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
            auto& kp = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
            auto& kf = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
            auto* v1 = static_cast<testing::VectorSource<float>*>(s1.raw());
            v1->values.assign(ref.begin(), ref.begin() + 4096);
            if (inverted) v1->_tags = {{2048, {{"invert_phase", true}}}};
            static_cast<testing::VectorSource<float>*>(s2.raw())->values.assign(resp.begin(), resp.begin() + 4096);
            EXPECT(g.connect(s1, "out"s, iq, "ref"s).has_value() && g.connect(s2, "out"s, iq, "resp"s).has_value());
            EXPECT(g.connect(iq, "amplitude"s, ka, "in"s).has_value() && g.connect(iq, "phase"s, kp, "in"s).has_value() && g.connect(iq, "frequency"s, kf, "in"s).has_value());
            auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
            if (!sched) return 1;
            sched->exchange(std::move(g));
            if (const auto r = sched->runAndWait(); !r) {
                std::fprintf(stderr, "iq settings graph: %s\n", r.error().message.c_str());
                return 3;
            }
            amp[inverted]    = static_cast<testing::VectorSink<float>*>(ka.raw())->_samples;
            ph[inverted]     = static_cast<testing::VectorSink<float>*>(kp.raw())->_samples;
            by_tag[inverted] = static_cast<filter::IQDemodulatorDecimating<float>*>(iq.raw())->_settings_by_tag;
        }
        EXPECT(by_tag[0] == 0 && by_tag[1] == 1 && amp[0].size() == 4 && amp[1].size() == 4 && ph[0].size() == 4 && ph[1].size() == 4);
        if (amp[0].size() == 4 && amp[1].size() == 4 && ph[0].size() == 4 && ph[1].size() == 4) {
            EXPECT(std::memcmp(amp[0].data(), amp[1].data(), 4 * sizeof(float)) == 0 && std::memcmp(ph[0].data(), ph[1].data(), 2 * sizeof(float)) == 0);
            for (std::size_t k = 2; k < 4; ++k) {
                const float turned = -ph[0][k];
                EXPECT(std::memcmp(&turned, &ph[1][k], sizeof(float)) == 0 && ph[0][k] != 0.f);
            }
        }
        std::printf("invert_phase by settings after two chunks: amplitude unchanged, phase turned from the third chunk on\n");
        std::printf("phase alone: %zu output, the all-connected graph's bit for bit\n", phase[1].size());
    }
    if (failures) std::printf("host-iq-demod: %d FAILURES\n", failures);
    else std::printf("host-iq-demod: all checks passed (compute_domain %s)\n", domain.c_str());
    return failures ? 1 : 0;
}
