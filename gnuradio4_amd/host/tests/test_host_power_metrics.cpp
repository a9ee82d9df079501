// PowerMetrics through the plugin entry (Plugin.hpp:82-85), like test_host_iq_demod: this program links neither the plugin nor libgr4hip.so.
//   test_host_power_metrics <libgr4hip_blocks.so> <compute_domain> [dir]
// Always: the two registered names (PowerEstimators.hpp:18-19, float) instantiate with the reference's members, `decimate` by settings moves input_chunk_size
// (:79-81), high_pass / low_pass are not reflected (:51), decimate 0 is refused.  With dir (holding u0..u2.f32, i0..i2.f32): three graphs on compute_domain,
//   single   u0, i0 -> SinglePhasePowerMetrics<float32> -> sinks on P, S, U_rms, I_rms; Q stays unconnected
//   three    all six inputs -> ThreePhasePowerMetrics<float32> -> fifteen sinks
//   restart  u0, i0 through a block with decimate 100, and a tag {decimate: 50} on the voltage stream at half its length: settings-by-tag in the middle of
//            the stream.  The work loop hands over chunks of 50 from the tag on and the device handle rebuilds its filters (gr4hip_powermetrics_set_params):
//            behind the tag the outputs are those of a fresh block at decimate 50 on the second half
// whose outputs go to dir/<graph>_<output><phase>.f32 (the Python side compares them with the oracle).  Exit code 3: a graph failed (a device domain without a
// device, or the host domain, fails loudly: there is no host arithmetic).
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/blocks.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static std::vector<float> read_f32(const std::string& path) {
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

// a host block whose chunk follows its `decimate` setting as PowerMetrics' does; it notes how the work loop chunked each call and keeps the first sample of a chunk
struct ChunkProbe : Block<ChunkProbe, Resampling<10U, 1U, false>> {
    PortIn<float>  in;
    PortOut<float> out;
    gr::Size_t     decimate = 10U;
    std::vector<std::pair<std::size_t, std::size_t>> calls; // (input samples, decimate in force)
    GR_MAKE_REFLECTABLE(ChunkProbe, in, out, decimate);
    void         settingsChanged(const property_map&, const property_map&) { this->input_chunk_size = decimate; }
    work::Status processBulk(std::span<const float> is, std::span<float> os) {
        calls.emplace_back(is.size(), decimate);
        for (std::size_t k = 0; k < os.size(); ++k) os[k] = is[k * decimate];
        return work::Status::OK;
    }
};

static const char* kOutputs[5] = {"P", "Q", "S", "U_rms", "I_rms"};

// sources -> block -> sinks; `skip`: an output left unconnected (or null); `tag_at`, `decimate_update`: a {decimate} tag on the first voltage stream at that sample (0: none)
static int run_graph(PluginLoader& loader, const std::string& type, const std::string& domain, const std::string& dir, const std::string& tag, std::size_t phases,
                     std::size_t tag_at, const char* skip, std::int64_t decimate_update) {
    Graph g;
    auto& pm = g.addBlock(loader.instantiate(type, {{"decimate", std::int64_t(100)}, {"compute_domain", domain}}));
    for (std::size_t k = 0; k < phases; ++k) {
        for (const char* in : {"U", "I"}) {
            auto x = read_f32(dir + "/" + (in[0] == 'U' ? "u" : "i") + std::to_string(k) + ".f32");
            auto& src = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>"));
            auto* vs  = static_cast<testing::VectorSource<float>*>(src.raw());
            vs->values = std::move(x);
            if (decimate_update && k == 0 && in[0] == 'U') vs->_tags.push_back(Tag{tag_at, property_map{{"decimate", decimate_update}}});
            EXPECT(g.connect(src, "out"s, pm, std::string(in) + "#" + std::to_string(k)).has_value());
        }
    }
    std::vector<std::pair<BlockModel*, std::string>> sinks;
    for (const char* out : kOutputs) {
        if (skip && std::string(skip) == out) continue;
        for (std::size_t k = 0; k < phases; ++k) {
            auto& snk = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
            EXPECT(g.connect(pm, std::string(out) + "#" + std::to_string(k), snk, "in"s).has_value());
            sinks.emplace_back(&snk, dir + "/" + tag + "_" + out + std::to_string(k) + ".f32");
        }
    }
    EXPECT(pm.compute_domain().is_device() == (domain != "host"));
    auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
    if (!sched) return 1;
    sched->exchange(std::move(g));
    if (const auto r = sched->runAndWait(); !r) {
        std::fprintf(stderr, "%s graph: %s\n", tag.c_str(), r.error().message.c_str());
        return 3;
    }
    for (const auto& [snk, path] : sinks) {
        const auto&   y = static_cast<testing::VectorSink<float>*>(snk->raw())->_samples;
        std::ofstream o(path, std::ios::binary);
        o.write(reinterpret_cast<const char*>(y.data()), static_cast<std::streamsize>(y.size() * 4));
    }
    std::printf("%s: %zu outputs per port\n", tag.c_str(), sinks.empty() ? std::size_t(0) : static_cast<testing::VectorSink<float>*>(sinks[0].first->raw())->_samples.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s plugin.so compute_domain [dir]\n", argv[0]); return 2; }
    const std::string domain = argv[2];
    PluginLoader loader;
    const auto ok = loader.load(argv[1]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    const std::string one = "gr::electrical::SinglePhasePowerMetrics<float32>", three = "gr::electrical::ThreePhasePowerMetrics<float32>";
    for (const auto& n : {one, three}) {
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"compute_domain", domain}}) != nullptr);
    }
    {
        auto  b   = loader.instantiate(three, {{"sample_rate", 20000.f}, {"decimate", std::int64_t(50)}});
        auto* blk = b ? static_cast<electrical::ThreePhasePowerMetrics<float>*>(b->raw()) : nullptr;
        EXPECT(blk && blk->U.size() == 3u && blk->I.size() == 3u && blk->P.size() == 3u && blk->Q.size() == 3u && blk->S.size() == 3u && blk->U_rms.size() == 3u &&
               blk->I_rms.size() == 3u);
        EXPECT(blk && blk->sample_rate == 20000.f && blk->decimate == 50u && blk->input_chunk_size == 50u && blk->output_chunk_size == 1u);
        EXPECT(blk && blk->high_pass == 2.f && blk->low_pass == 90.f);
    }
    {
        electrical::SinglePhasePowerMetrics<float> blk;
        EXPECT(blk.U.size() == 1u && blk.decimate == 100u && blk.input_chunk_size == 100u);
        constexpr auto names = electrical::SinglePhasePowerMetrics<float>::gr_member_names();
        EXPECT(names.size() == 9u); // U, I, P, Q, S, U_rms, I_rms, sample_rate, decimate (:51): high_pass and low_pass are not reflected
        for (const auto& n : names) EXPECT(std::string_view(n) != "high_pass" && std::string_view(n) != "low_pass");
        EXPECT(throws([&] { blk.applySettings({{"decimate", std::int64_t(0)}}); }));
        EXPECT(blk.decimate == 100u && blk.input_chunk_size == 100u); // a refused update leaves the block as it was
        EXPECT(!throws([&] { blk.applySettings({{"decimate", std::int64_t(200)}}); }) && blk.input_chunk_size == 200u);
    }
    { // settings-by-tag that change the chunk (host work loop, no device): {decimate: 50} at sample 40 makes a chunk larger than the 20 samples that were sized
      // up to the next tag at 60.  It is one forced chunk, the tag inside it is applied with it ({decimate: 20}), and no tag is lost
        Graph g;
        auto& src = g.emplaceBlock<testing::VectorSource<float>>();
        auto& blk = g.emplaceBlock<ChunkProbe>();
        auto& snk = g.emplaceBlock<testing::VectorSink<float>>();
        src.values.resize(200);
        for (std::size_t k = 0; k < 200; ++k) src.values[k] = static_cast<float>(k);
        src._tags.push_back(Tag{40, property_map{{"decimate", std::int64_t(50)}}});
        src._tags.push_back(Tag{60, property_map{{"decimate", std::int64_t(20)}}});
        EXPECT((g.connect<"out", "in">(src, blk)) && (g.connect<"out", "in">(blk, snk)));
        scheduler::Simple sched;
        sched.exchange(std::move(g));
        EXPECT(sched.runAndWait().has_value());
        EXPECT(blk.decimate == 20u && blk.input_chunk_size == 20u && blk._settings_by_tag == 2u);
        std::size_t total = 0;
        for (const auto& [n, d] : blk.calls) {
            EXPECT(n % d == 0 && d == (total < 40 ? 10u : 20u)); // every call in whole chunks of the setting in force; decimate 50 never processed a sample
            total += n;
        }
        EXPECT(total == 200u);
        const std::vector<float> want{0.f, 10.f, 20.f, 30.f, 40.f, 60.f, 80.f, 100.f, 120.f, 140.f, 160.f, 180.f};
        EXPECT(snk._samples == want);
    }
    if (argc >= 4) {
        const std::string dir  = argv[3];
        const std::size_t half = read_f32(dir + "/u0.f32").size() / 2;
        if (int rc = run_graph(loader, one, domain, dir, "single", 1, 0, "Q", 0)) return rc;
        if (int rc = run_graph(loader, three, domain, dir, "three", 3, 0, nullptr, 0)) return rc;
        if (int rc = run_graph(loader, one, domain, dir, "restart", 1, half, nullptr, 50)) return rc;
    }
    if (failures) std::printf("host-power-metrics: %d FAILURES\n", failures);
    else std::printf("host-power-metrics: all checks passed (compute_domain %s)\n", domain.c_str());
    return failures ? 1 : 0;
}
