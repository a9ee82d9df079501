// SvdDenoiser through the plugin entry (Plugin.hpp:82-85), like test_host_schmitt_trigger: this program links neither the plugin nor libgr4hip.so.
//   test_host_svd_denoiser <libgr4hip_blocks.so> <compute_domain> [dir]
// Always: the four registered names (SvdDenoiser.hpp:12) instantiate with the reference's members and defaults (:34-53), an update that names a setting marks the
// block for setParameters (:76-86), and what gr4hip_svddenoise_check refuses is refused by the block.  With dir (holding x.f32): graphs
// source -> SvdDenoiser<float32> -> sink on compute_domain with window_size 64, max_rank 3, energy_fraction 0.95,
//   whole    the stream in as few chunks as the scheduler likes
//   small    the denoiser's input limited to 50 samples a call (not a multiple of the hop of 16)
// whose samples go to dir/<graph>.f32 (the Python side compares them with the oracle and with each other).  Exit code 3: a graph failed (a device domain without
// a device, or the host domain, fails loudly: the block is device-only).
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

static int run_graph(PluginLoader& loader, const std::string& domain, const std::string& dir, const std::string& tag, std::size_t max_samples) {
    using B = filter::SvdDenoiser<float>;
    Graph        g;
    property_map settings{{"window_size", std::int64_t(64)}, {"max_rank", std::int64_t(3)}, {"energy_fraction", 0.95f}, {"compute_domain", domain}};
    auto& den = g.addBlock(loader.instantiate("gr::filter::SvdDenoiser<float32>", settings));
    auto& src = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>"));
    auto& snk = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
    static_cast<testing::VectorSource<float>*>(src.raw())->values = read_f32(dir + "/x.f32");
    auto* blk = static_cast<B*>(den.raw());
    if (max_samples) blk->in.max_samples = max_samples;
    EXPECT(blk->window_size.value == 64u && blk->max_rank.value == 3u && blk->energy_fraction.value == 0.95f && blk->_parameters_changed);
    EXPECT(g.connect(src, "out"s, den, "in"s).has_value());
    EXPECT(g.connect(den, "out"s, snk, "in"s).has_value());
    EXPECT(den.compute_domain().is_device() == (domain != "host"));
    auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
    if (!sched) return 1;
    sched->exchange(std::move(g));
    if (const auto r = sched->runAndWait(); !r) {
        std::fprintf(stderr, "%s graph: %s\n", tag.c_str(), r.error().message.c_str());
        return 3;
    }
    auto*         sink = static_cast<testing::VectorSink<float>*>(snk.raw());
    std::ofstream o(dir + "/" + tag + ".f32", std::ios::binary);
    o.write(reinterpret_cast<const char*>(sink->_samples.data()), static_cast<std::streamsize>(sink->_samples.size() * 4));
    std::printf("%s: %zu samples, %zu device calls\n", tag.c_str(), sink->_samples.size(), blk->_device_calls);
    return 0;
}

// max_rank by a settings tag at sample `at`: gr4hip_svddenoise_set_params, which resets.  From the tag on the output is therefore that of a second graph that
// starts at that sample with the new rank, bit for bit (the handle's outputs do not depend on how the stream is cut).  by_tag false: that second graph.
static int tail_from(PluginLoader& loader, const std::string& domain, const std::string& dir, std::size_t at, bool by_tag, std::vector<float>& tail, std::size_t& n_by_tag) {
    Graph g;
    auto& den = g.addBlock(loader.instantiate("gr::filter::SvdDenoiser<float32>", {{"window_size", std::int64_t(64)}, {"max_rank", std::int64_t(by_tag ? 3 : 1)}, {"energy_fraction", 0.95f}, {"compute_domain", domain}}));
    auto& src = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>"));
    auto& snk = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
    auto* vs  = static_cast<testing::VectorSource<float>*>(src.raw());
    vs->values = read_f32(dir + "/x.f32");
    if (by_tag) vs->_tags.push_back(Tag{at, property_map{{"max_rank", std::int64_t(1)}}});
    else vs->values.erase(vs->values.begin(), vs->values.begin() + static_cast<std::ptrdiff_t>(at));
    EXPECT(g.connect(src, "out"s, den, "in"s).has_value() && g.connect(den, "out"s, snk, "in"s).has_value());
    auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
    if (!sched) return 1;
    sched->exchange(std::move(g));
    if (const auto r = sched->runAndWait(); !r) {
        std::fprintf(stderr, "rank graph: %s\n", r.error().message.c_str());
        return 3;
    }
    n_by_tag      = static_cast<filter::SvdDenoiser<float>*>(den.raw())->_settings_by_tag;
    const auto& y = static_cast<testing::VectorSink<float>*>(snk.raw())->_samples;
    tail.assign(y.begin() + static_cast<std::ptrdiff_t>(by_tag ? std::min(at, y.size()) : 0), y.end());
    return 0;
}
static int new_rank_case(PluginLoader& loader, const std::string& domain, const std::string& dir) {
    const std::size_t  at = read_f32(dir + "/x.f32").size() / 2;
    std::vector<float> changed, fresh;
    std::size_t        n1 = 0, n2 = 0;
    if (int rc = tail_from(loader, domain, dir, at, true, changed, n1)) return rc;
    if (int rc = tail_from(loader, domain, dir, at, false, fresh, n2)) return rc;
    const bool same = !fresh.empty() && changed.size() == fresh.size() && std::memcmp(changed.data(), fresh.data(), fresh.size() * sizeof(float)) == 0;
    EXPECT(n1 == 1 && n2 == 0 && same);
    std::printf("max_rank by settings in mid-stream: %zu samples behind the tag, those of a denoiser started there: %s\n", changed.size(), same ? "bit for bit" : "NO");
    return 0;
}

template <typename T>
static void check_members(PluginLoader& loader, const std::string& suffix, const std::string& domain) {
    using B     = filter::SvdDenoiser<T>;
    using RealT = typename B::RealT;
    const std::string n = "gr::filter::SvdDenoiser<" + suffix + ">";
    EXPECT(loader.isBlockAvailable(n));
    EXPECT(loader.instantiate(n, {{"compute_domain", domain}}) != nullptr);
    auto  b   = loader.instantiate(n, {{"window_size", std::int64_t(32)}, {"hankel_rows", std::int64_t(8)}, {"hop_fraction", 0.5f}});
    auto* blk = b ? static_cast<B*>(b->raw()) : nullptr;
    EXPECT(blk && blk->window_size.value == 32u && blk->hankel_rows.value == 8u && blk->hop_fraction.value == RealT(0.5) && blk->_parameters_changed);
    B d; // (:37-51)
    EXPECT(d.window_size.value == 64u && d.hankel_rows.value == 0u && d.max_rank.value == std::numeric_limits<gr::Size_t>::max());
    EXPECT(d.relative_threshold.value == std::numeric_limits<RealT>::epsilon() && d.absolute_threshold.value == std::numeric_limits<RealT>::epsilon());
    EXPECT(d.energy_fraction.value == RealT(1) && d.hop_fraction.value == RealT(0.25) && !d._parameters_changed);
    EXPECT((std::is_same_v<RealT, float>) == (suffix == "float32" || suffix == "complex<float32>"));
    constexpr auto                         names = B::gr_member_names();
    const std::array<std::string_view, 9> want{"in", "out", "window_size", "hankel_rows", "max_rank", "relative_threshold", "absolute_threshold", "energy_fraction", "hop_fraction"}; // (:53)
    EXPECT(names.size() == want.size());
    for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
    const auto p = d.params();
    EXPECT(p.window_size == 64u && p.hankel_rows == 0u && p.max_rank == std::numeric_limits<gr::Size_t>::max() && p.hop_fraction == 0.25 && p.energy_fraction == 1.0);
    EXPECT(p.relative_threshold == static_cast<double>(std::numeric_limits<RealT>::epsilon()));
    d.applySettings({{"max_rank", std::int64_t(3)}}); // (:76-86)
    EXPECT(d._parameters_changed && d.max_rank.value == 3u);
    EXPECT(throws([&] { d.applySettings({{"hop_fraction", 1.5f}}); }));
    EXPECT(throws([&] { d.applySettings({{"hop_fraction", 0.25f}, {"relative_threshold", -1.f}}); }));
    EXPECT(throws([&] { d.applySettings({{"relative_threshold", 0.f}, {"hankel_rows", std::int64_t(65)}}); }));
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s plugin.so compute_domain [dir]\n", argv[0]); return 2; }
    const std::string domain = argv[2];
    PluginLoader      loader;
    const auto        ok = loader.load(argv[1]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    check_members<float>(loader, "float32", domain);
    check_members<double>(loader, "float64", domain);
    check_members<std::complex<float>>(loader, "complex<float32>", domain);
    check_members<std::complex<double>>(loader, "complex<float64>", domain);
    if (argc >= 4) {
        const std::string dir = argv[3];
        if (int rc = run_graph(loader, domain, dir, "whole", 0)) return rc;
        if (int rc = run_graph(loader, domain, dir, "small", 50)) return rc;
        if (int rc = new_rank_case(loader, domain, dir)) return rc;
    }
    if (failures) std::printf("host-svd-denoiser: %d FAILURES\n", failures);
    else std::printf("host-svd-denoiser: all checks passed (compute_domain %s)\n", domain.c_str());
    return failures ? 1 : 0;
}
