// SchmittTrigger through the plugin entry (Plugin.hpp:82-85), like test_host_power_metrics: this program links neither the plugin nor libgr4hip.so.
//   test_host_schmitt_trigger <libgr4hip_blocks.so> <compute_domain> [dir]
// Always: the twelve registered names (basic/Trigger.hpp:11-13, four sample types) instantiate with the reference's members and defaults (:47-62),
// SchmittTriggerPolynomial (:14) is not registered, sample_rate / trigger_time by settings move _period / _now (:68-74), offset / threshold mark the detector
// for a reset (:76-80) and a negative threshold is refused.  With dir (holding x.f32): graphs source -> trigger<float32> -> tag-recording sink on compute_domain,
// at sample_rate 1000 with trigger_time 1000000 and a tag {gr:marker} on the source at sample 300,
//   no, basic, linear   the three methods, the stream in as few chunks as the edges allow
//   small               LINEAR_INTERPOLATION with the trigger's input limited to 50 samples a call
//   nofall              LINEAR_INTERPOLATION with an empty trigger_name_falling_edge
//   nofwd               LINEAR_INTERPOLATION with forward_tag off: the source's tag is not passed on
//   cut                 LINEAR_INTERPOLATION with the input limited to 2 samples a call: every interpolated edge position (a few samples in front of the
//                       detecting sample) lies in front of its call, where the stream is published already, so the edge is dropped and counted
// whose samples go to dir/<graph>.f32 and tags to dir/<graph>.tags, one line per tag: index, then key=value pairs (the Python side compares them with the
// oracle).  Exit code 3: a graph failed (a device domain without a device, or the host domain, fails loudly: the block is device-only).
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

static std::string show(const pmt& v) {
    return std::visit(
        [](const auto& x) -> std::string {
            using X = std::decay_t<decltype(x)>;
            char buf[64];
            if constexpr (std::is_same_v<X, std::string>) return x;
            else if constexpr (std::is_same_v<X, float>) { std::snprintf(buf, sizeof buf, "%.9g", static_cast<double>(x)); return buf; }
            else if constexpr (std::is_same_v<X, double>) { std::snprintf(buf, sizeof buf, "%.17g", x); return buf; }
            else if constexpr (std::is_same_v<X, std::uint64_t>) return std::to_string(x);
            else if constexpr (std::is_same_v<X, std::int64_t>) return std::to_string(x);
            else if constexpr (std::is_same_v<X, bool>) return x ? "true" : "false";
            else return "?";
        },
        static_cast<const pmt_base&>(v));
}

template <typename B>
static int run_graph(PluginLoader& loader, const std::string& type, const std::string& domain, const std::string& dir, const std::string& tag, std::size_t max_samples,
                     bool falling, bool forward = true) {
    Graph g;
    property_map settings{{"offset", 0.1f}, {"threshold", 0.3f}, {"sample_rate", 1000.f}, {"trigger_time", std::uint64_t(1000000)}, {"context", "ctx"s}, {"compute_domain", domain}};
    if (!falling) settings.insert_or_assign("trigger_name_falling_edge", ""s);
    if (!forward) settings.insert_or_assign("forward_tag", false);
    auto& trg = g.addBlock(loader.instantiate(type, settings));
    auto& src = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>"));
    auto& snk = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
    auto* vs  = static_cast<testing::VectorSource<float>*>(src.raw());
    vs->values = read_f32(dir + "/x.f32");
    vs->_tags.push_back(Tag{300, property_map{{"gr:marker", std::int64_t(7)}}});
    auto* blk = static_cast<B*>(trg.raw());
    if (max_samples) blk->in.max_samples = max_samples;
    EXPECT(blk->_period == 1000u && blk->_now == 1000000u);
    EXPECT(g.connect(src, "out"s, trg, "in"s).has_value());
    EXPECT(g.connect(trg, "out"s, snk, "in"s).has_value());
    EXPECT(trg.compute_domain().is_device() == (domain != "host"));
    auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
    if (!sched) return 1;
    sched->exchange(std::move(g));
    if (const auto r = sched->runAndWait(); !r) {
        std::fprintf(stderr, "%s graph: %s\n", tag.c_str(), r.error().message.c_str());
        return 3;
    }
    auto* sink = static_cast<testing::VectorSink<float>*>(snk.raw());
    {
        std::ofstream o(dir + "/" + tag + ".f32", std::ios::binary);
        o.write(reinterpret_cast<const char*>(sink->_samples.data()), static_cast<std::streamsize>(sink->_samples.size() * 4));
    }
    std::ofstream o(dir + "/" + tag + ".tags");
    for (const Tag& t : sink->_tags) {
        o << t.index;
        for (const auto& [k, v] : t.map) o << '\t' << k << '=' << show(v);
        o << '\n';
    }
    std::printf("%s: %zu samples, %zu tags, %zu device calls, %zu dropped edges, now %llu\n", tag.c_str(), sink->_samples.size(), sink->_tags.size(), blk->_device_calls,
                blk->_dropped_edges, static_cast<unsigned long long>(blk->_now));
    return 0;
}

// threshold by a settings tag at sample `at`: gr4hip_schmitt_set_params, which resets the detector.  From the tag on the edges are therefore those of a second
// graph that starts at that sample with the new threshold: same names, same positions (moved by `at`), same trigger_offset.  `from` > 0: the stream from there on,
// the new threshold from the start.  Returns (position in the whole stream, name, offset) of every edge at or behind `at`.
using FoundEdge = std::tuple<std::size_t, std::string, float>;
static int edges_behind(PluginLoader& loader, const std::string& domain, const std::string& dir, std::size_t at, bool by_tag, std::vector<FoundEdge>& edges, std::size_t& n_by_tag) {
    using B = blocks::basic::SchmittTriggerLinear<float>;
    Graph g;
    auto& trg = g.addBlock(loader.instantiate("gr::blocks::basic::SchmittTrigger<float32>", {{"offset", 0.1f}, {"threshold", by_tag ? 0.3f : 0.15f}, {"sample_rate", 1000.f}, {"compute_domain", domain}}));
    auto& src = g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>"));
    auto& snk = g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>"));
    auto* vs  = static_cast<testing::VectorSource<float>*>(src.raw());
    vs->values = read_f32(dir + "/x.f32");
    if (by_tag) vs->_tags.push_back(Tag{at, property_map{{"threshold", 0.15f}}});
    else vs->values.erase(vs->values.begin(), vs->values.begin() + static_cast<std::ptrdiff_t>(at));
    EXPECT(g.connect(src, "out"s, trg, "in"s).has_value() && g.connect(trg, "out"s, snk, "in"s).has_value());
    auto sched = loader.instantiateScheduler("gr::scheduler::Simple");
    if (!sched) return 1;
    sched->exchange(std::move(g));
    if (const auto r = sched->runAndWait(); !r) {
        std::fprintf(stderr, "threshold graph: %s\n", r.error().message.c_str());
        return 3;
    }
    n_by_tag = static_cast<B*>(trg.raw())->_settings_by_tag;
    for (const Tag& t : static_cast<testing::VectorSink<float>*>(snk.raw())->_tags) {
        const auto name = t.map.find(tag::wireKey(tag::TRIGGER_NAME));
        const auto off  = t.map.find(tag::wireKey(tag::TRIGGER_OFFSET));
        if (name == t.map.end() || off == t.map.end()) continue;
        const std::size_t pos = by_tag ? t.index : t.index + at;
        if (pos >= at) edges.emplace_back(pos, std::get<std::string>(static_cast<const pmt_base&>(name->second)), std::get<float>(static_cast<const pmt_base&>(off->second)));
    }
    return 0;
}
static int new_threshold_case(PluginLoader& loader, const std::string& domain, const std::string& dir) {
    const std::size_t at = read_f32(dir + "/x.f32").size() / 2;
    std::vector<FoundEdge> changed, fresh;
    std::size_t       n1 = 0, n2 = 0;
    if (int rc = edges_behind(loader, domain, dir, at, true, changed, n1)) return rc;
    if (int rc = edges_behind(loader, domain, dir, at, false, fresh, n2)) return rc;
    EXPECT(n1 == 1 && n2 == 0 && !fresh.empty() && changed == fresh);
    std::printf("threshold by settings in mid-stream: %zu edges behind the tag, those of a detector started there: %s\n", changed.size(), changed == fresh ? "yes" : "NO");
    return 0;
}

template <typename T>
static void check_members(PluginLoader& loader, const std::string& suffix, const std::string& domain) {
    using namespace blocks::basic;
    for (const char* base : {"gr::blocks::basic::SchmittTriggerNoInterpolation", "gr::blocks::basic::SchmittTriggerBasic", "gr::blocks::basic::SchmittTrigger"}) {
        const std::string n = std::string(base) + "<" + suffix + ">";
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"compute_domain", domain}}) != nullptr);
    }
    EXPECT(!loader.isBlockAvailable("gr::blocks::basic::SchmittTriggerPolynomial<" + suffix + ">")); // (:14) no device implementation: not offered
    auto  b   = loader.instantiate("gr::blocks::basic::SchmittTrigger<" + suffix + ">", {{"offset", std::int64_t(5)}, {"threshold", std::int64_t(2)}, {"sample_rate", 1000.f}});
    auto* blk = b ? static_cast<SchmittTriggerLinear<T>*>(b->raw()) : nullptr;
    EXPECT(blk && blk->offset.value == T(5) && blk->threshold.value == T(2) && blk->_period == 1000u && blk->_detector_changed);
    SchmittTriggerLinear<T> d;
    EXPECT(d.offset.value == T(0) && d.threshold.value == T(1) && d.trigger_name_rising_edge.value == "RISING" && d.trigger_name_falling_edge.value == "FALLING");
    EXPECT(d.sample_rate.value == 1.f && d.forward_tag.value && d.trigger_name.value.empty() && d.trigger_time.value == 0u && d.trigger_offset.value == 0.f && d.context.empty());
    EXPECT(d._period == 1u && d._now == 0u && SchmittTriggerLinear<T>::N_HISTORY == 32u);
    constexpr auto names = SchmittTriggerLinear<T>::gr_member_names();
    const std::array<std::string_view, 12> want{"in", "out", "offset", "threshold", "trigger_name_rising_edge", "trigger_name_falling_edge", "sample_rate", "forward_tag",
                                                "trigger_name", "trigger_time", "trigger_offset", "context"}; // (:62)
    EXPECT(names.size() == want.size());
    for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
    d.applySettings({{"trigger_offset", 0.5f}, {"trigger_time", std::uint64_t(123)}}); // (:72-74)
    EXPECT(d._now == 123u + 500000u && !d._detector_changed);
    d.applySettings({{"sample_rate", 4.f}}); // (:69-71)
    EXPECT(d._period == 250000u && !d._detector_changed);
    d.applySettings({{"threshold", std::int64_t(3)}}); // (:76-80)
    EXPECT(d._detector_changed && d.threshold.value == T(3));
    EXPECT(throws([&] { d.applySettings({{"threshold", std::int64_t(-1)}}); }));
    if constexpr (std::is_same_v<T, std::int16_t>) EXPECT(throws([&] { d.applySettings({{"offset", std::int64_t(32767)}}); })); // offset + threshold leaves int16
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s plugin.so compute_domain [dir]\n", argv[0]); return 2; }
    const std::string domain = argv[2];
    PluginLoader loader;
    const auto ok = loader.load(argv[1]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    check_members<std::int16_t>(loader, "int16", domain);
    check_members<std::int32_t>(loader, "int32", domain);
    check_members<float>(loader, "float32", domain);
    check_members<double>(loader, "float64", domain);
    if (argc >= 4) {
        const std::string dir = argv[3];
        using namespace blocks::basic;
        if (int rc = run_graph<SchmittTriggerNoInterpolation<float>>(loader, "gr::blocks::basic::SchmittTriggerNoInterpolation<float32>", domain, dir, "no", 0, true)) return rc;
        if (int rc = run_graph<SchmittTriggerBasic<float>>(loader, "gr::blocks::basic::SchmittTriggerBasic<float32>", domain, dir, "basic", 0, true)) return rc;
        if (int rc = run_graph<SchmittTriggerLinear<float>>(loader, "gr::blocks::basic::SchmittTrigger<float32>", domain, dir, "linear", 0, true)) return rc;
        if (int rc = run_graph<SchmittTriggerLinear<float>>(loader, "gr::blocks::basic::SchmittTrigger<float32>", domain, dir, "small", 50, true)) return rc;
        if (int rc = run_graph<SchmittTriggerLinear<float>>(loader, "gr::blocks::basic::SchmittTrigger<float32>", domain, dir, "nofall", 0, false)) return rc;
        if (int rc = run_graph<SchmittTriggerLinear<float>>(loader, "gr::blocks::basic::SchmittTrigger<float32>", domain, dir, "nofwd", 0, true, false)) return rc;
        if (int rc = run_graph<SchmittTriggerLinear<float>>(loader, "gr::blocks::basic::SchmittTrigger<float32>", domain, dir, "cut", 2, true)) return rc;
        if (int rc = new_threshold_case(loader, domain, dir)) return rc;
    }
    if (failures) std::printf("host-schmitt-trigger: %d FAILURES\n", failures);
    else std::printf("host-schmitt-trigger: all checks passed (compute_domain %s)\n", domain.c_str());
    return failures ? 1 : 0;
}
