// PowerFactor and SystemUnbalance (PowerEstimators.hpp:144-257) as host mirror blocks, through the plugin entry like test_host_power_metrics: this program links
// neither the plugin nor libgr4hip.so.
//   test_host_electrical <libgr4hip_blocks.so> <compute_domain> [dir [phase_ulp_f32 phase_ulp_f64]]
// Always: the eight registered names (PowerEstimators.hpp:141-142, 190-191 for float and double) instantiate with the reference's members and port names.
// With dir, for T in {f32, f64} and X_<T>.bin holding three rows of one length for X in P, S, U, I: four graphs on compute_domain,
//   pf3   ThreePhasePowerFactorCalculator<T>, every port connected         pf1   SinglePhasePowerFactorCalculator<T> on row 0, `phase` left unconnected
//   ub3   ThreePhaseSystemUnbalanceCalculator<T>, every port connected     ub2   TwoPhaseSystemUnbalanceCalculator<T> on rows 0 and 1, the total power unconnected
// and for float ub3t: ThreePhaseSystemUnbalanceCalculator<float> on the first 256 samples with the total power alone connected (both unbalance outputs unread),
// whose sink contents go to dir/<graph>_<T>_<port>.bin (rows one after the other) and are compared with dir/want_<graph>_<T>_<port>.bin where that exists: the
// phase within the given number of units in the last place (2 by default: CONVERTERS.md's host bound for the C library), everything else bit for bit with NaN
// equal to NaN.  With dir/u.f32 and dir/i.f32 (three rows each) on a device domain: PowerMetrics<float, 3> (decimate 7) -> ThreePhasePowerFactorCalculator<float>
// + ThreePhaseSystemUnbalanceCalculator<float>, once built here (dir/chain_<port>.bin) and once from a GRC text through the plugin (dir/grc_<port>.bin).
// Exit code 3: a graph failed.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/blocks.hpp>
#include <gr4/grc.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

template <typename T>
static std::vector<T> read_bin(const std::string& path) {
    std::ifstream     f(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T>    x(raw.size() / sizeof(T));
    std::memcpy(x.data(), raw.data(), x.size() * sizeof(T));
    return x;
}
template <typename T>
static void write_bin(const std::string& path, const std::vector<T>& y) {
    std::ofstream o(path, std::ios::binary);
    o.write(reinterpret_cast<const char*>(y.data()), static_cast<std::streamsize>(y.size() * sizeof(T)));
}
static bool exists(const std::string& path) { return std::ifstream(path).good(); }

template <typename T> constexpr const char* tname() { return std::is_same_v<T, float> ? "f32" : "f64"; }
template <typename T> constexpr const char* portable() { return std::is_same_v<T, float> ? "float32" : "float64"; }

// distance in units in the last place on the ordered integers (0 for two NaNs, huge for one)
template <typename T>
static double ulp_distance(T a, T b) {
    using I = std::conditional_t<std::is_same_v<T, float>, std::int32_t, std::int64_t>;
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b) ? 0.0 : 1e300;
    const auto ordered = [](T v) {
        I i;
        std::memcpy(&i, &v, sizeof(T));
        return i < 0 ? static_cast<long double>(std::numeric_limits<I>::min()) - static_cast<long double>(i) : static_cast<long double>(i);
    };
    return static_cast<double>(std::fabs(ordered(a) - ordered(b)));
}
template <typename T>
static bool same_bits(T a, T b) { return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof(T)) == 0; }

// writes the sink contents and compares them with the expected file, if there is one: ulp < 0 asks for bit equality
template <typename T>
static void deliver(const std::string& dir, const std::string& name, const std::vector<T>& got, double ulp) {
    write_bin(dir + "/" + name + ".bin", got);
    const std::string want_path = dir + "/want_" + name + ".bin";
    if (!exists(want_path)) return;
    const auto want = read_bin<T>(want_path);
    EXPECT(want.size() == got.size());
    double      worst = 0.0;
    std::size_t bad   = 0;
    for (std::size_t k = 0; k < std::min(want.size(), got.size()); ++k) {
        if (ulp < 0) bad += !same_bits(got[k], want[k]);
        else worst = std::max(worst, ulp_distance(got[k], want[k]));
    }
    if (ulp < 0) std::printf("%s: %zu of %zu values differ from the oracle\n", name.c_str(), bad, got.size());
    else std::printf("%s: %g ulp from the oracle (bound %g)\n", name.c_str(), worst, ulp);
    EXPECT(bad == 0 && worst <= std::max(ulp, 0.0));
}

template <typename T>
static std::vector<T> row(const std::vector<T>& x, std::size_t k) {
    const std::size_t n = x.size() / 3;
    return std::vector<T>(x.begin() + static_cast<std::ptrdiff_t>(k * n), x.begin() + static_cast<std::ptrdiff_t>((k + 1) * n));
}

template <typename T>
static std::vector<T> gather(const std::vector<testing::VectorSink<T>*>& sinks) {
    std::vector<T> y;
    for (auto* s : sinks) y.insert(y.end(), s->_samples.begin(), s->_samples.end());
    return y;
}

// (the scheduler owns the graph's blocks: the caller keeps it for as long as it reads the sinks)
using SchedulerPtr = decltype(std::declval<PluginLoader&>().instantiateScheduler(""));
static int run(PluginLoader& loader, Graph&& g, const std::string& what, SchedulerPtr& sched) {
    sched = loader.instantiateScheduler("gr::scheduler::Simple");
    if (!sched) return 1;
    sched->exchange(std::move(g));
    if (const auto r = sched->runAndWait(); !r) {
        std::fprintf(stderr, "%s graph: %s\n", what.c_str(), r.error().message.c_str());
        return 3;
    }
    return 0;
}

template <typename T>
static int power_factor_graph(PluginLoader& loader, const std::string& domain, const std::string& dir, std::size_t phases, bool with_phase, double phase_ulp) {
    const std::string tag  = "pf" + std::to_string(phases) + "_" + tname<T>();
    const std::string type = (phases == 1 ? "gr::electrical::SinglePhasePowerFactorCalculator<"s : "gr::electrical::ThreePhasePowerFactorCalculator<"s) + portable<T>() + ">";
    const auto        P = read_bin<T>(dir + "/P_" + tname<T>() + ".bin"), S = read_bin<T>(dir + "/S_" + tname<T>() + ".bin");
    Graph             g;
    auto&             blk = g.addBlock(loader.instantiate(type, {{"compute_domain", domain}}));
    EXPECT(blk.compute_domain().is_device() == (domain != "host"));
    std::vector<testing::VectorSink<T>*> f, a;
    for (std::size_t k = 0; k < phases; ++k) {
        const std::string sub = "#" + std::to_string(k);
        auto&             sp  = g.emplaceBlock<testing::VectorSource<T>>();
        auto&             ss  = g.emplaceBlock<testing::VectorSource<T>>();
        sp.values             = row(P, k);
        ss.values             = row(S, k);
        EXPECT(g.connect(sp, "out"s, blk, "P" + sub).has_value() && g.connect(ss, "out"s, blk, "S" + sub).has_value());
        f.push_back(&g.emplaceBlock<testing::VectorSink<T>>());
        EXPECT(g.connect(blk, "power_factor" + sub, *f.back(), "in"s).has_value());
        if (with_phase) {
            a.push_back(&g.emplaceBlock<testing::VectorSink<T>>());
            EXPECT(g.connect(blk, "phase" + sub, *a.back(), "in"s).has_value());
        }
    }
    SchedulerPtr sched;
    if (const int rc = run(loader, std::move(g), tag, sched)) return rc;
    deliver(dir, tag + "_power_factor", gather(f), -1.0);
    if (with_phase) deliver(dir, tag + "_phase", gather(a), phase_ulp);
    return 0;
}

template <typename T>
static int unbalance_graph(PluginLoader& loader, const std::string& domain, const std::string& dir, std::size_t phases, bool with_total, bool total_alone = false) {
    const std::string tag  = "ub" + std::to_string(phases) + (total_alone ? "t_" : "_") + tname<T>();
    const std::string type = (phases == 2 ? "gr::electrical::TwoPhaseSystemUnbalanceCalculator<"s : "gr::electrical::ThreePhaseSystemUnbalanceCalculator<"s) + portable<T>() + ">";
    const auto        U = read_bin<T>(dir + "/U_" + tname<T>() + ".bin"), I = read_bin<T>(dir + "/I_" + tname<T>() + ".bin"), P = read_bin<T>(dir + "/P_" + tname<T>() + ".bin");
    Graph             g;
    auto&             blk = g.addBlock(loader.instantiate(type, {{"compute_domain", domain}}));
    for (std::size_t k = 0; k < phases; ++k) {
        const std::string sub = "#" + std::to_string(k);
        auto &su = g.emplaceBlock<testing::VectorSource<T>>(), &si = g.emplaceBlock<testing::VectorSource<T>>(), &sp = g.emplaceBlock<testing::VectorSource<T>>();
        su.values = row(U, k);
        si.values = row(I, k);
        sp.values = row(P, k);
        if (total_alone)
            for (auto* s : {&su, &si, &sp}) s->values.resize(256);
        EXPECT(g.connect(su, "out"s, blk, "voltage_rms_inputs" + sub).has_value() && g.connect(si, "out"s, blk, "current_rms_inputs" + sub).has_value() &&
               g.connect(sp, "out"s, blk, "active_power_inputs" + sub).has_value());
    }
    testing::VectorSink<T>* vu = total_alone ? nullptr : &g.emplaceBlock<testing::VectorSink<T>>();
    testing::VectorSink<T>* vi = total_alone ? nullptr : &g.emplaceBlock<testing::VectorSink<T>>();
    testing::VectorSink<T>* vt = with_total ? &g.emplaceBlock<testing::VectorSink<T>>() : nullptr;
    if (vu) EXPECT(g.connect(blk, "voltage_unbalance_output"s, *vu, "in"s).has_value() && g.connect(blk, "current_unbalance_output"s, *vi, "in"s).has_value());
    if (vt) EXPECT(g.connect(blk, "total_active_power_output"s, *vt, "in"s).has_value());
    SchedulerPtr sched;
    if (const int rc = run(loader, std::move(g), tag, sched)) return rc;
    if (vt) deliver(dir, tag + "_P_total", vt->_samples, -1.0);
    if (vu) deliver(dir, tag + "_U_unbalance", vu->_samples, -1.0);
    if (vi) deliver(dir, tag + "_I_unbalance", vi->_samples, -1.0);
    return 0;
}

static const char* kChainGrc = R"(
blocks:
  - id: gr::electrical::ThreePhasePowerMetrics<float32>
    parameters:
      name: metrics
      decimate: 7
      compute_domain: "DOMAIN"
  - id: gr::electrical::ThreePhasePowerFactorCalculator<float32>
    parameters:
      name: factor
      compute_domain: "DOMAIN"
  - id: gr::electrical::ThreePhaseSystemUnbalanceCalculator<float32>
    parameters:
      name: unbalance
      compute_domain: "DOMAIN"
)";

// PowerMetrics -> PowerFactor + SystemUnbalance: the metrics' P feeds both (a fan-out), S the power factor, U_rms and I_rms the unbalance
static int chain_graph(PluginLoader& loader, const std::string& domain, const std::string& dir, bool from_grc) {
    const std::string tag = from_grc ? "grc" : "chain";
    const auto        u = read_bin<float>(dir + "/u.f32"), i = read_bin<float>(dir + "/i.f32");
    Graph             g;
    BlockModel *      pm = nullptr, *pf = nullptr, *ub = nullptr;
    std::vector<BlockModel*> src, snk;
    const char*       sink_names[9] = {"power_factor0", "power_factor1", "power_factor2", "phase0", "phase1", "phase2", "P_total", "U_unbalance", "I_unbalance"};
    if (from_grc) {
        std::string text = kChainGrc;
        for (int k = 0; k < 6; ++k) text += "  - id: gr::testing::VectorSource<float32>\n    parameters:\n      name: src" + std::to_string(k) + "\n";
        for (const char* n : sink_names) text += "  - id: gr::testing::VectorSink<float32>\n    parameters:\n      name: "s + n + "\n";
        text += "connections:\n";
        for (int k = 0; k < 3; ++k) {
            const std::string s = std::to_string(k);
            text += "  - [src" + s + ", out, metrics, U#" + s + "]\n  - [src" + std::to_string(3 + k) + ", out, metrics, I#" + s + "]\n";
            text += "  - [metrics, P#" + s + ", factor, P#" + s + "]\n  - [metrics, S#" + s + ", factor, S#" + s + "]\n";
            text += "  - [metrics, U_rms#" + s + ", unbalance, voltage_rms_inputs#" + s + "]\n  - [metrics, I_rms#" + s + ", unbalance, current_rms_inputs#" + s + "]\n";
            text += "  - [metrics, [0, " + s + "], unbalance, [2, " + s + "]]\n"; // ports by [index, sub-index]: output 0 is P, input 2 is active_power_inputs
            text += "  - [factor, power_factor#" + s + ", power_factor" + s + ", in]\n  - [factor, [1, " + s + "], phase" + s + ", 0]\n";
        }
        text += "  - [unbalance, total_active_power_output, P_total, in]\n  - [unbalance, 1, U_unbalance, in]\n  - [unbalance, current_unbalance_output, I_unbalance, in]\n";
        for (std::size_t at; (at = text.find("DOMAIN")) != std::string::npos;) text.replace(at, 6, domain);
        auto loaded = loadGrc(loader, g, text);
        if (!loaded) {
            std::fprintf(stderr, "grc: %s\n", loaded.error().message.c_str());
            return 3;
        }
        EXPECT(loaded.value().size() == 18u);
        pm = loaded.value()[0].model;
        pf = loaded.value()[1].model;
        ub = loaded.value()[2].model;
        for (std::size_t k = 0; k < 6; ++k) src.push_back(loaded.value()[3 + k].model);
        for (std::size_t k = 0; k < 9; ++k) snk.push_back(loaded.value()[9 + k].model);
    } else {
        pm = &g.addBlock(loader.instantiate("gr::electrical::ThreePhasePowerMetrics<float32>", {{"decimate", std::int64_t(7)}, {"compute_domain", domain}}));
        pf = &g.addBlock(loader.instantiate("gr::electrical::ThreePhasePowerFactorCalculator<float32>", {{"compute_domain", domain}}));
        ub = &g.addBlock(loader.instantiate("gr::electrical::ThreePhaseSystemUnbalanceCalculator<float32>", {{"compute_domain", domain}}));
        for (int k = 0; k < 6; ++k) src.push_back(&g.addBlock(loader.instantiate("gr::testing::VectorSource<float32>")));
        for (int k = 0; k < 9; ++k) snk.push_back(&g.addBlock(loader.instantiate("gr::testing::VectorSink<float32>")));
        for (std::size_t k = 0; k < 3; ++k) {
            const std::string sub = "#" + std::to_string(k);
            EXPECT(g.connect(*src[k], "out"s, *pm, "U" + sub).has_value() && g.connect(*src[3 + k], "out"s, *pm, "I" + sub).has_value());
            EXPECT(g.connect(*pm, "P" + sub, *pf, "P" + sub).has_value() && g.connect(*pm, "S" + sub, *pf, "S" + sub).has_value());
            EXPECT(g.connect(*pm, "U_rms" + sub, *ub, "voltage_rms_inputs" + sub).has_value() && g.connect(*pm, "I_rms" + sub, *ub, "current_rms_inputs" + sub).has_value() &&
                   g.connect(*pm, "P" + sub, *ub, "active_power_inputs" + sub).has_value());
            EXPECT(g.connect(*pf, "power_factor" + sub, *snk[k], "in"s).has_value() && g.connect(*pf, "phase" + sub, *snk[3 + k], "in"s).has_value());
        }
        EXPECT(g.connect(*ub, "total_active_power_output"s, *snk[6], "in"s).has_value() && g.connect(*ub, "voltage_unbalance_output"s, *snk[7], "in"s).has_value() &&
               g.connect(*ub, "current_unbalance_output"s, *snk[8], "in"s).has_value());
    }
    for (std::size_t k = 0; k < 3; ++k) {
        static_cast<testing::VectorSource<float>*>(src[k]->raw())->values     = row(u, k);
        static_cast<testing::VectorSource<float>*>(src[3 + k]->raw())->values = row(i, k);
    }
    EXPECT(pm->compute_domain().is_device() && pf->compute_domain().is_device() && ub->compute_domain().is_device());
    SchedulerPtr sched;
    if (const int rc = run(loader, std::move(g), tag, sched)) return rc;
    for (std::size_t k = 0; k < 9; ++k) write_bin(dir + "/" + tag + "_" + sink_names[k] + ".bin", static_cast<testing::VectorSink<float>*>(snk[k]->raw())->_samples);
    std::printf("%s: %zu outputs per port\n", tag.c_str(), static_cast<testing::VectorSink<float>*>(snk[0]->raw())->_samples.size());
    return 0;
}

template <typename T>
static void members(PluginLoader& loader, const std::string& domain) {
    const std::string t = "<"s + portable<T>() + ">";
    for (const char* n : {"gr::electrical::SinglePhasePowerFactorCalculator", "gr::electrical::ThreePhasePowerFactorCalculator", "gr::electrical::TwoPhaseSystemUnbalanceCalculator",
                          "gr::electrical::ThreePhaseSystemUnbalanceCalculator"}) {
        EXPECT(loader.isBlockAvailable(n + t));
        EXPECT(loader.instantiate(n + t, {{"compute_domain", domain}}) != nullptr);
    }
    {
        auto  b   = loader.instantiate("gr::electrical::ThreePhasePowerFactorCalculator" + t);
        auto* blk = b ? static_cast<electrical::ThreePhasePowerFactorCalculator<T>*>(b->raw()) : nullptr;
        EXPECT(blk && blk->P.size() == 3u && blk->S.size() == 3u && blk->power_factor.size() == 3u && blk->phase.size() == 3u);
        auto  b1   = loader.instantiate("gr::electrical::SinglePhasePowerFactorCalculator" + t);
        auto* blk1 = b1 ? static_cast<electrical::SinglePhasePowerFactorCalculator<T>*>(b1->raw()) : nullptr;
        EXPECT(blk1 && blk1->P.size() == 1u && blk1->phase.size() == 1u);
        constexpr auto names = electrical::ThreePhasePowerFactorCalculator<T>::gr_member_names();
        const char*    want[] = {"P", "S", "power_factor", "phase"};
        EXPECT(names.size() == 4u);
        for (std::size_t k = 0; k < std::min<std::size_t>(names.size(), 4); ++k) EXPECT(std::string_view(names[k]) == want[k]);
    }
    {
        auto  b   = loader.instantiate("gr::electrical::TwoPhaseSystemUnbalanceCalculator" + t);
        auto* blk = b ? static_cast<electrical::TwoPhaseSystemUnbalanceCalculator<T>*>(b->raw()) : nullptr;
        EXPECT(blk && blk->voltage_rms_inputs.size() == 2u && blk->current_rms_inputs.size() == 2u && blk->active_power_inputs.size() == 2u);
        constexpr auto names = electrical::ThreePhaseSystemUnbalanceCalculator<T>::gr_member_names();
        const char*    want[] = {"voltage_rms_inputs", "current_rms_inputs", "active_power_inputs", "total_active_power_output", "voltage_unbalance_output", "current_unbalance_output"};
        EXPECT(names.size() == 6u);
        for (std::size_t k = 0; k < std::min<std::size_t>(names.size(), 6); ++k) EXPECT(std::string_view(names[k]) == want[k]);
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s plugin.so compute_domain [dir [phase_ulp_f32 phase_ulp_f64]]\n", argv[0]); return 2; }
    const std::string domain = argv[2];
    PluginLoader      loader;
    const auto        ok = loader.load(argv[1]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    members<float>(loader, domain);
    members<double>(loader, domain);
    if (argc >= 4) {
        const std::string dir = argv[3];
        const double      b32 = argc >= 6 ? std::atof(argv[4]) : 2.0, b64 = argc >= 6 ? std::atof(argv[5]) : 2.0;
        int               rc;
        if ((rc = power_factor_graph<float>(loader, domain, dir, 3, true, b32)) || (rc = power_factor_graph<float>(loader, domain, dir, 1, false, b32)) ||
            (rc = power_factor_graph<double>(loader, domain, dir, 3, true, b64)) || (rc = power_factor_graph<double>(loader, domain, dir, 1, false, b64)) ||
            (rc = unbalance_graph<float>(loader, domain, dir, 3, true)) || (rc = unbalance_graph<float>(loader, domain, dir, 2, false)) ||
            (rc = unbalance_graph<double>(loader, domain, dir, 3, true)) || (rc = unbalance_graph<double>(loader, domain, dir, 2, false)) ||
            (rc = unbalance_graph<float>(loader, domain, dir, 3, true, true)))
            return rc;
        if (domain != "host" && exists(dir + "/u.f32")) {
            if ((rc = chain_graph(loader, domain, dir, false)) || (rc = chain_graph(loader, domain, dir, true))) return rc;
        }
    }
    if (failures) std::printf("host-electrical: %d FAILURES\n", failures);
    else std::printf("host-electrical: all checks passed (compute_domain %s)\n", domain.c_str());
    return failures ? 1 : 0;
}
