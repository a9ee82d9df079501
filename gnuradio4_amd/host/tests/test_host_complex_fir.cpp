// gr::filter::complex_fir_filter<std::complex<float>> of the host layer (gr4/blocks.hpp, gr4/hip.hpp): complex taps on a complex stream, direct and decimating.
//   test_host_complex_fir host   <libgr4hip_blocks.so>   the CPU body against values computed here, the settings errors, the plugin registration,
//                                                        gr:sample_rate forwarded divided by `decimate`
//   test_host_complex_fir device <libgr4hip_blocks.so>   source -> complex_fir_filter -> sink on gpu:hip:0 against the CPU body, alone (the compute_domain seam)
//                                                        and inside a hip::plan run behind a Rotator
// Exit code 0: everything held; 1: a check failed; 3: a graph failed (a device domain without a device fails loudly).
#include <cstdio>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32 = std::complex<float>;
using B   = filter::complex_fir_filter<C32>;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static std::vector<C32> stream(std::size_t n, std::uint32_t seed) {
    std::vector<C32> x(n);
    std::uint32_t    lcg = seed;
    const auto       next = [&] { lcg = lcg * 1664525u + 1013904223u; return static_cast<float>(static_cast<std::int32_t>(lcg >> 8) % 2001 - 1000) / 1000.f; };
    for (auto& v : x) { const float re = next(), im = next(); v = {re, im}; }
    return x;
}
struct Taps {
    std::vector<float> re, im;
};
static Taps taps(std::size_t K, double shift) { // Hamming-windowed low-pass moved to `shift` fs
    Taps t;
    for (std::size_t k = 0; k < K; ++k) {
        const double w = (0.54 - 0.46 * std::cos(2 * std::numbers::pi * double(k) / double(K > 1 ? K - 1 : 1))) / (0.54 * double(K));
        t.re.push_back(static_cast<float>(w * std::cos(2 * std::numbers::pi * shift * double(k))));
        t.im.push_back(static_cast<float>(w * std::sin(2 * std::numbers::pi * shift * double(k))));
    }
    return t;
}
// the definition, in double: y[m] = sum_k b[k] x[m D - k], zero history
static std::vector<C32> direct(const Taps& t, const std::vector<C32>& x, std::size_t D) {
    std::vector<C32> y(x.size() / D);
    for (std::size_t m = 0; m < y.size(); ++m) {
        std::complex<double> acc{};
        for (std::size_t k = 0; k < t.re.size() && k <= m * D; ++k) acc += std::complex<double>(t.re[k], t.im[k]) * std::complex<double>(x[m * D - k]);
        y[m] = static_cast<C32>(acc);
    }
    return y;
}
static double max_rel(const std::vector<C32>& got, const std::vector<C32>& want) { // max |got - want| / max(|want|, rms(want))
    if (got.size() != want.size() || want.empty()) return 1e30;
    double rms = 0;
    for (const auto& v : want) rms += std::norm(std::complex<double>(v));
    rms = std::sqrt(rms / double(want.size()));
    double worst = 0;
    for (std::size_t i = 0; i < want.size(); ++i) worst = std::max(worst, std::abs(std::complex<double>(got[i]) - std::complex<double>(want[i])) / std::max(std::abs(std::complex<double>(want[i])), rms));
    return worst;
}

// source -> [Rotator ->] complex_fir_filter -> sink; domain "" = host
static int run_graph(const Taps& t, std::size_t D, const std::vector<C32>& x, const std::string& domain, bool rotator, bool planned, std::vector<C32>& y, std::vector<Tag>* tags = nullptr) {
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
    src.values = x;
    if (tags) src._tags = {{0, {{"gr:sample_rate", 1000.f}}}};
    property_map cfg{{"b_real", t.re}, {"b_imag", t.im}, {"decimate", std::int64_t(D)}};
    property_map rcfg{{"phase_increment", 0.25}};
    if (!domain.empty()) { cfg["compute_domain"] = domain; rcfg["compute_domain"] = domain; }
    auto& fir  = g.emplaceBlock<B>(cfg);
    fir._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<C32>>();
    if (rotator) {
        auto& rot = g.emplaceBlock<blocks::math::Rotator<C32>>(rcfg);
        if (!g.connect<"out", "in">(src, rot) || !g.connect<"out", "in">(rot, fir)) return 2;
    } else if (!g.connect<"out", "in">(src, fir)) return 2;
    if (!g.connect<"out", "in">(fir, sink)) return 2;
    if (planned) {
        const auto runs = hip::plan(g, rotator ? 2 : 1); // (alone: a run of one stage)
        std::printf("planner: %zu runs:", runs.size());
        for (auto* r : runs) std::printf(" [%s]", std::string(r->description()).c_str());
        std::printf("\n");
        EXPECT(runs.size() == 1 && runs[0]->stages().size() == (rotator ? 2u : 1u) && std::string(runs[0]->description()).find("cfir_c32") != std::string::npos);
    }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (!domain.empty() && !planned) EXPECT(fir._device_state != nullptr); // the seam was taken
    y = sink._samples;
    if (tags) *tags = sink._tags;
    return 0;
}

static int host_checks(PluginLoader& loader) {
    { // the body against the definition evaluated here, direct and decimating, in one piece and sample by sample across calls
        for (const auto& [K, D] : {std::pair<std::size_t, std::size_t>{1, 1}, {5, 1}, {33, 2}, {64, 3}, {100, 8}}) {
            const Taps t = taps(K, 0.2);
            const auto x = stream(D * 700, 17u + static_cast<std::uint32_t>(K));
            B          f;
            f.applySettings({{"b_real", t.re}, {"b_imag", t.im}, {"decimate", std::int64_t(D)}});
            EXPECT(f.input_chunk_size == D);
            std::vector<C32> y(x.size() / D);
            EXPECT(f.processBulk(std::span<const C32>(x), std::span<C32>(y)) == work::Status::OK);
            const auto want = direct(t, x, D);
            EXPECT(max_rel(y, want) <= 1e-5);
            B f2; // the history is carried: chunks of D samples give the same stream
            f2.applySettings({{"b_real", t.re}, {"b_imag", t.im}, {"decimate", std::int64_t(D)}});
            std::vector<C32> y2(y.size());
            for (std::size_t m = 0; m < y2.size(); ++m) EXPECT(f2.processBulk(std::span<const C32>(x.data() + m * D, D), std::span<C32>(y2.data() + m, 1)) == work::Status::OK);
            EXPECT(y2 == y);
            f2.reset();
            std::vector<C32> y3(y.size());
            (void)f2.processBulk(std::span<const C32>(x), std::span<C32>(y3));
            EXPECT(y3 == y); // reset cleared the history
        }
        // an impulse reads the taps back; j times the impulse gives j b
        const Taps t = taps(9, 0.3);
        B          f;
        f.applySettings({{"b_real", t.re}, {"b_imag", t.im}});
        std::vector<C32> x(12), y(12);
        x[1] = {1.f, 0.f};
        (void)f.processBulk(std::span<const C32>(x), std::span<C32>(y));
        for (std::size_t k = 0; k < 9; ++k) EXPECT(y[1 + k] == C32(t.re[k], t.im[k]));
        f.reset();
        x[1] = {0.f, 1.f};
        (void)f.processBulk(std::span<const C32>(x), std::span<C32>(y));
        for (std::size_t k = 0; k < 9; ++k) EXPECT(y[1 + k] == C32(-t.im[k], t.re[k]));
    }
    { // the settings errors; the reflected members
        B    f;
        bool threw = false;
        try { f.applySettings({{"b_real", std::vector<float>{1.f, 2.f}}, {"b_imag", std::vector<float>{0.f}}}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
        B g;
        threw = false;
        try { g.applySettings({{"decimate", std::int64_t(0)}}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
        B e;
        threw = false;
        try { e.applySettings({{"b_real", std::vector<float>{}}, {"b_imag", std::vector<float>{}}}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
        constexpr auto                        names = B::gr_member_names();
        const std::array<std::string_view, 5> want{"in", "out", "b_real", "b_imag", "decimate"};
        EXPECT(names.size() == want.size());
        for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
        B d; // defaults: the identity
        EXPECT(d.b_real == std::vector<float>{1.f} && d.b_imag == std::vector<float>{0.f} && d.decimate == 1u);
    }
    { // the plugin knows the block under the portable type name
        const std::string n = "gr::filter::complex_fir_filter<complex<float32>>";
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"b_real", std::vector<float>{0.5f, 0.25f}}, {"b_imag", std::vector<float>{0.f, -0.25f}}, {"decimate", std::int64_t(2)}}) != nullptr);
        EXPECT(!loader.isBlockAvailable("gr::filter::complex_fir_filter<float32>")); // complex streams only
    }
    { // in a graph: gr:sample_rate is forwarded divided by `decimate`, and the graph's output is the body's
        const Taps       t = taps(33, 0.2);
        const auto       x = stream(8 * 500, 5u);
        std::vector<C32> y;
        std::vector<Tag> tags;
        if (int rc = run_graph(t, 8, x, "", false, false, y, &tags)) return rc;
        EXPECT(max_rel(y, direct(t, x, 8)) <= 1e-5);
        EXPECT(tags.size() == 1u);
        if (tags.size() == 1) EXPECT(tags[0].index == 0u && (tags[0].map == property_map{{"gr:sample_rate", 125.f}}));
    }
    return 0;
}

static int device_checks() {
    const std::string dom = "gpu:hip:0";
    for (const auto& [K, D] : {std::pair<std::size_t, std::size_t>{5, 1}, {64, 1}, {128, 8}, {300, 3}}) {
        const Taps       t = taps(K, 0.2);
        const auto       x = stream(D * 40000, 99u + static_cast<std::uint32_t>(K));
        std::vector<C32> h, d, p;
        if (int rc = run_graph(t, D, x, "", false, false, h)) return rc;
        if (int rc = run_graph(t, D, x, dom, false, false, d)) return rc; // the block's own work() behind the seam
        if (int rc = run_graph(t, D, x, dom, false, true, p)) return rc;  // a planned run of one stage
        const double e1 = max_rel(d, h), e2 = max_rel(p, h);
        std::printf("complex_fir_filter K %zu D %zu: seam %.3g, planned %.3g%s\n", K, D, e1, e2, e1 <= 1e-5 && e2 <= 1e-5 ? "" : "  FAILED");
        EXPECT(e1 <= 1e-5 && e2 <= 1e-5);
    }
    { // behind a Rotator inside one hip::plan run
        const Taps       t = taps(128, 0.2);
        const auto       x = stream(8 * 30000, 7u);
        std::vector<C32> h, p;
        if (int rc = run_graph(t, 8, x, "", true, false, h)) return rc;
        if (int rc = run_graph(t, 8, x, dom, true, true, p)) return rc;
        // the host Rotator is the reference's float accumulator, which drifts (~1e-7 rad per step); the device evaluates the phase in closed form: compare with
        // the float64 phase in front of the definition
        std::vector<C32> xr(x.size());
        const double     inc = static_cast<double>(0.25f);
        for (std::size_t i = 0; i < x.size(); ++i) xr[i] = static_cast<C32>(std::complex<double>(x[i]) * std::polar(1.0, std::fmod(static_cast<double>(i + 1) * inc, 2.0 * std::numbers::pi)));
        const auto   want = direct(t, xr, 8);
        const double e = max_rel(p, want), eh = max_rel(std::vector<C32>(h.begin(), h.begin() + 16), std::vector<C32>(want.begin(), want.begin() + 16));
        std::printf("Rotator -> complex_fir_filter planned: %.3g (host body, first 16 outputs: %.3g)%s\n", e, eh, e <= 1e-5 && eh <= 1e-5 ? "" : "  FAILED");
        EXPECT(e <= 1e-5 && eh <= 1e-5);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s host|device plugin.so\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    PluginLoader      loader;
    const auto        ok = loader.load(argv[2]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    try {
        if (int rc = mode == "device" ? device_checks() : host_checks(loader)) return rc;
    } catch (const std::exception& e) { // (the planner makes its stages before anything runs: no device, no stage)
        std::fprintf(stderr, "graph: %s\n", e.what());
        return 3;
    }
    if (failures) std::printf("complex_fir %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("complex_fir %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
