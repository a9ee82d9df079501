// gr::blocks::fft::CrossSpectrum<float> of the host layer (gr4/blocks.hpp, gr4/hip.hpp): the averaged cross-spectral matrix of n_inputs spectra (CROSS_SPECTRUM.md).
//   test_host_cross_spectrum host   <libgr4hip_blocks.so> <prefix>   sources -> CrossSpectrum -> sink in a host-domain graph; inputs and output as files for
//                                                                   tests/test_cross_spectrum_host.py (which compares them bit for bit with the oracle's ordered
//                                                                   definition), the settings errors, the chunk sizes, gr:sample_rate, the plugin
//   test_host_cross_spectrum device <libgr4hip_blocks.so> <prefix>   the same graph with the block on gpu:hip:0 (the seam onto gr4hip_xcorr_process); files for
//                                                                   tests/test_gpu_cross_spectrum.py; and the seam's handle re-make: n_integrate changed by a
//                                                                   settings tag between two work() calls, device against the host body bit for bit
// Files: <prefix>.<name> = raw float32 {re, im} pairs; the input is [n_inputs][frames][vector_size].  Exit code 0: everything held; 1: a check failed; 3: a graph failed.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32   = std::complex<float>;
using Cross = blocks::fft::CrossSpectrum<float>;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

// noise in [-1, 1] per stream plus a component every stream shares
static std::vector<std::vector<C32>> streams(std::size_t S, std::size_t n, std::uint32_t seed) {
    std::uint32_t lcg  = seed;
    const auto    next = [&] { lcg = lcg * 1664525u + 1013904223u; return static_cast<float>(static_cast<std::int32_t>(lcg >> 8) % 2001 - 1000) / 1000.f; };
    std::vector<C32> common(n);
    for (auto& v : common) { const float re = next(), im = next(); v = C32(re, im); }
    std::vector<std::vector<C32>> x(S, std::vector<C32>(n));
    for (std::size_t s = 0; s < S; ++s) {
        const C32 g = static_cast<C32>(std::polar(0.7, 0.9 * static_cast<double>(s)));
        for (std::size_t i = 0; i < n; ++i) { const float re = next(), im = next(); x[s][i] = C32(re, im) + g * common[i]; }
    }
    return x;
}
template <typename V>
static void dump(const std::string& path, const std::vector<V>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(V)));
    if (!f) { ++failures; std::printf("FAIL cannot write %s\n", path.c_str()); }
}
static bool throws(const property_map& settings) {
    Cross b;
    try { b.applySettings(settings); } catch (const std::invalid_argument&) { return true; }
    return false;
}

static int graph(const std::string& domain, std::size_t N, std::size_t A, bool mean, const std::vector<std::vector<C32>>& x, std::vector<C32>& y, std::vector<Tag>* tags = nullptr,
                 const std::vector<Tag>& settings_tags = {}) {
    Graph        g;
    property_map cfg{{"n_inputs", std::int64_t(x.size())}, {"vector_size", std::int64_t(N)}, {"n_integrate", std::int64_t(A)}, {"mean", mean}};
    if (!domain.empty()) cfg["compute_domain"] = domain;
    auto& blk  = g.emplaceBlock<Cross>(cfg);
    auto& sink = g.emplaceBlock<testing::VectorSink<C32>>();
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    for (std::size_t s = 0; s < x.size(); ++s) {
        auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
        src.values = x[s];
        if (tags) src._tags = {{0, {{"gr:sample_rate", 48000.f}}}};
        if (s == 0 && !settings_tags.empty()) src._tags = settings_tags;
        if (!g.connect(src, "out"s, blk, "in#"s + std::to_string(s))) return 2;
    }
    if (!g.connect<"out", "in">(blk, sink)) return 2;
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (!domain.empty()) EXPECT(blk._device_state != nullptr); // the seam was taken
    EXPECT(blk._settings_by_tag == settings_tags.size());
    y = sink._samples;
    if (tags) *tags = sink._tags;
    return 0;
}

static int dumped_cases(const std::string& domain, const std::string& prefix) {
    struct Shape { std::size_t S, N, A; };
    for (const auto& [S, N, A] : {Shape{2, 8, 1}, Shape{3, 16, 63}, Shape{5, 8, 65}, Shape{4, 8, 130}}) {
        for (const bool mean : {false, true}) {
            const std::size_t frames = 2 * A + 3;
            const auto        x      = streams(S, N * frames, 11u + static_cast<std::uint32_t>(S + N + A));
            std::vector<C32>  y, flat;
            if (int rc = graph(domain, N, A, mean, x, y)) return rc;
            EXPECT(y.size() == frames / A * (S * (S + 1) / 2) * N); // A > 3: the three trailing frames complete nothing
            for (const auto& row : x) flat.insert(flat.end(), row.begin(), row.end());
            const std::string tag = prefix + ".S" + std::to_string(S) + ".N" + std::to_string(N) + ".A" + std::to_string(A) + (mean ? ".mean" : ".sum");
            dump(tag + ".in", flat);
            dump(tag + ".out", y);
        }
    }
    return 0;
}

// S = 2, vector_size 16: one integration of two frames (one work() call: the chunk ends where the tag starts), then n_integrate 4 by settings, then one integration of
// four frames.  The seam's handle was made for n_integrate 2 and has to be made anew.  Device against the host body: both are the ordered definition, bit for bit.
static int remake_case() {
    const std::size_t      N = 16;
    const auto             x = streams(2, N * (2 + 4), 5u);
    const std::vector<Tag> to_four{{N * 2, {{"n_integrate", std::int64_t(4)}}}};
    std::vector<C32>       dev, host;
    if (int rc = graph("gpu:hip:0", N, 2, false, x, dev, nullptr, to_four)) return rc;
    if (int rc = graph("", N, 2, false, x, host, nullptr, to_four)) return rc;
    EXPECT(host.size() == 2 * 3 * N && dev.size() == host.size() && std::memcmp(dev.data(), host.data(), host.size() * sizeof(C32)) == 0);
    EXPECT(host[0] != host[3 * N]); // two frames summed, then four: not the same matrix twice
    std::printf("handle re-make (n_integrate 2 -> 4 by settings): %zu values, device == host\n", dev.size());
    return 0;
}

static int host_checks(PluginLoader& loader, const std::string& prefix) {
    if (int rc = dumped_cases("", prefix)) return rc;
    { // gr:sample_rate leaves scaled by output_chunk_size / input_chunk_size = P / n_integrate
        const std::size_t             N = 16, A = 48, S = 2;
        std::vector<std::vector<C32>> x(S, std::vector<C32>(N * A * 3, C32(1.f, 0.f)));
        std::vector<C32>              y;
        std::vector<Tag>              tags;
        if (int rc = graph("", N, A, false, x, y, &tags)) return rc;
        EXPECT(y.size() == 3 * 3 * N && y[0] == C32(48.f, 0.f) && y[N] == C32(48.f, 0.f));
        EXPECT(tags.size() == 1u);
        if (tags.size() == 1) EXPECT(tags[0].index == 0u && (tags[0].map == property_map{{"gr:sample_rate", 3000.f}}));
    }
    { // the settings errors, the chunk sizes, the reflected members, the defaults
        EXPECT(throws({{"n_inputs", std::int64_t(1)}}));
        EXPECT(throws({{"n_inputs", std::int64_t(33)}}));
        EXPECT(throws({{"vector_size", std::int64_t(1)}}));
        EXPECT(throws({{"vector_size", std::int64_t(0)}}));
        EXPECT(throws({{"n_integrate", std::int64_t(0)}}));
        EXPECT(!throws({{"n_inputs", std::int64_t(32)}, {"vector_size", std::int64_t(1000)}, {"n_integrate", std::int64_t(7)}, {"mean", true}}));
        Cross b;
        b.applySettings({{"n_inputs", std::int64_t(5)}, {"vector_size", std::int64_t(1000)}, {"n_integrate", std::int64_t(7)}});
        EXPECT(b.input_chunk_size == 7000u && b.output_chunk_size == 15000u && b.in.size() == 5u);
        constexpr auto                        names = Cross::gr_member_names();
        const std::array<std::string_view, 6> want{"in", "out", "n_inputs", "vector_size", "n_integrate", "mean"};
        EXPECT(names.size() == want.size());
        for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
        Cross d;
        EXPECT(d.n_inputs == 2u && d.vector_size == 1024u && d.n_integrate == 1u && !d.mean && d.in.size() == 2u);
        EXPECT(gr4hip_xcorr_leaf() == 64u);
    }
    { // the plugin knows the block under its portable type name
        const std::string n = "gr::blocks::fft::CrossSpectrum<float32>";
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"n_inputs", std::int64_t(3)}, {"vector_size", std::int64_t(64)}, {"n_integrate", std::int64_t(3)}}) != nullptr);
        std::printf("plugin: %s %s\n", n.c_str(), loader.isBlockAvailable(n) ? "available" : "MISSING");
        EXPECT(!loader.isBlockAvailable("gr::blocks::fft::CrossSpectrum<float64>")); // float64 spectra are out of scope
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s host|device plugin.so output-prefix\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    PluginLoader      loader;
    const auto        ok = loader.load(argv[2]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    try {
        if (int rc = mode == "device" ? dumped_cases("gpu:hip:0", argv[3]) : host_checks(loader, argv[3])) return rc;
        if (int rc = mode == "device" ? remake_case() : 0) return rc;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "graph: %s\n", e.what());
        return 3;
    }
    if (failures) std::printf("cross spectrum %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("cross spectrum %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
