// gr::blocks::fft::SpectrumIntegrator<float> of the host layer (gr4/blocks.hpp, gr4/hip.hpp): sum / mean of n_integrate power spectra (SPECTRUM_INTEGRATOR.md).
//   test_host_spectrum_integrator host   <libgr4hip_blocks.so> <prefix>   source -> SpectrumIntegrator -> sink in a host-domain graph; input and output as files for
//                                                                        tests/test_spectrum_integrator_host.py (which compares them bit for bit with the oracle's
//                                                                        ordered sums), the settings errors, gr:sample_rate divided by n_integrate, the plugin
//   test_host_spectrum_integrator device <libgr4hip_blocks.so> <prefix>   source -> PowerSpectrum | PfbPowerSpectrum -> SpectrumIntegrator -> sink on gpu:hip:0: as a
//                                                                        hip::plan run (one fused stage) and unplanned (two device blocks); outputs as files for
//                                                                        tests/test_gpu_spectrum_integrator.py (which compares them with the C-ABI's)
// Files: <prefix>.<name> = raw float32 (complex values as {re, im} pairs).  Exit code 0: everything held; 1: a check failed; 3: a graph failed.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32   = std::complex<float>;
using Integ = blocks::fft::SpectrumIntegrator<float>;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static std::vector<C32> stream(std::size_t n, std::uint32_t seed) { // noise in [-1, 1] plus a tone
    std::vector<C32> x(n);
    std::uint32_t    lcg = seed;
    const auto       next = [&] { lcg = lcg * 1664525u + 1013904223u; return static_cast<float>(static_cast<std::int32_t>(lcg >> 8) % 2001 - 1000) / 1000.f; };
    for (std::size_t i = 0; i < n; ++i) {
        const float re = next(), im = next();
        x[i] = C32(re, im) + static_cast<C32>(std::polar(2.0, 2.0 * std::numbers::pi * 0.137 * static_cast<double>(i)));
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
    Integ b;
    try { b.applySettings(settings); } catch (const std::invalid_argument&) { return true; }
    return false;
}

// source -> SpectrumIntegrator -> sink in the host domain
static int host_graph(std::size_t N, std::size_t A, bool mean, const std::vector<float>& m, std::vector<float>& y, std::vector<Tag>* tags = nullptr) {
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<float>>();
    src.values = m;
    if (tags) src._tags = {{0, {{"gr:sample_rate", 48000.f}}}};
    auto& blk  = g.emplaceBlock<Integ>(property_map{{"vector_size", std::int64_t(N)}, {"n_integrate", std::int64_t(A)}, {"mean", mean}});
    auto& sink = g.emplaceBlock<testing::VectorSink<float>>();
    if (!g.connect<"out", "in">(src, blk) || !g.connect<"out", "in">(blk, sink)) return 2;
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    y = sink._samples;
    if (tags) *tags = sink._tags;
    return 0;
}

static int host_checks(PluginLoader& loader, const std::string& prefix) {
    // power-like frames (squares of the stream) through a host graph: files for the bit-for-bit comparison with the oracle
    for (const auto& [N, A] : {std::pair<std::size_t, std::size_t>{8, 1}, {16, 31}, {32, 33}, {64, 67}, {16, 32}}) {
        for (const bool mean : {false, true}) {
            const auto         x = stream(N * (2 * A + 3), 5u + static_cast<std::uint32_t>(N + A));
            std::vector<float> m(x.size()), y;
            for (std::size_t i = 0; i < x.size(); ++i) m[i] = std::norm(x[i]) * 1000.f;
            if (int rc = host_graph(N, A, mean, m, y)) return rc;
            EXPECT(y.size() == (2 * A + 3) / A * N); // A > 3: the three trailing frames complete nothing
            const std::string tag = prefix + ".N" + std::to_string(N) + ".A" + std::to_string(A) + (mean ? ".mean" : ".sum");
            dump(tag + ".in", m);
            dump(tag + ".out", y);
        }
    }
    { // gr:sample_rate leaves divided by n_integrate
        const std::size_t  N = 16, A = 48;
        std::vector<float> m(N * A * 3, 1.f), y;
        std::vector<Tag>   tags;
        if (int rc = host_graph(N, A, false, m, y, &tags)) return rc;
        EXPECT(y.size() == 3 * N && y[0] == 48.f);
        EXPECT(tags.size() == 1u);
        if (tags.size() == 1) EXPECT(tags[0].index == 0u && (tags[0].map == property_map{{"gr:sample_rate", 1000.f}}));
    }
    { // the settings errors, the chunk sizes, the reflected members, the defaults
        EXPECT(throws({{"vector_size", std::int64_t(1)}}));
        EXPECT(throws({{"vector_size", std::int64_t(0)}}));
        EXPECT(throws({{"n_integrate", std::int64_t(0)}}));
        EXPECT(!throws({{"vector_size", std::int64_t(1000)}, {"n_integrate", std::int64_t(7)}, {"mean", true}}));
        Integ b;
        b.applySettings({{"vector_size", std::int64_t(1000)}, {"n_integrate", std::int64_t(7)}});
        EXPECT(b.input_chunk_size == 7000u && b.output_chunk_size == 1000u);
        constexpr auto                        names = Integ::gr_member_names();
        const std::array<std::string_view, 5> want{"in", "out", "vector_size", "n_integrate", "mean"};
        EXPECT(names.size() == want.size());
        for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
        Integ d;
        EXPECT(d.vector_size == 1024u && d.n_integrate == 1u && !d.mean);
        EXPECT(gr4hip_specint_leaf() == 32u);
    }
    { // the plugin knows the block under its portable type name
        const std::string n = "gr::blocks::fft::SpectrumIntegrator<float32>";
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"vector_size", std::int64_t(64)}, {"n_integrate", std::int64_t(3)}}) != nullptr);
        std::printf("plugin: %s %s\n", n.c_str(), loader.isBlockAvailable(n) ? "available" : "MISSING");
        EXPECT(!loader.isBlockAvailable("gr::blocks::fft::SpectrumIntegrator<complex<float32>>")); // power spectra are float streams
    }
    return 0;
}

// source -> Spec -> SpectrumIntegrator -> sink on the device
template <typename Spec>
static int device_graph(const property_map& spec_cfg, std::size_t N, std::size_t A, const std::vector<C32>& x, bool planned, const std::string& want_kind, std::vector<float>& y) {
    const std::string dom = "gpu:hip:0";
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
    src.values = x;
    property_map cfg = spec_cfg;
    cfg["compute_domain"] = dom;
    auto& spec  = g.emplaceBlock<Spec>(cfg);
    auto& integ = g.emplaceBlock<Integ>(property_map{{"vector_size", std::int64_t(N)}, {"n_integrate", std::int64_t(A)}, {"compute_domain", dom}});
    auto& sink  = g.emplaceBlock<testing::VectorSink<float>>();
    spec._log = integ._log = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    if (!g.connect<"out", "in">(src, spec) || !g.connect<"out", "in">(spec, integ) || !g.connect<"out", "in">(integ, sink)) return 2;
    if (planned) {
        const auto runs = hip::plan(g, 1);
        for (auto* r : runs) std::printf("planned run: %zu stage(s): %s\n", r->stages().size(), std::string(r->description()).c_str());
        EXPECT(runs.size() == 1 && runs[0]->stages().size() == 1u);
        if (runs.size() == 1 && runs[0]->stages().size() == 1) EXPECT(runs[0]->stages()[0]->kind() == want_kind);
    }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (!planned) EXPECT(spec._device_state != nullptr && integ._device_state != nullptr); // both seams were taken
    y = sink._samples;
    return 0;
}

static int device_checks(const std::string& prefix) {
    const std::size_t N = 1024, A = 33, M = 2 * A + 3;
    const auto        x = stream(N * M, 77u);
    dump(prefix + ".in", x);
    using PS  = blocks::fft::PowerSpectrum<C32>;
    using PFB = blocks::fft::PfbPowerSpectrum<C32>;
    const property_map ps_cfg{{"fftSize", std::int64_t(N)}, {"window", "Hann"s}}, pfb_cfg{{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(4)}};
    std::vector<float> fp, fu, bp, bu;
    if (int rc = device_graph<PS>(ps_cfg, N, A, x, true, "power_spectrum_integrated_c32", fp)) return rc;
    if (int rc = device_graph<PS>(ps_cfg, N, A, x, false, "", fu)) return rc;
    if (int rc = device_graph<PFB>(pfb_cfg, N, A, x, true, "pfb_mag2_integrated_c32", bp)) return rc;
    if (int rc = device_graph<PFB>(pfb_cfg, N, A, x, false, "", bu)) return rc;
    EXPECT(fp.size() == 2 * N && bp.size() == 2 * N);
    EXPECT(fp == fu && bp == bu); // the fused stage and the two device blocks: the same bits (no NaN in these streams)
    dump(prefix + ".fft.planned", fp);
    dump(prefix + ".fft.seam", fu);
    dump(prefix + ".pfb.planned", bp);
    dump(prefix + ".pfb.seam", bu);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s host|device plugin.so output-prefix\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    PluginLoader      loader;
    const auto        ok = loader.load(argv[2]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    try {
        if (int rc = mode == "device" ? device_checks(argv[3]) : host_checks(loader, argv[3])) return rc;
    } catch (const std::exception& e) { // (the planner makes its stages before anything runs: no device, no stage)
        std::fprintf(stderr, "graph: %s\n", e.what());
        return 3;
    }
    if (failures) std::printf("spectrum integrator %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("spectrum integrator %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
