// gr::blocks::fft::AdaptiveWeights<float> of the host layer (gr4/blocks.hpp, gr4/hip.hpp): MVDR / Capon weights from the correlator's matrices (ADAPTIVE_WEIGHTS.md).
//   test_host_adaptive_weights host   <libgr4hip_blocks.so> <prefix>   sources -> CrossSpectrum -> AdaptiveWeights -> sink in a host-domain graph; inputs, steering
//                                                                     vectors and output as files for tests/test_adaptive_weights_host.py (which compares them
//                                                                     with the oracle's long-double result under the bound), the settings errors, the chunk
//                                                                     sizes, gr:sample_rate, the C-ABI's refusals, the plugin
//   test_host_adaptive_weights device <libgr4hip_blocks.so> <prefix>   the same graph with AdaptiveWeights on gpu:hip:0 (the seam onto gr4hip_mvdr_process); files for
//                                                                     tests/test_gpu_adaptive_weights.py
// Files: <prefix>.<name> = raw float32 {re, im} pairs; the input is [n_inputs][matrices * n_integrate][vector_size], the steering vectors
// [n_beams][n_inputs][vector_size] (".full") or [n_beams][n_inputs] (".short"), the output [matrices][n_beams][n_inputs][vector_size].
// Exit code 0: everything held; 1: a check failed; 3: a graph failed.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32   = std::complex<float>;
using Cross = blocks::fft::CrossSpectrum<float>;
using Mvdr  = blocks::fft::AdaptiveWeights<float>;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static constexpr std::size_t kMatrices = 2;

struct Lcg {
    std::uint32_t v;
    float next() { v = v * 1664525u + 1013904223u; return static_cast<float>(static_cast<std::int32_t>(v >> 8) % 2001 - 1000) / 1000.f; }
};

// noise in [-1, 1] per stream plus a component every stream shares
static std::vector<std::vector<C32>> streams(std::size_t S, std::size_t n, std::uint32_t seed) {
    Lcg              g{seed};
    std::vector<C32> common(n);
    for (auto& v : common) { const float re = g.next(), im = g.next(); v = C32(re, im); }
    std::vector<std::vector<C32>> x(S, std::vector<C32>(n));
    for (std::size_t s = 0; s < S; ++s) {
        const C32 ph = static_cast<C32>(std::polar(0.7, 0.9 * static_cast<double>(s)));
        for (std::size_t i = 0; i < n; ++i) { const float re = g.next(), im = g.next(); x[s][i] = C32(re, im) + ph * common[i]; }
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
    Mvdr b;
    try { b.applySettings(settings); } catch (const std::invalid_argument&) { return true; }
    return false;
}

static int graph(const std::string& domain, std::size_t B, std::size_t N, std::size_t A, double loading, const std::vector<float>& ar, const std::vector<float>& ai,
                 const std::vector<std::vector<C32>>& x, std::vector<C32>& y, std::vector<Tag>* tags = nullptr) {
    Graph        g;
    property_map cfg{{"n_inputs", std::int64_t(x.size())}, {"n_beams", std::int64_t(B)}, {"vector_size", std::int64_t(N)}, {"steering_real", ar}, {"steering_imag", ai}, {"loading", loading}};
    if (!domain.empty()) cfg["compute_domain"] = domain;
    auto& xc   = g.emplaceBlock<Cross>({{"n_inputs", std::int64_t(x.size())}, {"vector_size", std::int64_t(N)}, {"n_integrate", std::int64_t(A)}, {"mean", true}});
    auto& blk  = g.emplaceBlock<Mvdr>(cfg);
    auto& sink = g.emplaceBlock<testing::VectorSink<C32>>();
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    for (std::size_t s = 0; s < x.size(); ++s) {
        auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
        src.values = x[s];
        if (tags) src._tags = {{0, {{"gr:sample_rate", 48000.f}}}};
        if (!g.connect(src, "out"s, xc, "in#"s + std::to_string(s))) return 2;
    }
    if (!g.connect<"out", "in">(xc, blk)) return 2;
    if (!g.connect<"out", "in">(blk, sink)) return 2;
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (!domain.empty()) EXPECT(blk._device_state != nullptr); // the seam was taken
    y = sink._samples;
    if (tags) *tags = sink._tags;
    return 0;
}

// the matrices straight into the block (no CrossSpectrum in front: a settings tag reaches it with its sample index); a weight set depends on its own matrix and the
// settings only, so with new steering vectors and loading by a tag in front of matrix 2 of 4 the first two sets are those of the old settings and the last two those
// of the new ones, bit for bit -- on the device the steering table and the loading go to the live handle again
static int direct(const std::string& domain, std::size_t S, std::size_t N, const std::vector<C32>& matrices, const std::vector<float>& ar, const std::vector<float>& ai, double loading,
                  const std::vector<Tag>& tags, std::vector<C32>& y) {
    Graph g;
    auto& blk  = g.emplaceBlock<Mvdr>({{"n_inputs", std::int64_t(S)}, {"n_beams", std::int64_t(1)}, {"vector_size", std::int64_t(N)}, {"steering_real", ar}, {"steering_imag", ai}, {"loading", loading},
                                       {"compute_domain", domain}});
    auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
    auto& sink = g.emplaceBlock<testing::VectorSink<C32>>();
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    src.values = matrices;
    src._tags  = tags;
    if (!g.connect<"out", "in">(src, blk) || !g.connect<"out", "in">(blk, sink)) return 2;
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    EXPECT(blk._device_state != nullptr && blk._settings_by_tag == tags.size());
    y = sink._samples;
    return 0;
}
static int new_steering_case() {
    const std::size_t S = 2, N = 16, A = 8, P = S * (S + 1) / 2;
    std::vector<C32>  matrices;
    { // four mean cross-spectral matrices from the host CrossSpectrum
        Graph g;
        auto& xc   = g.emplaceBlock<Cross>({{"n_inputs", std::int64_t(S)}, {"vector_size", std::int64_t(N)}, {"n_integrate", std::int64_t(A)}, {"mean", true}});
        auto& sink = g.emplaceBlock<testing::VectorSink<C32>>();
        const auto x = streams(S, N * A * 4, 57u);
        for (std::size_t s = 0; s < S; ++s) {
            auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
            src.values = x[s];
            if (!g.connect(src, "out"s, xc, "in#"s + std::to_string(s))) return 2;
        }
        if (!g.connect<"out", "in">(xc, sink)) return 2;
        scheduler::Simple sched;
        sched.exchange(std::move(g));
        if (!sched.runAndWait()) return 3;
        matrices = sink._samples;
    }
    EXPECT(matrices.size() == 4 * P * N);
    const std::vector<float> ar1{1.f, 0.f}, ai1{0.f, 1.f}, ar2{0.6f, -0.8f}, ai2{0.8f, 0.6f};
    const std::vector<Tag>   again{{2 * P * N, {{"steering_real", ar2}, {"steering_imag", ai2}, {"loading", 0.01}}}};
    std::vector<C32>         changed, before, after;
    if (int rc = direct("gpu:hip:0", S, N, matrices, ar1, ai1, 0.001, again, changed)) return rc;
    if (int rc = direct("gpu:hip:0", S, N, matrices, ar1, ai1, 0.001, {}, before)) return rc;
    if (int rc = direct("gpu:hip:0", S, N, matrices, ar2, ai2, 0.01, {}, after)) return rc;
    const std::size_t half = 2 * S * N; // two weight sets [1 beam][S][N]
    const bool sizes = changed.size() == 2 * half && before.size() == 2 * half && after.size() == 2 * half;
    EXPECT(sizes);
    if (!sizes) return 0;
    EXPECT(std::memcmp(changed.data(), before.data(), half * sizeof(C32)) == 0 && std::memcmp(changed.data() + half, after.data() + half, half * sizeof(C32)) == 0);
    EXPECT(std::memcmp(before.data() + half, after.data() + half, half * sizeof(C32)) != 0);
    std::printf("steering and loading again on the live handle (by settings in front of matrix 2 of 4): %zu weights, old settings' then new settings'\n", changed.size());
    return 0;
}

static int dumped_cases(const std::string& domain, const std::string& prefix) {
    struct Shape { std::size_t S, B, N, A; double loading; };
    for (const auto& [S, B, N, A, loading] : {Shape{2, 1, 8, 64, 0.0}, Shape{3, 5, 16, 19, 1e-3}, Shape{9, 2, 8, 40, 1e-2}}) {
        for (const bool full : {true, false}) {
            const auto         x = streams(S, N * A * kMatrices, 31u + static_cast<std::uint32_t>(S + B + N));
            Lcg                g{91u + static_cast<std::uint32_t>(S * B)};
            const std::size_t  na = full ? B * S * N : B * S;
            std::vector<float> ar(na), ai(na);
            std::vector<C32>   a(na), y, flat;
            for (std::size_t i = 0; i < na; ++i) { // unit modulus, any phase
                const C32 v = static_cast<C32>(std::polar(1.0, 3.14159265358979323846 * static_cast<double>(g.next())));
                ar[i] = v.real(); ai[i] = v.imag(); a[i] = v;
            }
            if (int rc = graph(domain, B, N, A, loading, ar, ai, x, y)) return rc;
            EXPECT(y.size() == kMatrices * B * S * N);
            for (const auto& row : x) flat.insert(flat.end(), row.begin(), row.end());
            const std::string tag = prefix + ".S" + std::to_string(S) + ".B" + std::to_string(B) + ".N" + std::to_string(N) + (full ? ".full" : ".short");
            dump(tag + ".in", flat);
            dump(tag + ".a", a);
            dump(tag + ".out", y);
        }
    }
    return 0;
}

static int host_checks(PluginLoader& loader, const std::string& prefix) {
    if (int rc = dumped_cases("", prefix)) return rc;
    { // gr:sample_rate leaves scaled by output_chunk_size / input_chunk_size = n_beams n_inputs / P (behind the correlator's P / n_integrate)
        const std::size_t N = 16, S = 2, B = 3, A = 4;
        const auto        x = streams(S, N * A * 2, 5u);
        std::vector<C32>  y;
        std::vector<Tag>  tags;
        if (int rc = graph("", B, N, A, 0.5, std::vector<float>(B * S, 1.f), std::vector<float>(B * S, 0.f), x, y, &tags)) return rc;
        EXPECT(y.size() == 2 * B * S * N);
        EXPECT(tags.size() == 1u);
        if (tags.size() == 1) EXPECT(tags[0].index == 0u && (tags[0].map == property_map{{"gr:sample_rate", 72000.f}})); // 48000 * (3 / 4) * (6 / 3)
    }
    { // the settings errors, the chunk sizes, the reflected members, the defaults
        const std::vector<float> a6(6, 1.f), a5(5, 1.f), a48(48, 1.f);
        EXPECT(throws({{"n_inputs", std::int64_t(1)}}));
        EXPECT(throws({{"n_inputs", std::int64_t(33)}}));
        EXPECT(throws({{"n_beams", std::int64_t(0)}}));
        EXPECT(throws({{"n_beams", std::int64_t(33)}}));
        EXPECT(throws({{"vector_size", std::int64_t(1)}}));
        EXPECT(throws({{"loading", -1.0}}));
        EXPECT(throws({{"loading", std::numeric_limits<double>::infinity()}}));
        EXPECT(throws({{"loading", std::numeric_limits<double>::quiet_NaN()}}));
        EXPECT(throws({{"n_inputs", std::int64_t(3)}}));                                                                                                        // two values for three inputs
        EXPECT(throws({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"steering_real", a6}, {"steering_imag", a5}}));                           // lengths differ
        EXPECT(throws({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(8)}, {"steering_real", a5}, {"steering_imag", a5}})); // neither B S nor B S N
        EXPECT(!throws({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(8)}, {"steering_real", a6}, {"steering_imag", a6}}));
        EXPECT(!throws({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(8)}, {"steering_real", a48}, {"steering_imag", a48}, {"loading", 0.25}}));
        Mvdr b;
        b.applySettings({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(1000)}, {"steering_real", a6}, {"steering_imag", a6}});
        EXPECT(b.input_chunk_size == 6000u && b.output_chunk_size == 6000u && b.nBaselines() == 6u);
        b.applySettings({{"n_inputs", std::int64_t(4)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(100)}, {"steering_real", std::vector<float>(8, 1.f)}, {"steering_imag", std::vector<float>(8, 0.f)}});
        EXPECT(b.input_chunk_size == 1000u && b.output_chunk_size == 800u);
        constexpr auto                        names = Mvdr::gr_member_names();
        const std::array<std::string_view, 8> want{"in", "out", "n_inputs", "n_beams", "vector_size", "steering_real", "steering_imag", "loading"};
        EXPECT(names.size() == want.size());
        for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
        Mvdr d;
        EXPECT(d.n_inputs == 2u && d.n_beams == 1u && d.vector_size == 1024u && d.loading == 0.0 && d.steering_real == (std::vector<float>{1.f, 1.f}));
    }
    { // the C-ABI's refusals that need no device
        gr4hip_mvdr_t* h = nullptr;
        EXPECT(gr4hip_mvdr_create(nullptr, 2, 1, 8) == GR4HIP_INVALID_ARGUMENT);
        EXPECT(gr4hip_mvdr_create(&h, 1, 1, 8) == GR4HIP_INVALID_ARGUMENT && !h);
        EXPECT(gr4hip_mvdr_create(&h, 2, 0, 8) == GR4HIP_INVALID_ARGUMENT && !h);
        EXPECT(gr4hip_mvdr_create(&h, 2, 1, 1) == GR4HIP_INVALID_ARGUMENT && !h);
        EXPECT(gr4hip_mvdr_create(&h, 33, 1, 8) == GR4HIP_UNSUPPORTED && !h);
        EXPECT(gr4hip_mvdr_create(&h, 2, 33, 8) == GR4HIP_UNSUPPORTED && !h);
        EXPECT(gr4hip_mvdr_create(&h, 2, 1, 8) == GR4HIP_OK && h);
        alignas(8) float v[128] = {};
        EXPECT(gr4hip_mvdr_process(h, v, 1, v + 64, nullptr, nullptr) == GR4HIP_INVALID_ARGUMENT); // no steering vectors yet
        EXPECT(gr4hip_mvdr_process(h, v, 0, v + 64, nullptr, nullptr) == GR4HIP_OK);               // no matrices: a no-op
        EXPECT(gr4hip_mvdr_process(nullptr, v, 1, v + 64, nullptr, nullptr) == GR4HIP_INVALID_ARGUMENT);
        EXPECT(gr4hip_mvdr_set_steering(h, nullptr, nullptr) == GR4HIP_INVALID_ARGUMENT);
        EXPECT(gr4hip_mvdr_set_loading(h, -0.5) == GR4HIP_INVALID_ARGUMENT && gr4hip_mvdr_set_loading(h, 0.5) == GR4HIP_OK);
        EXPECT(gr4hip_mvdr_destroy(h) == GR4HIP_OK);
    }
    { // the plugin knows the block under its portable type name
        const std::string n = "gr::blocks::fft::AdaptiveWeights<float32>";
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(64)}, {"steering_real", std::vector<float>(6, 1.f)},
                                      {"steering_imag", std::vector<float>(6, 0.f)}}) != nullptr);
        std::printf("plugin: %s %s\n", n.c_str(), loader.isBlockAvailable(n) ? "available" : "MISSING");
        EXPECT(!loader.isBlockAvailable("gr::blocks::fft::AdaptiveWeights<float64>")); // float64 visibilities are out of scope
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
        if (int rc = mode == "device" ? new_steering_case() : 0) return rc;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "graph: %s\n", e.what());
        return 3;
    }
    if (failures) std::printf("adaptive weights %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("adaptive weights %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
