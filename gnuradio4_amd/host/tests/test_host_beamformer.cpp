// gr::blocks::fft::Beamformer<float> of the host layer (gr4/blocks.hpp, gr4/hip.hpp): the per-bin weighted sum of n_inputs spectra into n_beams beams (BEAMFORMER.md).
//   test_host_beamformer host   <libgr4hip_blocks.so> <prefix>   sources -> Beamformer -> sink in a host-domain graph; inputs, weights and output as files for
//                                                               tests/test_beamformer_host.py (which compares them bit for bit with the oracle's ordered
//                                                               definition), the settings errors, the chunk sizes, gr:sample_rate, the plugin
//   test_host_beamformer device <libgr4hip_blocks.so> <prefix>   the same graph with the block on gpu:hip:0 (the seam onto gr4hip_beamform_process); files for
//                                                               tests/test_gpu_beamformer.py
// Files: <prefix>.<name> = raw float32 {re, im} pairs; the input is [n_inputs][frames][vector_size], the weights [n_beams][n_inputs][vector_size] (".full") or
// [n_beams][n_inputs] (".short"), the output [frames][n_beams][vector_size].  Exit code 0: everything held; 1: a check failed; 3: a graph failed.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32  = std::complex<float>;
using Beam = blocks::fft::Beamformer<float>;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static constexpr std::size_t kFrames = 7;

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
    Beam b;
    try { b.applySettings(settings); } catch (const std::invalid_argument&) { return true; }
    return false;
}

static int graph(const std::string& domain, std::size_t B, std::size_t N, const std::vector<float>& wr, const std::vector<float>& wi, const std::vector<std::vector<C32>>& x,
                 std::vector<C32>& y, std::vector<Tag>* tags = nullptr, const std::vector<Tag>& settings_tags = {}) {
    Graph        g;
    property_map cfg{{"n_inputs", std::int64_t(x.size())}, {"n_beams", std::int64_t(B)}, {"vector_size", std::int64_t(N)}, {"weights_real", wr}, {"weights_imag", wi}};
    if (!domain.empty()) cfg["compute_domain"] = domain;
    auto& blk  = g.emplaceBlock<Beam>(cfg);
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
    struct Shape { std::size_t S, B, N; };
    for (const auto& [S, B, N] : {Shape{1, 1, 8}, Shape{3, 5, 16}, Shape{9, 2, 8}}) {
        for (const bool full : {true, false}) {
            const auto         x = streams(S, N * kFrames, 23u + static_cast<std::uint32_t>(S + B + N));
            Lcg                g{77u + static_cast<std::uint32_t>(S * B)};
            const std::size_t  nw = full ? B * S * N : B * S;
            std::vector<float> wr(nw), wi(nw);
            std::vector<C32>   w(nw), y, flat;
            for (std::size_t i = 0; i < nw; ++i) { wr[i] = g.next(); wi[i] = g.next(); w[i] = C32(wr[i], wi[i]); }
            if (int rc = graph(domain, B, N, wr, wi, x, y)) return rc;
            EXPECT(y.size() == kFrames * B * N);
            for (const auto& row : x) flat.insert(flat.end(), row.begin(), row.end());
            const std::string tag = prefix + ".S" + std::to_string(S) + ".B" + std::to_string(B) + ".N" + std::to_string(N) + (full ? ".full" : ".short");
            dump(tag + ".in", flat);
            dump(tag + ".w", w);
            dump(tag + ".out", y);
        }
    }
    return 0;
}

// S = 2, one beam, vector_size 16: two frames, then new weights by settings, then two frames.  The seam keeps its handle (the shape is the same) and sends the
// weights to the device again.  Device against the host body: both are the ordered definition, bit for bit.
static int new_weights_case() {
    const std::size_t      N = 16;
    const auto             x = streams(2, N * 4, 31u);
    const std::vector<Tag> reweigh{{N * 2, {{"weights_real", std::vector<float>{-0.25f, 0.75f}}, {"weights_imag", std::vector<float>{0.5f, -1.f}}}}};
    std::vector<C32>       dev, host, unchanged;
    if (int rc = graph("gpu:hip:0", 1, N, {0.5f, 0.5f}, {0.f, 0.25f}, x, dev, nullptr, reweigh)) return rc;
    if (int rc = graph("", 1, N, {0.5f, 0.5f}, {0.f, 0.25f}, x, host, nullptr, reweigh)) return rc;
    if (int rc = graph("", 1, N, {0.5f, 0.5f}, {0.f, 0.25f}, x, unchanged)) return rc;
    EXPECT(host.size() == 4 * N && dev.size() == host.size() && std::memcmp(dev.data(), host.data(), host.size() * sizeof(C32)) == 0);
    EXPECT(unchanged.size() == host.size() && std::equal(host.begin(), host.begin() + 2 * N, unchanged.begin()) && !std::equal(host.begin() + 2 * N, host.end(), unchanged.begin() + 2 * N));
    std::printf("weights again with the handle kept (new weights by settings): %zu values, device == host\n", dev.size());
    return 0;
}

static int host_checks(PluginLoader& loader, const std::string& prefix) {
    if (int rc = dumped_cases("", prefix)) return rc;
    { // gr:sample_rate leaves scaled by output_chunk_size / input_chunk_size = n_beams
        const std::size_t             N = 16, S = 2, B = 3;
        std::vector<std::vector<C32>> x(S, std::vector<C32>(N * 4, C32(1.f, 0.f)));
        std::vector<C32>              y;
        std::vector<Tag>              tags;
        if (int rc = graph("", B, N, std::vector<float>(B * S, 0.5f), std::vector<float>(B * S, 0.f), x, y, &tags)) return rc;
        EXPECT(y.size() == 4 * B * N && y[0] == C32(1.f, 0.f) && y[B * N] == C32(1.f, 0.f));
        EXPECT(tags.size() == 1u);
        if (tags.size() == 1) EXPECT(tags[0].index == 0u && (tags[0].map == property_map{{"gr:sample_rate", 144000.f}}));
    }
    { // the settings errors, the chunk sizes, the reflected members, the defaults
        const std::vector<float> w6(6, 1.f), w5(5, 1.f), w48(48, 1.f);
        EXPECT(throws({{"n_inputs", std::int64_t(0)}}));
        EXPECT(throws({{"n_inputs", std::int64_t(33)}}));
        EXPECT(throws({{"n_beams", std::int64_t(0)}}));
        EXPECT(throws({{"n_beams", std::int64_t(33)}}));
        EXPECT(throws({{"vector_size", std::int64_t(1)}}));
        EXPECT(throws({{"n_inputs", std::int64_t(3)}}));                                                                                                      // two weights for three inputs
        EXPECT(throws({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"weights_real", w6}, {"weights_imag", w5}}));                           // lengths differ
        EXPECT(throws({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(8)}, {"weights_real", w5}, {"weights_imag", w5}})); // neither B S nor B S N
        EXPECT(!throws({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(8)}, {"weights_real", w6}, {"weights_imag", w6}}));
        EXPECT(!throws({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(8)}, {"weights_real", w48}, {"weights_imag", w48}}));
        Beam b;
        b.applySettings({{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(1000)}, {"weights_real", w6}, {"weights_imag", w6}});
        EXPECT(b.input_chunk_size == 1000u && b.output_chunk_size == 2000u && b.in.size() == 3u);
        constexpr auto                        names = Beam::gr_member_names();
        const std::array<std::string_view, 7> want{"in", "out", "n_inputs", "n_beams", "vector_size", "weights_real", "weights_imag"};
        EXPECT(names.size() == want.size());
        for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
        Beam d;
        EXPECT(d.n_inputs == 2u && d.n_beams == 1u && d.vector_size == 1024u && d.in.size() == 2u && d.weights_real == (std::vector<float>{0.5f, 0.5f}));
    }
    { // the C-ABI's refusals that need no device
        gr4hip_beamform_t* h = nullptr;
        EXPECT(gr4hip_beamform_create(nullptr, 2, 1, 8) == GR4HIP_INVALID_ARGUMENT);
        EXPECT(gr4hip_beamform_create(&h, 0, 1, 8) == GR4HIP_INVALID_ARGUMENT && !h);
        EXPECT(gr4hip_beamform_create(&h, 2, 0, 8) == GR4HIP_INVALID_ARGUMENT && !h);
        EXPECT(gr4hip_beamform_create(&h, 2, 1, 1) == GR4HIP_INVALID_ARGUMENT && !h);
        EXPECT(gr4hip_beamform_create(&h, 33, 1, 8) == GR4HIP_UNSUPPORTED && !h);
        EXPECT(gr4hip_beamform_create(&h, 2, 33, 8) == GR4HIP_UNSUPPORTED && !h);
        EXPECT(gr4hip_beamform_create(&h, 2, 1, 8) == GR4HIP_OK && h);
        float        v[32] = {};
        const float* ins[2] = {v, v};
        float*       outs[1] = {v + 16};
        EXPECT(gr4hip_beamform_process(h, ins, 1, outs, 8, nullptr) == GR4HIP_INVALID_ARGUMENT); // no weights yet
        EXPECT(gr4hip_beamform_process(h, ins, 0, outs, 8, nullptr) == GR4HIP_OK);               // no frames: a no-op
        EXPECT(gr4hip_beamform_process(nullptr, ins, 1, outs, 8, nullptr) == GR4HIP_INVALID_ARGUMENT);
        EXPECT(gr4hip_beamform_set_weights(h, nullptr, nullptr) == GR4HIP_INVALID_ARGUMENT);
        EXPECT(gr4hip_beamform_destroy(h) == GR4HIP_OK);
    }
    { // the plugin knows the block under its portable type name
        const std::string n = "gr::blocks::fft::Beamformer<float32>";
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"n_inputs", std::int64_t(3)}, {"n_beams", std::int64_t(2)}, {"vector_size", std::int64_t(64)}, {"weights_real", std::vector<float>(6, 1.f)},
                                      {"weights_imag", std::vector<float>(6, 0.f)}}) != nullptr);
        std::printf("plugin: %s %s\n", n.c_str(), loader.isBlockAvailable(n) ? "available" : "MISSING");
        EXPECT(!loader.isBlockAvailable("gr::blocks::fft::Beamformer<float64>")); // float64 spectra are out of scope
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
        if (int rc = mode == "device" ? new_weights_case() : 0) return rc;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "graph: %s\n", e.what());
        return 3;
    }
    if (failures) std::printf("beamformer %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("beamformer %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
