// gr::blocks::fft::PfbPowerSpectrum / PfbChannelizer of the host layer (gr4/blocks.hpp, gr4/hip.hpp): the polyphase filter bank in front of the transform (PFB.md).
//   test_host_pfb host   <libgr4hip_blocks.so> <prefix>   the CPU bodies' outputs as files for tests/test_pfb_host.py (which compares them with the float64 oracle), the
//                                                         settings errors, the history across settings changes, the plugin registration
//   test_host_pfb device <libgr4hip_blocks.so> <prefix>   source -> block -> sink on gpu:hip:0, alone (the compute_domain seam) and as a hip::plan run; outputs as files
//                                                         for tests/test_gpu_pfb.py (which compares them with the C-ABI's)
// Files: <prefix>.<name> = raw float32 (complex values as {re, im} pairs).  Exit code 0: everything held; 1: a check failed; 3: a graph failed.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32  = std::complex<float>;
using Spec = blocks::fft::PfbPowerSpectrum<C32>;
using Chan = blocks::fft::PfbChannelizer<C32>;

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
template <typename B>
static bool throws(const property_map& settings) {
    B b;
    try { b.applySettings(settings); } catch (const std::invalid_argument&) { return true; }
    return false;
}

template <typename B>
static std::vector<typename std::decay_t<decltype(B{}.out)>::value_type> body(B& b, const std::vector<C32>& x) {
    std::vector<typename std::decay_t<decltype(B{}.out)>::value_type> y(x.size());
    EXPECT(b.processBulk(std::span<const C32>(x), std::span(y)) == work::Status::OK);
    return y;
}

static int host_checks(PluginLoader& loader, const std::string& prefix) {
    // the bodies on designed (Hamming) prototypes: files for the oracle comparison
    for (const auto& [N, P] : {std::pair<std::size_t, std::size_t>{8, 1}, {16, 3}, {64, 4}, {256, 8}}) {
        const auto        x   = stream(N * (P + 6), 11u + static_cast<std::uint32_t>(N));
        const std::string tag = prefix + ".N" + std::to_string(N) + ".P" + std::to_string(P);
        Spec s;
        Chan c;
        s.applySettings({{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}});
        c.applySettings({{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}});
        EXPECT(s.input_chunk_size == N && s.output_chunk_size == N && c.input_chunk_size == N && c.output_chunk_size == N);
        dump(tag + ".in", x);
        const auto ys = body(s, x);
        const auto yc = body(c, x);
        dump(tag + ".mag2", ys);
        dump(tag + ".spec", yc);
        bool same = ys.size() == yc.size(); // both blocks run one front end and one transform
        for (std::size_t i = 0; same && i < ys.size(); ++i) same = std::abs(ys[i] - std::norm(yc[i])) <= 1e-5f * ys[i] + 1e-30f;
        EXPECT(same);
        // frame by frame is the same stream; reset brings the zeros back
        Chan c2;
        c2.applySettings({{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}});
        std::vector<C32> y2(x.size());
        for (std::size_t m = 0; m < x.size() / N; ++m) EXPECT(c2.processBulk(std::span<const C32>(x.data() + m * N, N), std::span<C32>(y2.data() + m * N, N)) == work::Status::OK);
        EXPECT(y2 == yc);
        c2.reset();
        EXPECT(body(c2, x) == yc);
    }
    { // the history across settings changes: new taps keep it, another fftSize or taps_per_channel clears it
        const std::size_t N = 32, P = 4;
        const auto        x = stream(N * 12, 3u);
        std::vector<float> h2(N * P);
        for (std::size_t j = 0; j < h2.size(); ++j) h2[j] = static_cast<float>(std::sin(0.37 * static_cast<double>(j + 1))) / static_cast<float>(P);
        const std::vector<C32> a(x.begin(), x.begin() + 5 * N), b(x.begin() + 5 * N, x.begin() + 9 * N), c(x.begin() + 9 * N, x.end());
        Chan blk;
        blk.applySettings({{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}});
        dump(prefix + ".hist.a.in", a);
        dump(prefix + ".hist.a.spec", body(blk, a));
        blk.applySettings({{"taps", h2}}); // taps alone: frames of b see the end of a
        EXPECT(blk._core.hist.size() == (P - 1) * N && blk._core.hist.back() == a.back());
        dump(prefix + ".hist.taps", h2);
        dump(prefix + ".hist.b.in", b);
        dump(prefix + ".hist.b.spec", body(blk, b));
        blk.applySettings({{"taps", std::vector<float>{}}, {"taps_per_channel", std::int64_t(2)}}); // another P (designed again): zeros in front of c
        EXPECT(blk._core.hist.size() == N && blk._core.hist.back() == C32{});
        dump(prefix + ".hist.c.in", c);
        dump(prefix + ".hist.c.spec", body(blk, c));
        (void)body(blk, c);
        blk.applySettings({{"fftSize", std::int64_t(2 * N)}}); // another fftSize: cleared too
        EXPECT(blk._core.hist.size() == 2 * N && std::all_of(blk._core.hist.begin(), blk._core.hist.end(), [](C32 v) { return v == C32{}; }));
    }
    { // every bad setting throws, in both blocks; the reflected members; the defaults
        const auto bad = [](auto tag) {
            using B = typename decltype(tag)::type;
            EXPECT(throws<B>({{"fftSize", std::int64_t(1000)}}));
            EXPECT(throws<B>({{"fftSize", std::int64_t(1)}}));
            EXPECT(throws<B>({{"fftSize", std::int64_t(0)}}));
            EXPECT(throws<B>({{"taps_per_channel", std::int64_t(0)}}));
            EXPECT(throws<B>({{"taps_per_channel", std::int64_t(33)}}));
            EXPECT(throws<B>({{"fftSize", std::int64_t(16)}, {"taps_per_channel", std::int64_t(2)}, {"taps", std::vector<float>(31, 1.f)}}));
            EXPECT(throws<B>({{"fftSize", std::int64_t(16)}, {"taps_per_channel", std::int64_t(2)}, {"taps", std::vector<float>(33, 1.f)}}));
            EXPECT(throws<B>({{"window", "NoSuchWindow"s}}));
            EXPECT(!throws<B>({{"fftSize", std::int64_t(16)}, {"taps_per_channel", std::int64_t(2)}, {"taps", std::vector<float>(32, 1.f)}}));
            EXPECT(!throws<B>({{"fftSize", std::int64_t(8192)}, {"taps_per_channel", std::int64_t(32)}, {"window", "Kaiser"s}}));
            constexpr auto                        names = B::gr_member_names();
            const std::array<std::string_view, 6> want{"in", "out", "fftSize", "taps_per_channel", "taps", "window"};
            EXPECT(names.size() == want.size());
            for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
            B d;
            EXPECT(d.fftSize == 1024u && d.taps_per_channel == 4u && d.taps.empty() && d.window == "Hamming");
        };
        bad(std::type_identity<Spec>{});
        bad(std::type_identity<Chan>{});
    }
    { // the plugin knows both blocks under their portable type names
        for (const std::string n : {"gr::blocks::fft::PfbPowerSpectrum<complex<float32>>", "gr::blocks::fft::PfbChannelizer<complex<float32>>"}) {
            EXPECT(loader.isBlockAvailable(n));
            EXPECT(loader.instantiate(n, {{"fftSize", std::int64_t(64)}, {"taps_per_channel", std::int64_t(3)}}) != nullptr);
            std::printf("plugin: %s %s\n", n.c_str(), loader.isBlockAvailable(n) ? "available" : "MISSING");
        }
        EXPECT(!loader.isBlockAvailable("gr::blocks::fft::PfbPowerSpectrum<float32>")); // complex streams only
    }
    return 0;
}

// source -> block -> sink; domain "" = host
template <typename B>
static int run_graph(std::size_t N, std::size_t P, const std::vector<C32>& x, const std::string& domain, bool planned, std::vector<typename std::decay_t<decltype(B{}.out)>::value_type>& y) {
    using TOut = typename std::decay_t<decltype(B{}.out)>::value_type;
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
    src.values = x;
    property_map cfg{{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}};
    if (!domain.empty()) cfg["compute_domain"] = domain;
    auto& blk  = g.emplaceBlock<B>(cfg);
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<TOut>>();
    if (!g.connect<"out", "in">(src, blk) || !g.connect<"out", "in">(blk, sink)) return 2;
    if (planned) {
        const auto runs = hip::plan(g, 1); // (alone: a run of one stage)
        for (auto* r : runs) std::printf("planned run: %zu stage(s): %s\n", r->stages().size(), std::string(r->description()).c_str());
        EXPECT(runs.size() == 1 && runs[0]->stages().size() == 1u);
    }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (!domain.empty() && !planned) EXPECT(blk._device_state != nullptr); // the seam was taken
    y = sink._samples;
    return 0;
}

template <typename T>
static double max_rel(const std::vector<T>& got, const std::vector<T>& want) { // max |got - want| / max(|want|, rms(want))
    if (got.size() != want.size() || want.empty()) return 1e30;
    double rms = 0;
    for (const auto& v : want) rms += std::norm(std::complex<double>(v));
    rms = std::sqrt(rms / double(want.size()));
    double worst = 0;
    for (std::size_t i = 0; i < want.size(); ++i) worst = std::max(worst, std::abs(std::complex<double>(got[i]) - std::complex<double>(want[i])) / std::max(std::abs(std::complex<double>(want[i])), rms));
    return worst;
}

static int device_checks(const std::string& prefix) {
    const std::string dom = "gpu:hip:0";
    const std::size_t N = 256, P = 4, M = 40;
    const auto        x = stream(N * M, 77u);
    dump(prefix + ".in", x);
    std::vector<float> hm, dm, pm;
    if (int rc = run_graph<Spec>(N, P, x, "", false, hm)) return rc;
    if (int rc = run_graph<Spec>(N, P, x, dom, false, dm)) return rc; // the block's own work() behind the seam
    if (int rc = run_graph<Spec>(N, P, x, dom, true, pm)) return rc;  // a planned run of one stage
    std::vector<C32> hs, ds, ps;
    if (int rc = run_graph<Chan>(N, P, x, "", false, hs)) return rc;
    if (int rc = run_graph<Chan>(N, P, x, dom, false, ds)) return rc;
    if (int rc = run_graph<Chan>(N, P, x, dom, true, ps)) return rc;
    dump(prefix + ".mag2.seam", dm);
    dump(prefix + ".mag2.planned", pm);
    dump(prefix + ".spec.seam", ds);
    dump(prefix + ".spec.planned", ps);
    const double e[4] = {max_rel(dm, hm), max_rel(pm, hm), max_rel(ds, hs), max_rel(ps, hs)};
    std::printf("device against the host body: |X|^2 seam %.3g planned %.3g, spectrum seam %.3g planned %.3g\n", e[0], e[1], e[2], e[3]);
    for (double v : e) EXPECT(v <= 1e-5);
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
    if (failures) std::printf("pfb %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("pfb %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
