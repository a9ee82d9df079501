// gr::blocks::fft::InverseFFT / PfbSynthesizer of the host layer (gr4/blocks.hpp, gr4/hip.hpp): the inverse transform and the polyphase synthesis bank (INVERSE_FFT.md).
//   test_host_ifft host   <libgr4hip_blocks.so> <prefix>   the CPU bodies' outputs as files for tests/test_ifft_host.py (which compares them with the float64 oracle), the
//                                                          settings errors, the history across settings changes, the plugin registration
//   test_host_ifft device <libgr4hip_blocks.so> <prefix>   source -> PfbChannelizer -> PfbSynthesizer -> sink on gpu:hip:0 as a hip::plan run against the CPU graph, and
//                                                          source -> InverseFFT -> sink behind the compute_domain seam; outputs as files for tests/test_gpu_ifft.py
// Files: <prefix>.<name> = raw float32 (complex values as {re, im} pairs).  Exit code 0: everything held; 1: a check failed; 3: a graph failed.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32   = std::complex<float>;
using Inv   = blocks::fft::InverseFFT<C32>;
using InvR  = blocks::fft::InverseFFT<float>;
using Synth = blocks::fft::PfbSynthesizer<C32>;
using Chan  = blocks::fft::PfbChannelizer<C32>;

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
    // the bodies: files for the oracle comparison
    for (const std::size_t N : {std::size_t(8), std::size_t(64)}) {
        const auto        x   = stream(N * 9, 5u + static_cast<std::uint32_t>(N));
        const std::string tag = prefix + ".N" + std::to_string(N);
        dump(tag + ".in", x);
        Inv  c, cs;
        InvR r;
        c.applySettings({{"fftSize", std::int64_t(N)}});
        cs.applySettings({{"fftSize", std::int64_t(N)}, {"window", "Hann"s}, {"scale", true}});
        r.applySettings({{"fftSize", std::int64_t(N)}});
        EXPECT(c.input_chunk_size == N && c.output_chunk_size == N && r.input_chunk_size == N && r.output_chunk_size == N);
        dump(tag + ".c2c", body(c, x));
        dump(tag + ".c2c.hann.scaled", body(cs, x));
        dump(tag + ".c2r", body(r, x));
        for (const std::size_t P : {std::size_t(1), std::size_t(3)}) {
            Synth s;
            s.applySettings({{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}});
            EXPECT(s.input_chunk_size == N && s.output_chunk_size == N);
            const auto y = body(s, x);
            dump(tag + ".P" + std::to_string(P) + ".synth", y);
            // frame by frame is the same stream; reset brings the zeros back
            Synth s2;
            s2.applySettings({{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}});
            std::vector<C32> y2(x.size());
            for (std::size_t m = 0; m < x.size() / N; ++m) EXPECT(s2.processBulk(std::span<const C32>(x.data() + m * N, N), std::span<C32>(y2.data() + m * N, N)) == work::Status::OK);
            EXPECT(y2 == y);
            s2.reset();
            EXPECT(body(s2, x) == y);
        }
    }
    { // the history across settings changes: new taps keep it, another fftSize or taps_per_channel clears it
        const std::size_t N = 32, P = 4;
        const auto        x = stream(N * 12, 3u);
        std::vector<float> g2(N * P);
        for (std::size_t j = 0; j < g2.size(); ++j) g2[j] = static_cast<float>(std::sin(0.37 * static_cast<double>(j + 1))) / static_cast<float>(P);
        const std::vector<C32> a(x.begin(), x.begin() + 5 * N), b(x.begin() + 5 * N, x.begin() + 9 * N), c(x.begin() + 9 * N, x.end());
        Synth blk;
        blk.applySettings({{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}});
        dump(prefix + ".hist.a.in", a);
        dump(prefix + ".hist.a.synth", body(blk, a));
        blk.applySettings({{"taps", g2}}); // taps alone: frames of b see the end of a
        EXPECT(blk._hist.size() == (P - 1) * N && blk._hist.back() != C32{});
        dump(prefix + ".hist.taps", g2);
        dump(prefix + ".hist.b.in", b);
        dump(prefix + ".hist.b.synth", body(blk, b));
        blk.applySettings({{"taps", std::vector<float>{}}, {"taps_per_channel", std::int64_t(2)}}); // another P (designed again): zeros in front of c
        EXPECT(blk._hist.size() == N && std::all_of(blk._hist.begin(), blk._hist.end(), [](C32 v) { return v == C32{}; }));
        dump(prefix + ".hist.c.in", c);
        dump(prefix + ".hist.c.synth", body(blk, c));
        blk.applySettings({{"fftSize", std::int64_t(2 * N)}}); // another fftSize: cleared too
        EXPECT(blk._hist.size() == 2 * N && std::all_of(blk._hist.begin(), blk._hist.end(), [](C32 v) { return v == C32{}; }));
    }
    { // every bad setting throws; the reflected members; the defaults
        const auto bad_size = [](auto tag) {
            using B = typename decltype(tag)::type;
            EXPECT(throws<B>({{"fftSize", std::int64_t(1000)}}));
            EXPECT(throws<B>({{"fftSize", std::int64_t(16384)}}));
            EXPECT(throws<B>({{"fftSize", std::int64_t(1)}}));
            EXPECT(throws<B>({{"fftSize", std::int64_t(0)}}));
            EXPECT(throws<B>({{"window", "NoSuchWindow"s}}));
            EXPECT(!throws<B>({{"fftSize", std::int64_t(8192)}, {"window", "Kaiser"s}, {"scale", true}}));
        };
        bad_size(std::type_identity<Inv>{});
        bad_size(std::type_identity<InvR>{});
        bad_size(std::type_identity<Synth>{});
        EXPECT(throws<Synth>({{"taps_per_channel", std::int64_t(0)}}));
        EXPECT(throws<Synth>({{"taps_per_channel", std::int64_t(33)}}));
        EXPECT(throws<Synth>({{"fftSize", std::int64_t(16)}, {"taps_per_channel", std::int64_t(2)}, {"taps", std::vector<float>(31, 1.f)}}));
        EXPECT(throws<Synth>({{"fftSize", std::int64_t(16)}, {"taps_per_channel", std::int64_t(2)}, {"taps", std::vector<float>(33, 1.f)}}));
        EXPECT(!throws<Synth>({{"fftSize", std::int64_t(16)}, {"taps_per_channel", std::int64_t(2)}, {"taps", std::vector<float>(32, 1.f)}}));
        {
            constexpr auto                        names = Inv::gr_member_names();
            const std::array<std::string_view, 5> want{"in", "out", "fftSize", "window", "scale"};
            EXPECT(names.size() == want.size());
            for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
            Inv d;
            EXPECT(d.fftSize == 1024u && d.window == "None" && !d.scale);
        }
        {
            constexpr auto                        names = Synth::gr_member_names();
            const std::array<std::string_view, 7> want{"in", "out", "fftSize", "taps_per_channel", "taps", "window", "scale"};
            EXPECT(names.size() == want.size());
            for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
            Synth d;
            EXPECT(d.fftSize == 1024u && d.taps_per_channel == 4u && d.taps.empty() && d.window == "Hamming" && !d.scale);
        }
    }
    { // the plugin knows the three blocks under their portable type names
        for (const std::string n : {"gr::blocks::fft::InverseFFT<complex<float32>>", "gr::blocks::fft::InverseFFT<float32>", "gr::blocks::fft::PfbSynthesizer<complex<float32>>"}) {
            EXPECT(loader.isBlockAvailable(n));
            EXPECT(loader.instantiate(n, {{"fftSize", std::int64_t(64)}}) != nullptr);
            std::printf("plugin: %s %s\n", n.c_str(), loader.isBlockAvailable(n) ? "available" : "MISSING");
        }
        EXPECT(!loader.isBlockAvailable("gr::blocks::fft::PfbSynthesizer<float32>")); // complex streams only
    }
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

// source -> PfbChannelizer -> PfbSynthesizer -> sink; domain "" = host, otherwise a planned run of the two stages
static int run_bank_graph(std::size_t N, std::size_t P, const std::vector<C32>& x, const std::string& domain, std::vector<C32>& y) {
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
    src.values = x;
    property_map cfg{{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}};
    property_map syn{{"fftSize", std::int64_t(N)}, {"taps_per_channel", std::int64_t(P)}, {"scale", true}};
    if (!domain.empty()) cfg["compute_domain"] = syn["compute_domain"] = domain;
    auto& ana  = g.emplaceBlock<Chan>(cfg);
    auto& bank = g.emplaceBlock<Synth>(syn);
    ana._log = bank._log = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<C32>>();
    if (!g.connect<"out", "in">(src, ana) || !g.connect<"out", "in">(ana, bank) || !g.connect<"out", "in">(bank, sink)) return 2;
    if (!domain.empty()) {
        const auto runs = hip::plan(g);
        for (auto* r : runs) std::printf("planned run: %zu stage(s): %s\n", r->stages().size(), std::string(r->description()).c_str());
        EXPECT(runs.size() == 1 && runs[0]->stages().size() == 2u);
    }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    y = sink._samples;
    return 0;
}

// source -> InverseFFT<T> -> sink; domain "" = host, otherwise the block's own work() behind the seam
template <typename B>
static int run_ifft_graph(std::size_t N, const std::vector<C32>& x, const std::string& domain, std::vector<typename std::decay_t<decltype(B{}.out)>::value_type>& y) {
    using TOut = typename std::decay_t<decltype(B{}.out)>::value_type;
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
    src.values = x;
    property_map cfg{{"fftSize", std::int64_t(N)}, {"window", "Hann"s}, {"scale", true}};
    if (!domain.empty()) cfg["compute_domain"] = domain;
    auto& blk  = g.emplaceBlock<B>(cfg);
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<TOut>>();
    if (!g.connect<"out", "in">(src, blk) || !g.connect<"out", "in">(blk, sink)) return 2;
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (!domain.empty()) EXPECT(blk._device_state != nullptr); // the seam was taken
    y = sink._samples;
    return 0;
}

static int device_checks(const std::string& prefix) {
    const std::string dom = "gpu:hip:0";
    const std::size_t N = 256, P = 4, M = 40;
    const auto        x = stream(N * M, 77u);
    dump(prefix + ".in", x);
    std::vector<C32> hb, pb, hc, dc;
    std::vector<float> hr, dr;
    if (int rc = run_bank_graph(N, P, x, "", hb)) return rc;
    if (int rc = run_bank_graph(N, P, x, dom, pb)) return rc;
    if (int rc = run_ifft_graph<Inv>(N, x, "", hc)) return rc;
    if (int rc = run_ifft_graph<Inv>(N, x, dom, dc)) return rc;
    if (int rc = run_ifft_graph<InvR>(N, x, "", hr)) return rc;
    if (int rc = run_ifft_graph<InvR>(N, x, dom, dr)) return rc;
    dump(prefix + ".bank.host", hb);
    dump(prefix + ".bank.planned", pb);
    dump(prefix + ".c2c.seam", dc);
    dump(prefix + ".c2r.seam", dr);
    const double e[3] = {max_rel(pb, hb), max_rel(dc, hc), max_rel(dr, hr)};
    std::printf("device against the host body: analysis -> synthesis planned %.3g, inverse transform seam %.3g, complex-to-real seam %.3g\n", e[0], e[1], e[2]);
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
    if (failures) std::printf("ifft %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("ifft %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
