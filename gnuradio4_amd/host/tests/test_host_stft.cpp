// The `stride` setting of the host layer (gr4/core.hpp Block::stride / strideCounter, gr4/hip.hpp StftPowerStage; OVERLAPPED_FFT.md) on gr::blocks::fft::PowerSpectrum.
//   test_host_stft host   <libgr4hip_blocks.so> <prefix>   source -> PowerSpectrum{fftSize 64, stride 0 | 32 | 64 | 67} -> sink on the CPU path, from a source that
//                                                          delivers everything at once and from one that delivers 1, 7 and then many samples per call; outputs as
//                                                          files for tests/test_stft_host.py (which compares them with the frames by the definition)
//   test_host_stft device <libgr4hip_blocks.so> <prefix>   the same graphs on gpu:hip:0, planned and unplanned, against the CPU path; the same graph from YAML with
//                                                          `stride:` through the plugin; outputs as files for tests/test_gpu_stft.py
// Files: <prefix>.<name> = raw float32 (complex values as {re, im} pairs).  Exit code 0: everything held; 1: a check failed; 3: a graph failed.
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/grc.hpp>
#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32  = std::complex<float>;
using Spec = blocks::fft::PowerSpectrum<C32>;

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

// a source that delivers 1, then 7, then up to `many` samples per call
struct PacedSource : Block<PacedSource> {
    PortOut<C32>     out;
    std::vector<C32> values{};
    Size_t           many = 1000;
    std::size_t      _produced = 0, _call = 0;
    GR_MAKE_REFLECTABLE(PacedSource, out, values, many);

    work::Result customWork(std::size_t requested) {
        if (_produced >= values.size()) return {requested, 0, work::Status::DONE};
        if (!out.connected()) return {requested, 0, work::Status::ERROR};
        const std::size_t want = _call == 0 ? 1 : _call == 1 ? 7 : many;
        const std::size_t n    = std::min({want, values.size() - _produced, out.buffer->free_space(), requested});
        if (n == 0) return {requested, 0, work::Status::INSUFFICIENT_OUTPUT_ITEMS};
        auto span = out.buffer->write_span(n);
        std::copy_n(values.begin() + static_cast<std::ptrdiff_t>(_produced), n, span.begin());
        out.buffer->publish(n);
        _produced += n;
        ++_call;
        if (_produced >= values.size()) out.buffer->producer_done = true;
        return {requested, n, work::Status::OK};
    }
};

// source -> PowerSpectrum -> sink; stride < 0: the setting is not given at all; domain "" = host
static int run_graph(std::size_t N, long stride, const std::vector<C32>& x, const std::string& domain, bool planned, bool paced, std::vector<float>& y) {
    Graph        g;
    property_map cfg{{"fftSize", std::int64_t(N)}, {"window", "Hann"s}};
    if (stride >= 0) cfg["stride"] = std::int64_t(stride);
    if (!domain.empty()) cfg["compute_domain"] = domain;
    auto& blk  = g.emplaceBlock<Spec>(cfg);
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<float>>();
    bool  ok   = static_cast<bool>(g.connect<"out", "in">(blk, sink));
    if (paced) {
        auto& src  = g.emplaceBlock<PacedSource>();
        src.values = x;
        ok         = ok && static_cast<bool>(g.connect<"out", "in">(src, blk));
    } else {
        auto& src  = g.emplaceBlock<testing::VectorSource<C32>>();
        src.values = x;
        ok         = ok && static_cast<bool>(g.connect<"out", "in">(src, blk));
    }
    if (!ok) return 2;
    const bool active = stride > 0 && static_cast<std::size_t>(stride) != N;
    EXPECT(blk.strideActive() == active && blk.strideCounter == 0u);
    if (planned) { // an active stride keeps the block out of fused runs: it runs through its own seam
        const auto runs = hip::plan(g, 1);
        for (auto* r : runs) std::printf("planned run: %zu stage(s): %s\n", r->stages().size(), std::string(r->description()).c_str());
        EXPECT(runs.size() == (active ? 0u : 1u));
    }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (!domain.empty() && (!planned || active)) EXPECT(blk._device_state != nullptr); // the seam was taken
    y = sink._samples;
    return 0;
}

static std::size_t frames_of(std::size_t n, std::size_t N, std::size_t S) { return n < N ? 0 : (n - N) / S + 1; }

static double max_rel(const std::vector<float>& got, const std::vector<float>& want) { // max |got - want| / max(|want|, rms(want))
    if (got.size() != want.size() || want.empty()) return 1e30;
    double rms = 0;
    for (const auto& v : want) rms += double(v) * double(v);
    rms = std::sqrt(rms / double(want.size()));
    double worst = 0;
    for (std::size_t i = 0; i < want.size(); ++i) worst = std::max(worst, std::abs(double(got[i]) - double(want[i])) / std::max(std::abs(double(want[i])), rms));
    return worst;
}

constexpr std::size_t kN = 64;
static const long     kStrides[] = {32, 67, 1, 64, 0};

static int host_checks(PluginLoader& loader, const std::string& prefix) {
    const auto x = stream(20 * kN + 37, 5u); // (a trailing partial frame: EOS drops it)
    dump(prefix + ".in", x);
    std::vector<float> plain;
    if (int rc = run_graph(kN, -1, x, "", false, false, plain)) return rc; // the block without the setting
    EXPECT(plain.size() == (x.size() / kN) * kN);
    for (const long S : kStrides) {
        const std::size_t  eff = S == 0 ? kN : static_cast<std::size_t>(S);
        std::vector<float> once, paced;
        if (int rc = run_graph(kN, S, x, "", false, false, once)) return rc;
        if (int rc = run_graph(kN, S, x, "", false, true, paced)) return rc;
        EXPECT(once.size() == frames_of(x.size(), kN, eff) * kN);
        EXPECT(paced == once); // 1, 7, then many samples per call: the same stream
        if (S == 0 || S == long(kN)) EXPECT(once == plain); // an inactive stride: what the block gives without the setting, value for value
        dump(prefix + ".S" + std::to_string(S) + ".mag2", once);
        std::printf("host: stride %ld -> %zu frames\n", S, once.size() / kN);
    }
    { // the setting itself: every block has it, a new value starts a new stride, a wrong type throws
        Spec b;
        EXPECT(b.stride == 0u && !b.strideActive() && b.hasSetting("stride"));
        b.applySettings({{"fftSize", std::int64_t(64)}, {"stride", std::int64_t(16)}});
        EXPECT(b.stride == 16u && b.strideActive());
        b.strideCounter = 5;
        const auto gen = b._settings_generation;
        b.applySettings({{"stride", std::int64_t(64)}});
        EXPECT(!b.strideActive() && b.strideCounter == 0u && b._settings_generation > gen);
        bool threw = false;
        try { b.applySettings({{"stride", "wide"s}}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
    }
    { // through the plugin: `stride` is a parameter like any other
        const std::string n = "gr::blocks::fft::PowerSpectrum<complex<float32>>";
        EXPECT(loader.isBlockAvailable(n));
        auto m = loader.instantiate(n, {{"fftSize", std::int64_t(64)}, {"stride", std::int64_t(32)}});
        EXPECT(m != nullptr && m->stride_active());
        auto m0 = loader.instantiate(n, {{"fftSize", std::int64_t(64)}});
        EXPECT(m0 != nullptr && !m0->stride_active());
    }
    return 0;
}

static int device_checks(const std::string& prefix) {
    const std::string dom = "gpu:hip:0";
    for (const std::size_t N : {std::size_t(64), std::size_t(1024)}) { // the gather path and the hop kernels
        const auto x = stream(40 * N + 37, 77u + static_cast<std::uint32_t>(N));
        dump(prefix + ".N" + std::to_string(N) + ".in", x);
        for (const long S : {long(N / 2), long(N + 3), long(0)}) {
            std::vector<float> hm, dm, pm;
            if (int rc = run_graph(N, S, x, "", false, false, hm)) return rc;
            if (int rc = run_graph(N, S, x, dom, false, false, dm)) return rc; // the block's own work() behind the seam
            if (int rc = run_graph(N, S, x, dom, true, true, pm)) return rc;   // planned (and fed 1, 7, many): an active stride stays out of the runs
            EXPECT(hm.size() == frames_of(x.size(), N, S == 0 ? N : std::size_t(S)) * N);
            EXPECT(pm == dm || S == 0); // planned and unplanned: the same stream (S = 0: a run's kernels, compared below like the seam's)
            const double e0 = max_rel(dm, hm), e1 = max_rel(pm, hm);
            std::printf("N %zu stride %ld: device against the CPU path: seam %.3g planned %.3g (%zu frames)\n", N, S, e0, e1, hm.size() / N);
            EXPECT(e0 <= 1e-5 && e1 <= 1e-5);
            dump(prefix + ".N" + std::to_string(N) + ".S" + std::to_string(S) + ".mag2.seam", dm);
        }
    }
    return 0;
}

// the same graph from YAML with `stride:` through the plugin
static int yaml_checks(PluginLoader& loader, const std::string& prefix) {
    const std::size_t N = 256, S = 64, n = 20 * N;
    const std::string yaml = "blocks:\n"
                             "  - id: gr::testing::VectorSource<complex<float32>>\n    parameters:\n      name: src\n      n_samples_max: " + std::to_string(n) + "\n"
                             "  - id: gr::blocks::fft::PowerSpectrum<complex<float32>>\n    parameters:\n      name: spec\n      fftSize: " + std::to_string(N) + "\n      window: Hann\n      stride: " + std::to_string(S) + "\n      compute_domain: \"gpu:hip:0\"\n"
                             "  - id: gr::testing::VectorSink<float32>\n    parameters:\n      name: sink\n"
                             "connections:\n  - [src, 0, spec, 0]\n  - [spec, 0, sink, 0]\n";
    Graph      g;
    const auto loaded = loadGrc(loader, g, yaml);
    if (!loaded) { std::fprintf(stderr, "grc: %s\n", loaded.error().message.c_str()); return 3; }
    testing::VectorSink<float>* sink = nullptr;
    BlockModel*                 spec = nullptr;
    for (const auto& b : loaded.value()) {
        if (b.name == "sink") sink = static_cast<testing::VectorSink<float>*>(b.model->raw());
        if (b.name == "spec") spec = b.model;
    }
    EXPECT(sink && spec && spec->stride_active());
    if (!sink) return 1;
    EXPECT(hip::plan(g, 1).empty());
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) { std::fprintf(stderr, "graph: %s\n", r.error().message.c_str()); return 3; }
    EXPECT(sink->_samples.size() == frames_of(n, N, S) * N); // zeros in: zeros out, frame count by the definition
    EXPECT(std::all_of(sink->_samples.begin(), sink->_samples.end(), [](float v) { return v == 0.f; }));
    std::printf("yaml: stride %zu -> %zu frames\n", S, sink->_samples.size() / N);
    (void)prefix;
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s host|device plugin.so output-prefix\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    PluginLoader      loader;
    const auto        ok = loader.load(argv[2]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    try {
        if (mode == "device") {
            if (int rc = device_checks(argv[3])) return rc;
            if (int rc = yaml_checks(loader, argv[3])) return rc;
        } else if (int rc = host_checks(loader, argv[3])) return rc;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "graph: %s\n", e.what());
        return 3;
    }
    if (failures) std::printf("stft %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("stft %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
