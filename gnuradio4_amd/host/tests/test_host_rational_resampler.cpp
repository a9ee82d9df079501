// gr::filter::rational_resampler<T> of the host layer (gr4/blocks.hpp, gr4/hip.hpp): polyphase FIR at rate interpolate / decimate, float and complex<float>.
//   test_host_rational_resampler host   <libgr4hip_blocks.so>   the CPU body against the literal definition evaluated here over chunked calls, the carried inputs
//                                                               across settings changes, the settings errors, the plugin registration, gr:sample_rate times L / M
//   test_host_rational_resampler device <libgr4hip_blocks.so>   source -> rational_resampler -> sink on gpu:hip:0 against the CPU body, behind the compute_domain
//                                                               seam and as a hip::plan run
// Exit code 0: everything held; 1: a check failed; 3: a graph failed (a device domain without a device fails loudly).
#include <cstdio>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;
using C32 = std::complex<float>;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

template <typename T>
static std::vector<T> stream(std::size_t n, std::uint32_t seed) {
    std::vector<T> x(n);
    std::uint32_t  lcg  = seed;
    const auto     next = [&] { lcg = lcg * 1664525u + 1013904223u; return static_cast<float>(static_cast<std::int32_t>(lcg >> 8) % 2001 - 1000) / 1000.f; };
    for (auto& v : x) {
        if constexpr (std::is_same_v<T, C32>) { const float re = next(), im = next(); v = {re, im}; }
        else v = next();
    }
    return x;
}
static std::vector<float> taps(std::size_t K, std::size_t L, std::size_t M) { // Hamming low-pass at 0.4 / max(L, M) of the L-times rate, DC gain 1
    std::vector<double> h(K);
    const double        fc2 = 0.8 / double(std::max(L, M)), mid = double(K - 1) * 0.5;
    double              sum = 0;
    for (std::size_t k = 0; k < K; ++k) {
        const double a = std::numbers::pi * fc2 * (double(k) - mid);
        h[k]           = (0.54 - 0.46 * std::cos(2 * std::numbers::pi * double(k) / double(K > 1 ? K - 1 : 1))) * (a == 0.0 ? 1.0 : std::sin(a) / a);
        sum += h[k];
    }
    std::vector<float> b(K);
    for (std::size_t k = 0; k < K; ++k) b[k] = static_cast<float>(h[k] / sum);
    return b;
}
template <typename T> struct wide { using type = double; };
template <> struct wide<C32> { using type = std::complex<double>; };
// the literal definition in double: u = x zero-stuffed by L (history `before` in front), v[n] = L sum_k b[k] u[n - k], y[j] = v[j M]
template <typename T>
static std::vector<T> literal(const std::vector<float>& b, const std::vector<T>& x, std::size_t L, std::size_t M, const std::vector<T>& before = {}) {
    using W = typename wide<T>::type;
    const long     nb = static_cast<long>(before.size());
    const auto     at = [&](long i) { return i >= 0 ? W(x[static_cast<std::size_t>(i)]) : (i >= -nb ? W(before[static_cast<std::size_t>(nb + i)]) : W{}); };
    std::vector<T> y(x.size() / M * L);
    for (std::size_t j = 0; j < y.size(); ++j) {
        W acc{};
        for (std::size_t k = 0; k < b.size(); ++k) {
            const long n = static_cast<long>(j * M) - static_cast<long>(k); // position at the L-times rate
            if (((n % long(L)) + long(L)) % long(L) != 0) continue;           // a stuffed zero
            acc += double(b[k]) * at(n >= 0 ? n / long(L) : -((-n) / long(L)));
        }
        y[j] = static_cast<T>(double(L) * acc);
    }
    return y;
}
template <typename T>
static double max_rel(const std::vector<T>& got, const std::vector<T>& want) { // max |got - want| / max(|want|, rms(want))
    using W = typename wide<T>::type;
    if (got.size() != want.size() || want.empty()) return 1e30;
    double rms = 0;
    for (const auto& v : want) rms += std::norm(W(v));
    rms = std::sqrt(rms / double(want.size()));
    double worst = 0;
    for (std::size_t i = 0; i < want.size(); ++i) worst = std::max(worst, std::abs(W(got[i]) - W(want[i])) / std::max(std::abs(W(want[i])), rms));
    return worst;
}
template <typename T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

template <typename T>
static property_map settings(const std::vector<float>& b, std::size_t L, std::size_t M) { return {{"b", b}, {"interpolate", std::int64_t(L)}, {"decimate", std::int64_t(M)}}; }

// source -> rational_resampler -> sink; domain "" = host
template <typename T>
static int run_graph(const std::vector<float>& b, std::size_t L, std::size_t M, const std::vector<T>& x, const std::string& domain, bool planned, std::vector<T>& y, std::vector<Tag>* tags = nullptr) {
    using B = filter::rational_resampler<T>;
    Graph g;
    auto& src  = g.emplaceBlock<testing::VectorSource<T>>();
    src.values = x;
    if (tags) src._tags = {{0, {{"gr:sample_rate", 48000.f}}}};
    property_map cfg = settings<T>(b, L, M);
    if (!domain.empty()) cfg["compute_domain"] = domain;
    auto& rs   = g.emplaceBlock<B>(cfg);
    rs._log    = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<T>>();
    if (!g.connect<"out", "in">(src, rs) || !g.connect<"out", "in">(rs, sink)) return 2;
    if (planned) {
        const auto runs = hip::plan(g, 1); // a run of one stage
        std::printf("planner: %zu runs:", runs.size());
        for (auto* r : runs) std::printf(" [%s]", std::string(r->description()).c_str());
        std::printf("\n");
        EXPECT(runs.size() == 1 && runs[0]->stages().size() == 1u && std::string(runs[0]->description()).find("fir_resamp") != std::string::npos);
    }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (!domain.empty() && !planned) EXPECT(rs._device_state != nullptr); // the seam was taken
    y = sink._samples;
    if (tags) *tags = sink._tags;
    return 0;
}

template <typename T>
static void body_checks() {
    using B = filter::rational_resampler<T>;
    struct Shape { std::size_t L, M, K; };
    for (const Shape& s : {Shape{1, 1, 5}, {2, 3, 25}, {3, 2, 2}, {3, 4, 96}, {5, 7, 43}, {7, 5, 59}, {4, 6, 24}, {8, 1, 67}, {1, 8, 64}, {16, 5, 131}, {147, 160, 1179}}) {
        const auto b = taps(s.K, s.L, s.M);
        const auto x = stream<T>(s.M * 97, 17u + static_cast<std::uint32_t>(s.K));
        B          f;
        f.applySettings(settings<T>(b, s.L, s.M));
        EXPECT(f.input_chunk_size == s.M && f.output_chunk_size == s.L);
        std::vector<T> y(x.size() / s.M * s.L);
        EXPECT(f.processBulk(std::span<const T>(x), std::span<T>(y)) == work::Status::OK);
        const double e = max_rel(y, literal(b, x, s.L, s.M));
        if (e > 1e-5) std::printf("L %zu M %zu K %zu: %.3g\n", s.L, s.M, s.K, e);
        EXPECT(e <= 1e-5);
        B f2; // chunks of 1, 2, 3, ... cycles give the same stream bit for bit
        f2.applySettings(settings<T>(b, s.L, s.M));
        std::vector<T> y2(y.size());
        for (std::size_t c = 0, n = 1; c < 97; c += n, ++n) {
            const std::size_t m = std::min(n, 97 - c);
            EXPECT(f2.processBulk(std::span<const T>(x.data() + c * s.M, m * s.M), std::span<T>(y2.data() + c * s.L, m * s.L)) == work::Status::OK);
        }
        EXPECT(same_bits(y2, y));
        f2.reset();
        std::vector<T> y3(y.size());
        (void)f2.processBulk(std::span<const T>(x), std::span<T>(y3));
        EXPECT(same_bits(y3, y)); // reset cleared the carried inputs
    }
    { // a unit impulse at input i reads the branch taps back: output j = c L + p holds float(L) b[q L + phi_p] with q = c M + o_p - i
        const std::size_t L = 3, M = 4, K = 20, i = 5;
        std::vector<float> b(K);
        for (std::size_t k = 0; k < K; ++k) b[k] = 0.25f + float(k) / 64.f;
        B f;
        f.applySettings(settings<T>(b, L, M));
        std::vector<T> x(M * 8), y(L * 8);
        x[i] = T(1.f);
        (void)f.processBulk(std::span<const T>(x), std::span<T>(y));
        for (std::size_t j = 0; j < y.size(); ++j) {
            const long  q   = long(j / L * M + (j % L) * M / L) - long(i);
            const auto  k   = std::size_t(q) * L + (j % L) * M % L;
            const float exp = q >= 0 && k < K ? float(L) * b[k] : 0.f;
            EXPECT(y[j] == T(exp));
        }
    }
    { // new taps keep the carried inputs; another rate clears them
        const std::size_t L = 3, M = 4;
        const auto        b1 = taps(40, L, M), b2 = taps(61, L, M);
        const auto        x1 = stream<T>(M * 50, 3u), x2 = stream<T>(M * 50, 4u);
        B                 f;
        f.applySettings(settings<T>(b1, L, M));
        std::vector<T> y(L * 50);
        (void)f.processBulk(std::span<const T>(x1), std::span<T>(y));
        f.applySettings({{"b", b2}});
        (void)f.processBulk(std::span<const T>(x2), std::span<T>(y));
        EXPECT(max_rel(y, literal(b2, x2, L, M, x1)) <= 1e-5);
        EXPECT(max_rel(y, literal(b2, x2, L, M)) > 1e-3); // (the history matters in this comparison)
        f.applySettings({{"decimate", std::int64_t(5)}});
        std::vector<T> z(L * 40);
        (void)f.processBulk(std::span<const T>(x1), std::span<T>(z));
        EXPECT(max_rel(z, literal(b2, x1, L, 5)) <= 1e-5);
        f.applySettings({{"interpolate", std::int64_t(2)}});
        std::vector<T> w(2 * 40);
        (void)f.processBulk(std::span<const T>(x2), std::span<T>(w));
        EXPECT(max_rel(w, literal(b2, x2, 2, 5)) <= 1e-5);
    }
}

static int host_checks(PluginLoader& loader) {
    body_checks<float>();
    body_checks<C32>();
    { // the settings errors; the reflected members; the defaults
        using B = filter::rational_resampler<float>;
        for (const property_map& bad : {property_map{{"interpolate", std::int64_t(0)}}, property_map{{"decimate", std::int64_t(0)}}, property_map{{"b", std::vector<float>{}}}}) {
            B    f;
            bool threw = false;
            try { f.applySettings(bad); } catch (const std::invalid_argument&) { threw = true; }
            EXPECT(threw);
        }
        constexpr auto                        names = B::gr_member_names();
        const std::array<std::string_view, 5> want{"in", "out", "b", "interpolate", "decimate"};
        EXPECT(names.size() == want.size());
        for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
        B d; // defaults: the identity
        EXPECT(d.b == std::vector<float>{1.f} && d.interpolate == 1u && d.decimate == 1u);
        std::vector<float> x{1.f, -2.f, 3.f}, y(3);
        (void)d.processBulk(std::span<const float>(x), std::span<float>(y));
        EXPECT(y == x);
    }
    { // the plugin knows both instantiations under their portable type names
        for (const std::string n : {"gr::filter::rational_resampler<float32>", "gr::filter::rational_resampler<complex<float32>>"}) {
            EXPECT(loader.isBlockAvailable(n));
            EXPECT(loader.instantiate(n, {{"b", std::vector<float>{0.5f, 0.25f}}, {"interpolate", std::int64_t(3)}, {"decimate", std::int64_t(2)}}) != nullptr);
        }
        EXPECT(!loader.isBlockAvailable("gr::filter::rational_resampler<float64>"));
    }
    { // in a graph: whole cycles per work() call, gr:sample_rate forwarded times L / M, the graph's output is the body's
        const std::size_t  L = 147, M = 160;
        const auto         b = taps(8 * L + 3, L, M);
        const auto         x = stream<float>(M * 300, 5u);
        std::vector<float> y;
        std::vector<Tag>   tags;
        if (int rc = run_graph(b, L, M, x, "", false, y, &tags)) return rc;
        EXPECT(max_rel(y, literal(b, x, L, M)) <= 1e-5);
        EXPECT(tags.size() == 1u);
        if (tags.size() == 1) EXPECT(tags[0].index == 0u && (tags[0].map == property_map{{"gr:sample_rate", 44100.f}}));
    }
    return 0;
}

template <typename T>
static int device_checks_of(const char* what) {
    const std::string dom = "gpu:hip:0";
    struct Shape { std::size_t L, M, K; };
    for (const Shape& s : {Shape{3, 4, 96}, {147, 160, 1179}, {8, 1, 67}, {1, 8, 64}}) { // the window and the gather form, more and fewer outputs than inputs
        const auto     b = taps(s.K, s.L, s.M);
        const auto     x = stream<T>(s.M * 1501, 99u + static_cast<std::uint32_t>(s.K));
        std::vector<T> h, d, p;
        if (int rc = run_graph(b, s.L, s.M, x, "", false, h)) return rc;
        if (int rc = run_graph(b, s.L, s.M, x, dom, false, d)) return rc; // the block's own work() behind the seam
        if (int rc = run_graph(b, s.L, s.M, x, dom, true, p)) return rc;  // a planned run of one stage
        const double e1 = max_rel(d, h), e2 = max_rel(p, h);
        std::printf("rational_resampler<%s> L %zu M %zu K %zu: seam %.3g, planned %.3g%s\n", what, s.L, s.M, s.K, e1, e2, e1 <= 1e-5 && e2 <= 1e-5 ? "" : "  FAILED");
        EXPECT(e1 <= 1e-5 && e2 <= 1e-5);
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
        int rc = 0;
        if (mode == "device") { rc = device_checks_of<float>("float"); if (!rc) rc = device_checks_of<C32>("complex<float>"); }
        else rc = host_checks(loader);
        if (rc) return rc;
    } catch (const std::exception& e) { // (the planner makes its stages before anything runs: no device, no stage)
        std::fprintf(stderr, "graph: %s\n", e.what());
        return 3;
    }
    if (failures) std::printf("rational_resampler %s: %d FAILURES\n", mode.c_str(), failures);
    else std::printf("rational_resampler %s: ok\n", mode.c_str());
    return failures ? 1 : 0;
}
