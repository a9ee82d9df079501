// The Savitzky-Golay blocks of the host layer (gr4/blocks.hpp, gr4/hip.hpp); links libgr4hip.so, whose host code designs the coefficients.
//   test_host_savitzky_golay <libgr4hip_blocks.so> <compute_domain> [dir]
// Always: the defaults and reflected members of both blocks (SavitzkyGolayFilter.hpp:37-43, 111-116), settings by name, "an alignment that is not Causal is Centred",
// "a boundary policy that is not Replicate is Reflect", the four registered names in the plugin.
// With dir (holding x.f32 and x.f64, the same stream in both types), on compute_domain:
//   stream_f32   source -> SavitzkyGolayFilter<float>  {11, 4, 1, sample_rate 1000, Causal} -> sink   (a device domain: through hip::plan, one run of one stage)
//   stream_f64   source -> SavitzkyGolayFilter<double> {33, 3, 0, Centred} -> sink
//   stream_set   as stream_f32 but {5, 2, 0} at first and a tag at sample 2000 that sets window_size 11: the history starts again there
//   dataset_f32  source -> FFT<float> {512, Hann} (host) -> SavitzkyGolayDataSetFilter<float>  {11, 4, 0, Reflect} -> sink
//   dataset_f64  source -> FFT<double> {256, Hann} (host) -> SavitzkyGolayDataSetFilter<double> {8, 2, 1, Replicate} -> sink
//   dataset_gap  source of three DataSet<float> with 32, 0 and 32 values -> SavitzkyGolayDataSetFilter<float> {11, 4, 0, Reflect} -> sink: the empty one is
//                passed through between two that are filtered
//   dataset_retune  three DataSet<float> of 32 values, {11, 4, 0, Reflect}, window_size 7 by a settings tag on the second: new coefficients on the live handle
// The outputs go to dir/<graph>.<domain tag>.bin, the DataSet graphs' unfiltered signal_values to dir/<graph>.in.bin (the Python side compares them with the oracle,
// and the device's with the host's).  Exit code 3: a graph failed (a device domain without a device fails loudly).
#include <cstdio>
#include <fstream>
#include <iostream>

#include <gr4/hip.hpp>
#include <gr4/plugin.hpp>

using namespace gr;
using namespace std::string_literals;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

template <typename T>
static std::vector<T> load(const std::string& path) {
    std::ifstream     f(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T>    x(raw.size() / sizeof(T));
    std::memcpy(x.data(), raw.data(), x.size() * sizeof(T));
    return x;
}
template <typename T>
static void dump(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

template <typename T>
static int stream_graph(const std::string& domain, const std::string& dir, const std::string& name, property_map settings, bool retune) {
    using B = filter::SavitzkyGolayFilter<T>;
    const bool dev = domain != "host";
    Graph      g;
    auto&      src = g.emplaceBlock<testing::VectorSource<T>>();
    src.values     = load<T>(dir + (sizeof(T) == 4 ? "/x.f32" : "/x.f64"));
    if (retune) src._tags.push_back(Tag{2000, property_map{{"window_size", std::int64_t(11)}}});
    settings["compute_domain"] = domain;
    auto& blk  = g.emplaceBlock<B>(settings);
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    auto& sink = g.emplaceBlock<testing::VectorSink<T>>();
    if (!g.connect<"out", "in">(src, blk) || !g.connect<"out", "in">(blk, sink)) return 2;
    std::size_t runs = 0;
    if (dev && !retune) { // the planner takes the block as a run of one stage
        const auto r = hip::plan(g, 1);
        runs         = r.size();
        EXPECT(runs == 1 && r[0]->stages().size() == 1 && r[0]->description() == (sizeof(T) == 4 ? "savgol_f32" : "savgol_f64"));
    }
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "%s graph: %s\n", name.c_str(), r.error().message.c_str());
        return 3;
    }
    EXPECT(sink._samples.size() == src.values.size());
    dump(dir + "/" + name + (dev ? ".device.bin" : ".host.bin"), sink._samples);
    std::printf("%s: %zu samples, %zu planned runs\n", name.c_str(), sink._samples.size(), runs);
    return 0;
}

template <typename T, typename FFTBlock>
static int dataset_graph(const std::string& domain, const std::string& dir, const std::string& name, std::int64_t fft_size, property_map settings) {
    using B = filter::SavitzkyGolayDataSetFilter<T>;
    const bool dev = domain != "host";
    std::vector<T> filtered, unfiltered;
    for (int pass = 0; pass < 2; ++pass) { // 0: the FFT's DataSets as they are; 1: through the filter
        Graph g;
        auto& src  = g.emplaceBlock<testing::VectorSource<T>>();
        src.values = load<T>(dir + (sizeof(T) == 4 ? "/x.f32" : "/x.f64"));
        src.values.resize(static_cast<std::size_t>(fft_size) * 3);
        auto& fft  = g.emplaceBlock<FFTBlock>({{"fftSize", fft_size}, {"window", "Hann"s}});
        auto& sink = g.emplaceBlock<testing::VectorSink<DataSet<T>>>();
        B*    blk  = nullptr;
        if (pass) {
            settings["compute_domain"] = domain;
            blk       = &g.emplaceBlock<B>(settings);
            blk->_log = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
            if (!g.connect<"out", "in">(src, fft) || !g.connect<"out", "in">(fft, *blk) || !g.connect<"out", "in">(*blk, sink)) return 2;
        } else if (!g.connect<"out", "in">(src, fft) || !g.connect<"out", "in">(fft, sink)) return 2;
        scheduler::Simple sched;
        sched.exchange(std::move(g));
        if (const auto r = sched.runAndWait(); !r) {
            std::fprintf(stderr, "%s graph: %s\n", name.c_str(), r.error().message.c_str());
            return 3;
        }
        EXPECT(sink._samples.size() == 3);
        if (pass && dev) EXPECT(blk->_device_state != nullptr);
        for (const auto& ds : sink._samples) {
            auto& to = pass ? filtered : unfiltered;
            to.insert(to.end(), ds.signal_values.begin(), ds.signal_values.end());
            EXPECT(ds.signal_names.size() == 4 && ds.signal_ranges.size() == 4 && ds.axis_values.size() == 1); // everything else is passed through
        }
    }
    EXPECT(filtered.size() == unfiltered.size() && !filtered.empty());
    dump(dir + "/" + name + ".in.bin", unfiltered);
    dump(dir + "/" + name + (dev ? ".device.bin" : ".host.bin"), filtered);
    std::printf("%s: %zu values in 3 DataSets\n", name.c_str(), filtered.size());
    return 0;
}

// hands out the DataSets it was given (VectorSource's `values` is a setting, and settings are compared: a DataSet is not)
struct DataSetSource : Block<DataSetSource> {
    PortOut<DataSet<float>> out;
    GR_MAKE_REFLECTABLE(DataSetSource, out);
    std::vector<DataSet<float>> values;
    std::vector<Tag>            _tags; // as VectorSource's
    std::size_t                 _produced = 0;
    work::Result customWork(std::size_t requested) {
        if (_produced >= values.size()) return {requested, 0, work::Status::DONE};
        if (!out.connected()) return {requested, 0, work::Status::ERROR};
        const std::size_t n = std::min({values.size() - _produced, out.buffer->free_space(), requested});
        if (n == 0) return {requested, 0, work::Status::INSUFFICIENT_OUTPUT_ITEMS};
        std::copy_n(values.begin() + static_cast<std::ptrdiff_t>(_produced), n, out.buffer->write_span(n).begin());
        for (const Tag& t : _tags)
            if (t.index >= _produced && t.index < _produced + n) out.buffer->publishTag(t.map, t.index - _produced);
        out.buffer->publish(n);
        _produced += n;
        return {requested, n, work::Status::OK};
    }
};

static int gap_graph(const std::string& domain, const std::string& dir) {
    using B = filter::SavitzkyGolayDataSetFilter<float>;
    const bool         dev = domain != "host";
    const auto         x   = load<float>(dir + "/x.f32");
    std::vector<float> filtered, unfiltered(x.begin(), x.begin() + 64);
    Graph g;
    auto& src = g.emplaceBlock<DataSetSource>();
    src.values.resize(3);
    src.values[0].signal_values.assign(x.begin(), x.begin() + 32);
    src.values[2].signal_values.assign(x.begin() + 32, x.begin() + 64);
    for (auto& ds : src.values) ds.signal_names = {"gap"};
    auto& blk  = g.emplaceBlock<B>({{"window_size", std::int64_t(11)}, {"poly_order", std::int64_t(4)}, {"compute_domain", domain}});
    auto& sink = g.emplaceBlock<testing::VectorSink<DataSet<float>>>();
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    if (!g.connect<"out", "in">(src, blk) || !g.connect<"out", "in">(blk, sink)) return 2;
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "dataset_gap graph: %s\n", r.error().message.c_str());
        return 3;
    }
    if (dev) EXPECT(blk._device_state != nullptr);
    EXPECT(sink._samples.size() == 3);
    if (sink._samples.size() != 3) return 0;
    EXPECT(sink._samples[0].signal_values.size() == 32 && sink._samples[1].signal_values.empty() && sink._samples[2].signal_values.size() == 32);
    for (const auto& ds : sink._samples) {
        EXPECT(ds.signal_names == std::vector<std::string>{"gap"}); // everything else is passed through
        filtered.insert(filtered.end(), ds.signal_values.begin(), ds.signal_values.end());
    }
    EXPECT(filtered != unfiltered);
    dump(dir + "/dataset_gap.in.bin", unfiltered);
    dump(dir + "/dataset_gap" + (dev ? ".device.bin" : ".host.bin"), filtered);
    std::printf("dataset_gap: %zu values in 3 DataSets, the middle one empty\n", filtered.size());
    return 0;
}

static int retune_graph(const std::string& domain, const std::string& dir) {
    using B = filter::SavitzkyGolayDataSetFilter<float>;
    const bool         dev = domain != "host";
    const auto         x   = load<float>(dir + "/x.f32");
    std::vector<float> filtered, unfiltered(x.begin() + 64, x.begin() + 160);
    Graph g;
    auto& src = g.emplaceBlock<DataSetSource>();
    src.values.resize(3);
    for (std::size_t f = 0; f < 3; ++f) src.values[f].signal_values.assign(unfiltered.begin() + static_cast<std::ptrdiff_t>(32 * f), unfiltered.begin() + static_cast<std::ptrdiff_t>(32 * (f + 1)));
    src._tags  = {{1, {{"window_size", std::int64_t(7)}}}};
    auto& blk  = g.emplaceBlock<B>({{"window_size", std::int64_t(11)}, {"poly_order", std::int64_t(4)}, {"compute_domain", domain}});
    auto& sink = g.emplaceBlock<testing::VectorSink<DataSet<float>>>();
    blk._log   = [](std::string_view m) { std::cerr << "[log] " << m << "\n"; };
    if (!g.connect<"out", "in">(src, blk) || !g.connect<"out", "in">(blk, sink)) return 2;
    scheduler::Simple sched;
    sched.exchange(std::move(g));
    if (const auto r = sched.runAndWait(); !r) {
        std::fprintf(stderr, "dataset_retune graph: %s\n", r.error().message.c_str());
        return 3;
    }
    EXPECT(sink._samples.size() == 3 && blk._settings_by_tag == 1 && blk.window_size.value == 7u);
    for (const auto& ds : sink._samples) filtered.insert(filtered.end(), ds.signal_values.begin(), ds.signal_values.end());
    EXPECT(filtered.size() == unfiltered.size());
    dump(dir + "/dataset_retune.in.bin", unfiltered);
    dump(dir + "/dataset_retune" + (dev ? ".device.bin" : ".host.bin"), filtered);
    std::printf("dataset_retune: %zu values in 3 DataSets, window_size 11 then 7\n", filtered.size());
    return 0;
}

template <typename T>
static void check_blocks(PluginLoader& loader, const std::string& suffix) {
    using S = filter::SavitzkyGolayFilter<T>;
    using D = filter::SavitzkyGolayDataSetFilter<T>;
    for (const char* base : {"gr::filter::SavitzkyGolayFilter", "gr::filter::SavitzkyGolayDataSetFilter"}) {
        const std::string n = std::string(base) + "<" + suffix + ">";
        EXPECT(loader.isBlockAvailable(n));
        EXPECT(loader.instantiate(n, {{"window_size", std::int64_t(21)}, {"poly_order", std::int64_t(3)}}) != nullptr);
    }
    S s; // (:37-41)
    EXPECT(s.window_size.value == 11u && s.poly_order.value == 4u && s.deriv_order.value == 0u && s.sample_rate.value == 1.0f && s.alignment.value == "Centred");
    EXPECT(!s._parameters_changed && !s.causal() && s.delta() == T(1));
    {
        constexpr auto                        names = S::gr_member_names();
        const std::array<std::string_view, 7> want{"in", "out", "window_size", "poly_order", "deriv_order", "sample_rate", "alignment"}; // (:43)
        EXPECT(names.size() == want.size());
        for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
    }
    s.applySettings({{"window_size", std::int64_t(7)}, {"poly_order", std::int64_t(2)}, {"deriv_order", std::int64_t(1)}, {"sample_rate", 250.f}, {"alignment", "Causal"s}});
    EXPECT(s._parameters_changed && s.window_size.value == 7u && s.poly_order.value == 2u && s.deriv_order.value == 1u && s.causal() && s.delta() == T(1) / T(250));
    const auto causal = s.designCoefficients();
    s.applySettings({{"alignment", "Sideways"s}}); // anything but "Causal" is Centred (:53-55)
    EXPECT(!s.causal());
    const auto centred = s.designCoefficients();
    s.applySettings({{"alignment", "Centred"s}});
    EXPECT(centred == s.designCoefficients() && centred != causal && centred.size() == 7);
    s.applySettings({{"sample_rate", -3.f}}); // (:52) not positive: delta 1
    EXPECT(s.delta() == T(1));
    // the streaming body: an impulse gives the coefficients back to front, and setParameters clears the history
    S f;
    f.applySettings({{"window_size", std::int64_t(5)}, {"poly_order", std::int64_t(2)}});
    const auto      c = f.designCoefficients();
    std::vector<T>  y;
    for (int i = 0; i < 5; ++i) y.push_back(f.processOne(i == 0 ? T(1) : T(0)));
    for (int i = 0; i < 5; ++i) EXPECT(y[static_cast<std::size_t>(i)] == c[static_cast<std::size_t>(4 - i)]);
    (void)f.processOne(T(100));
    f.applySettings({{"deriv_order", std::int64_t(0)}}); // names a setting: a reset (:67-76)
    EXPECT(f.processOne(T(0)) == T(0));
    (void)f.processOne(T(100));
    f.reset();
    EXPECT(f.processOne(T(0)) == T(0));

    D d; // (:111-114)
    EXPECT(d.window_size.value == 11u && d.poly_order.value == 4u && d.deriv_order.value == 0u && d.boundary_policy.value == "Reflect" && !d.replicate());
    {
        constexpr auto                        names = D::gr_member_names();
        const std::array<std::string_view, 6> want{"in", "out", "window_size", "poly_order", "deriv_order", "boundary_policy"}; // (:116)
        EXPECT(names.size() == want.size());
        for (std::size_t k = 0; k < std::min(names.size(), want.size()); ++k) EXPECT(std::string_view(names[k]) == want[k]);
    }
    d.applySettings({{"boundary_policy", "Replicate"s}, {"window_size", std::int64_t(4)}, {"poly_order", std::int64_t(9)}});
    EXPECT(d.replicate() && d._parameters_changed);
    const auto p = d.params();
    EXPECT(p.window_size == 4u && p.poly_order == 9u && p.boundary_policy == GR4HIP_SAVGOL_REPLICATE && p.dtype == (sizeof(T) == 4 ? GR4HIP_F32 : GR4HIP_F64));
    d.applySettings({{"boundary_policy", "Wrap"s}}); // anything but "Replicate" is Reflect (:126-128)
    EXPECT(!d.replicate());
    DataSet<T> empty;
    empty.signal_names = {"nothing"};
    const auto back    = d.processOne(empty); // (:150-152)
    EXPECT(back.signal_values.empty() && back.signal_names.size() == 1);
    DataSet<T> one;
    one.signal_values = {T(1), T(2), T(4), T(8), T(16), T(32)};
    one.signal_names  = {"a", "b"};
    const auto got    = d.processOne(one);
    std::vector<T> want(6);
    const auto     cz = filter::savitzky_golay::design<T>(4, 9, 0, T(1), false);
    filter::savitzky_golay::applyZeroPhase<T>(std::span<const T>(one.signal_values), std::span<T>(want), std::span<const T>(cz), false);
    EXPECT(got.signal_values == want && got.signal_names.size() == 2 && cz.size() == 4);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s plugin.so compute_domain [dir]\n", argv[0]); return 2; }
    const std::string domain = argv[2];
    PluginLoader      loader;
    const auto        ok = loader.load(argv[1]);
    if (!ok) { std::fprintf(stderr, "%s\n", ok.error().message.c_str()); return 2; }
    check_blocks<float>(loader, "float32");
    check_blocks<double>(loader, "float64");
    if (argc >= 4) try {
        const std::string dir = argv[3];
        if (int rc = stream_graph<float>(domain, dir, "stream_f32", {{"window_size", std::int64_t(11)}, {"poly_order", std::int64_t(4)}, {"deriv_order", std::int64_t(1)}, {"sample_rate", 1000.f}, {"alignment", "Causal"s}}, false)) return rc;
        if (int rc = stream_graph<double>(domain, dir, "stream_f64", {{"window_size", std::int64_t(33)}, {"poly_order", std::int64_t(3)}}, false)) return rc;
        if (int rc = stream_graph<float>(domain, dir, "stream_set", {{"window_size", std::int64_t(5)}, {"poly_order", std::int64_t(2)}}, true)) return rc;
        if (int rc = dataset_graph<float, blocks::fft::FFT<float>>(domain, dir, "dataset_f32", 512, {{"window_size", std::int64_t(11)}, {"poly_order", std::int64_t(4)}})) return rc;
        if (int rc = dataset_graph<double, blocks::fft::FFT<double, DataSet<double>>>(domain, dir, "dataset_f64", 256, {{"window_size", std::int64_t(8)}, {"poly_order", std::int64_t(2)}, {"deriv_order", std::int64_t(1)}, {"boundary_policy", "Replicate"s}})) return rc;
        if (int rc = gap_graph(domain, dir)) return rc;
        if (int rc = retune_graph(domain, dir)) return rc;
    } catch (const std::exception& e) { // (the planner makes its stages before anything runs: no device, no stage)
        std::fprintf(stderr, "graph: %s\n", e.what());
        return 3;
    }
    if (failures) std::printf("host-savitzky-golay: %d FAILURES\n", failures);
    else std::printf("host-savitzky-golay: all checks passed (compute_domain %s)\n", domain.c_str());
    return failures ? 1 : 0;
}
