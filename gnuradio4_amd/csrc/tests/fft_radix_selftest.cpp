// fft_radix_selftest.cpp -- the register-level butterflies of csrc/fft_radix.hpp on the host, against float64 DFTs (tests/test_fft_radix_host.py builds and runs it;
// host side of a HIP compile: hipcc -x hip --cuda-host-only).  Prints one line per check, "<name> <error>", the error relative to the largest output magnitude
// (worst over the inputs: a unit impulse in every slot; seeded noise).  The bars are the test's.
#include "../fft_radix.hpp"

#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <vector>

using cd = std::complex<double>;
using namespace gr4;

static const uint64_t kSeed = 0x9E3779B97F4A7C15ull;
static uint64_t       rng_state = kSeed;
static double   uniform() { // xorshift64*, (0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 + 1e-17;
}
static double gauss() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }

static std::vector<cd> dft(const std::vector<cd>& x) {
    const int       n = (int)x.size();
    std::vector<cd> X(n);
    for (int k = 0; k < n; ++k) {
        cd s = 0;
        for (int j = 0; j < n; ++j) s += x[j] * std::polar(1.0, -2.0 * M_PI * ((j * k) % n) / n);
        X[k] = s;
    }
    return X;
}
static double rel_err(const std::vector<cd>& got, const std::vector<cd>& want) {
    double e = 0, m = 0;
    for (size_t i = 0; i < want.size(); ++i) { e = std::max(e, std::abs(got[i] - want[i])); m = std::max(m, std::abs(want[i])); }
    return e / m;
}

// input i of n-point checks: i < n a unit impulse at slot i, then noise
static std::vector<float2> input(int n, int i) {
    std::vector<float2> x(n, make_float2(0.f, 0.f));
    if (i < n) x[i] = make_float2(1.f, 0.f);
    else for (auto& v : x) v = make_float2((float)gauss(), (float)gauss());
    return x;
}
static cd wide(float2 a) { return cd(a.x, a.y); }

template <bool FOLD>
static double check_fft16(int lo, int hi) { // inputs lo .. hi - 1
    double worst = 0;
    for (int i = lo; i < hi; ++i) {
        std::vector<float2> x = input(16, i);
        std::vector<cd>     xd(16), got(16);
        for (int r = 0; r < 16; ++r) xd[r] = wide(x[r]);
        if constexpr (FOLD) fft16_fold<1>(x.data());
        else fft16<1>(x.data());
        for (int m = 0; m < 16; ++m) got[m] = wide(x[perm16(m)]);
        worst = std::max(worst, rel_err(got, dft(xd)));
    }
    return worst;
}

template <bool FOLD>
static double check_fft16_tw(int lo, int hi) { // unit-modulus twiddles of random phase, as float32 values: the reference multiplies by what the code was given
    double worst = 0;
    for (int i = lo; i < hi; ++i) {
        std::vector<float2> x = input(16, i);
        float2              tw[16];
        tw[0] = make_float2(1.f, 0.f);
        for (int r = 1; r < 16; ++r) { const double p = 6.283185307179586 * uniform(); tw[r] = make_float2((float)std::cos(p), (float)std::sin(p)); }
        std::vector<cd> xd(16), got(16);
        for (int r = 0; r < 16; ++r) xd[r] = wide(x[r]) * wide(tw[r]);
        if constexpr (FOLD) fft16_tw_fold<1>(x.data(), [&](int r) { return tw[r]; });
        else fft16_tw<1>(x.data(), [&](int r) { return tw[r]; });
        for (int m = 0; m < 16; ++m) got[m] = wide(x[perm16(m)]);
        worst = std::max(worst, rel_err(got, dft(xd)));
    }
    return worst;
}

template <bool FOLD>
static void run(const char* name) { // both families on the same inputs: the generator starts over
    rng_state = kSeed;
    const int n_noise = 64;
    std::printf("%s_impulses %.6e\n", name, check_fft16<FOLD>(0, 16));
    std::printf("%s_noise %.6e\n", name, check_fft16<FOLD>(16, 16 + n_noise));
    std::printf("%s_tw_impulses %.6e\n", name, check_fft16_tw<FOLD>(0, 16));
    std::printf("%s_tw_noise %.6e\n", name, check_fft16_tw<FOLD>(16, 16 + n_noise));
}

int main() {
    run<false>("fft16");      // the plain butterflies (the FFT block's kernels)
    run<true>("fft16_fold");  // the folded second step (the fused chain)
    return 0;
}
