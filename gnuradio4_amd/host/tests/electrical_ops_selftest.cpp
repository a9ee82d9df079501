// The arithmetic of PowerFactor / SystemUnbalance (gr4/electrical_ops.hpp) over the special-value grid, as a stand-alone program: tests/test_electrical_host.py
// builds it with -fsanitize=address,undefined and runs it.  Every expression is defined behaviour on every input, and the consequences POWER_QUALITY.md lists hold.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include <gr4/electrical_ops.hpp>

namespace ops = gr4::electrical_ops;
static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

template <typename T>
static std::vector<T> specials() {
    using L = std::numeric_limits<T>;
    return {T(0), -T(0), T(1), T(-1), L::quiet_NaN(), L::infinity(), -L::infinity(), L::max(), -L::max(), L::min(), L::denorm_min(), T(230), T(232.3), T(227.7)};
}
template <typename T>
static bool same_bits(T a, T b) { return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof(T)) == 0; }

static unsigned long long sink = 0; // keeps every result alive

template <typename T>
static void power_factor() {
    const T half_pi = std::acos(T(0)), pi = std::acos(T(-1));
    for (T P : specials<T>())
        for (T S : specials<T>()) {
            const T c = ops::power_factor<T>(P, S), phi = ops::acos_of(c);
            sink += c == c;
            EXPECT(std::isnan(c) || (c >= T(-1) && c <= T(1)));
            EXPECT(std::isnan(c) == std::isnan(phi));
            if (S == T(0)) EXPECT(c == T(0) && !std::signbit(c) && phi == half_pi);
            if (std::isnan(P) || std::isnan(S)) EXPECT(S == T(0) || std::isnan(c)); // (S is never both)
            if (!std::isnan(c)) EXPECT(phi >= T(0) && phi <= pi);
        }
    EXPECT(ops::power_factor<T>(-T(0), T(1)) == T(0) && std::signbit(ops::power_factor<T>(-T(0), T(1))) && ops::acos_of(ops::power_factor<T>(-T(0), T(1))) == half_pi);
    EXPECT(ops::power_factor<T>(T(3), T(2)) == T(1) && ops::acos_of(T(1)) == T(0));
    EXPECT(ops::power_factor<T>(T(-5), T(2)) == T(-1) && ops::acos_of(T(-1)) == pi);
    const T inf = std::numeric_limits<T>::infinity();
    EXPECT(ops::power_factor<T>(T(1), inf) == T(0) && !std::signbit(ops::power_factor<T>(T(1), inf)));
    EXPECT(std::isnan(ops::power_factor<T>(inf, inf)) && std::isnan(ops::acos_of(ops::power_factor<T>(inf, inf))));
}

template <typename T, int N>
static void unbalance() {
    const auto        sp = specials<T>();
    const std::size_t m  = sp.size();
    std::size_t       total = 1, differ = 0;
    for (int k = 0; k < N; ++k) total *= m;
    const T inf = std::numeric_limits<T>::infinity();
    for (std::size_t idx = 0; idx < total; ++idx) {
        std::array<T, N> x;
        std::size_t      r = idx;
        for (int k = 0; k < N; ++k) { x[k] = sp[r % m]; r /= m; }
        const auto get = [&](int i) { return x[static_cast<std::size_t>(i)]; };
        const T    u = ops::voltage_unbalance<T>(get, N), c = ops::current_unbalance<T>(get, N), s = ops::sum_of<T>(get, N);
        sink += (u == u) + (c == c) + (s == s);
        bool any_nan = false, all_inf = true;
        for (T v : x) { any_nan = any_nan || std::isnan(v); all_inf = all_inf && v == inf; }
        if (any_nan) EXPECT(u == T(0) && c == T(0) && std::isnan(s)); // avg = NaN: 0
        if (!same_bits(u, c)) {
            ++differ;
            EXPECT(all_inf && u == T(0) && std::isnan(c)); // the one input on which the reference's two reductions disagree
        }
        const T avg = ops::mean_of<T>(s, N);
        if (!(avg > T(0))) EXPECT(u == T(0) && c == T(0));
        if (avg == inf && !all_inf) EXPECT(std::isnan(u) && std::isnan(c)); // (a finite phase, or the sum of finite phases overflowed)
    }
    EXPECT(differ == 1);
    const std::array<T, 3> z{-T(0), -T(0), -T(0)};
    const T                s = ops::sum_of<T>([&](int i) { return z[static_cast<std::size_t>(i)]; }, N);
    EXPECT(s == T(0) && !std::signbit(s)); // ((0 + -0) + -0) = +0
}

int main() {
    power_factor<float>();
    power_factor<double>();
    unbalance<float, 2>();
    unbalance<float, 3>();
    unbalance<double, 2>();
    unbalance<double, 3>();
    { // the reference QA's values (qa_PowerEstimators.cpp:236-237)
        const std::array<double, 3> U{230.0, 230.0 * 1.01f, 230.0 * 0.99f}, I{10.0, 10.0 * 1.02f, 10.0 * 0.98f};
        EXPECT(std::fabs(ops::voltage_unbalance<double>([&](int i) { return U[static_cast<std::size_t>(i)]; }, 3) - 1.0000013) < 1e-4);
        EXPECT(std::fabs(ops::current_unbalance<double>([&](int i) { return I[static_cast<std::size_t>(i)]; }, 3) - 1.9999981) < 1e-4);
    }
    std::printf("%s (%llu)\n", failures ? "FAILED" : "electrical_ops: all checks passed", sink);
    return failures ? 1 : 0;
}
