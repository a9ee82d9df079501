// The arithmetic rules of the converter blocks (gr4/converter_ops.hpp) on their edge cases, as a stand-alone program: tests/test_converter_host.py builds it with
// -fsanitize=address,undefined and runs it -- every conversion below is defined behaviour, also where the reference's static_cast is not.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include <gr4/converter_ops.hpp>

namespace ops = gr4::converter_ops;
static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

template <typename F>
static std::vector<F> float_specials() {
    using L = std::numeric_limits<F>;
    std::vector<F> v{F(0), -F(0), L::quiet_NaN(), L::infinity(), -L::infinity(), L::max(), -L::max(), L::min(), L::denorm_min(), F(0.5), F(-0.5), F(127.5), F(-128.5), F(255.9), F(256),
                     F(32767.5), F(-32768.9), F(65535.5), F(2147483648.0), F(-2147483648.0), F(4294967296.0), F(9223372036854775808.0), F(-9223372036854775808.0),
                     F(18446744073709551616.0), F(1e19), F(-1e19), F(1e30)};
    return v;
}
template <typename T>
static std::vector<T> int_specials() {
    using L = std::numeric_limits<T>;
    return {L::min(), L::max(), T(0), T(1), T(L::max() - 1), T(L::min() + 1), T(L::max() / 2), T(100), T(200 % (int)std::min<long long>(L::max(), 255)), T(-1)};
}
template <typename T>
static std::vector<T> specials() {
    if constexpr (std::is_floating_point_v<T>) return float_specials<T>();
    else return int_specials<T>();
}

static unsigned long long sink = 0; // keeps every result alive
template <typename T, typename R>
static void pair() {
    for (T x : specials<T>())
        for (T s : specials<T>()) {
            const R r = ops::cast<R>(ops::mul<T>(x, s));
            if constexpr (std::is_integral_v<R>) sink += (unsigned long long)r;
            else sink += r == r;
            if constexpr (std::is_floating_point_v<T> && std::is_integral_v<R>) {
                const auto p = ops::mul<T>(x, s);
                if (p != p) EXPECT(r == R(0));
                else if (p >= (decltype(p))std::numeric_limits<R>::max()) EXPECT(r == std::numeric_limits<R>::max());
                else if (p <= (decltype(p))std::numeric_limits<R>::min()) EXPECT(r == std::numeric_limits<R>::min());
                else EXPECT((decltype(p))r == std::trunc(p));
            }
        }
    if constexpr (std::is_integral_v<T>)
        for (T x : specials<T>()) sink += (unsigned long long)ops::abs_int<T>(x);
}
template <typename T>
static void from() {
    pair<T, std::uint8_t>(); pair<T, std::uint16_t>(); pair<T, std::uint32_t>(); pair<T, std::uint64_t>();
    pair<T, std::int8_t>(); pair<T, std::int16_t>(); pair<T, std::int32_t>(); pair<T, std::int64_t>();
    pair<T, float>(); pair<T, double>();
}

int main() {
    from<std::uint8_t>(); from<std::uint16_t>(); from<std::uint32_t>(); from<std::uint64_t>();
    from<std::int8_t>(); from<std::int16_t>(); from<std::int32_t>(); from<std::int64_t>();
    from<float>(); from<double>();
    EXPECT(ops::cast<float>(ops::mul<std::uint8_t>(200, 200)) == 40000.0f);
    EXPECT(ops::cast<std::int32_t>(ops::mul<std::int16_t>(-300, 300)) == -90000 && ops::cast<std::int16_t>(ops::mul<std::int16_t>(-300, 300)) == -24464);
    EXPECT(ops::cast<float>(std::int64_t((1ll << 60) + (1ll << 36) + 1)) == 0x1.000002p+60f);
    EXPECT(ops::cast<std::int64_t>(ops::mul<std::uint16_t>(65535, 65535)) == 65535ll * 65535ll - (1ll << 32));
    EXPECT(ops::mul<std::int32_t>(std::numeric_limits<std::int32_t>::max(), 2) == -2 && ops::mul<std::int64_t>(1ll << 62, 4) == 0);
    EXPECT(ops::abs_int<std::uint8_t>(200) == 56 && ops::abs_int<std::int8_t>(-128) == -128 && ops::abs_int<std::int32_t>(std::numeric_limits<std::int32_t>::min()) == std::numeric_limits<std::int32_t>::min());
    EXPECT(ops::cast<std::int8_t>(127.9f) == 127 && ops::cast<std::int8_t>(-128.9f) == -128 && ops::cast<std::int8_t>(1e10f) == 127 && ops::cast<std::uint8_t>(-1.9f) == 0);
    EXPECT(ops::cast<std::uint64_t>(1e19) == 10000000000000000000ull && ops::cast<std::uint64_t>(18446744073709551616.0) == std::numeric_limits<std::uint64_t>::max());
    EXPECT(ops::cast<std::int16_t>(std::nan("")) == 0);
    std::printf("%s (%llu)\n", failures ? "FAILED" : "converter_ops: all checks passed", sink);
    return failures ? 1 : 0;
}
