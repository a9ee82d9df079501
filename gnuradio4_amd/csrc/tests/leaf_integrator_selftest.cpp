// leaf_integrator_selftest.cpp -- the geometry and the emit step of csrc/leaf_integrator.hpp on the host (tests/test_leaf_integrator_host.py builds and runs it;
// host side of a HIP compile: hipcc -x hip --cuda-host-only).  Two checks, each for leaves of 32 and of 64 frames; the first mismatch is printed with the
// tuple it belongs to and the program exits 1.
//   1. geometry, exhaustive: leaf_geom and leaf_range against a walk over the call's frames
//   2. fold: a stream cut into calls, each folded on the CPU with leaf_emit_element over [nq][M], against the uncut definition, bit for bit, the carry included
#include "../leaf_integrator.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace gr4;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }
static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

// ---- check 1.  Frame f of the call is frame pos + f of its first integration: integration q = F / A, leaf l = (F % A) / LEAF, leaf number K = q lpi + l.
template <int LEAF>
static int check_geometry() {
    const long lengths[] = {1, 2, LEAF - 1, LEAF, LEAF + 1, 2 * LEAF, 2 * LEAF + 3};
    long       cases = 0;
    for (const long A : lengths) {
        const long lpi = (A + LEAF - 1) / LEAF;
        for (long pos = 0; pos < A; ++pos) {
            for (long n = 1; n <= 2 * A + LEAF + 1; ++n, ++cases) {
                std::vector<long> first, count; // per touched leaf, in the order of the walk
                long              K_first = -1, K_prev = -1, q_last = 0;
                for (long f = 0; f < n; ++f) {
                    const long F = pos + f, q = F / A, l = (F % A) / LEAF, K = q * lpi + l;
                    if (f == 0) K_first = K;
                    if (K != K_prev) { first.push_back(f); count.push_back(0); }
                    ++count.back();
                    K_prev = K;
                    q_last = q;
                }
                const LeafGeom<LEAF> g = leaf_geom<LEAF>(pos, n, A);
                if (g.pos != pos || g.n != n || g.A != A || g.lpi != lpi || g.k0 != K_first || g.nl != (long)first.size() || g.nq != q_last + 1) {
                    std::printf("geometry LEAF=%d A=%ld pos=%ld n=%ld: leaf_geom gives lpi=%ld k0=%ld nl=%ld nq=%ld, the walk lpi=%ld k0=%ld nl=%zu nq=%ld\n", LEAF, A, pos, n, g.lpi,
                                g.k0, g.nl, g.nq, lpi, K_first, first.size(), q_last + 1);
                    return 1;
                }
                long next = 0; // the ranges tile the call: each starts where the one before ended, the last ends at n
                for (long k = 0; k < g.nl; ++k) {
                    long got_first;
                    int  got_count;
                    bool got_complete;
                    leaf_range(g, k, &got_first, &got_count, &got_complete);
                    const long K = K_first + k, q = K / lpi, l = K % lpi;
                    const long leaf_last = std::min(q * A + (l + 1) * LEAF, (q + 1) * A) - 1; // the leaf's last frame
                    const bool complete  = leaf_last <= pos + n - 1;
                    if (got_first != first[k] || got_count != count[k] || got_complete != complete || got_first != next) {
                        std::printf("geometry LEAF=%d A=%ld pos=%ld n=%ld k=%ld: leaf_range gives first=%ld count=%d complete=%d, the walk first=%ld count=%ld complete=%d (tiling: %ld)\n",
                                    LEAF, A, pos, n, k, got_first, got_count, (int)got_complete, first[k], count[k], (int)complete, next);
                        return 1;
                    }
                    next = got_first + got_count;
                }
                if (next != n) { std::printf("geometry LEAF=%d A=%ld pos=%ld n=%ld: the ranges end at %ld\n", LEAF, A, pos, n, next); return 1; }
            }
        }
    }
    std::printf("geometry LEAF=%d: %ld calls ok\n", LEAF, cases);
    return 0;
}

// ---- check 2.  Rows of M floats; HERMITIAN: S = 2 streams, N = 2 bins, P = 3 baselines, M = 2 P N = 12 interleaved complex values, the diagonal p = 0 and 2.
struct Carry {
    std::vector<double> acc[2];
    std::vector<float>  leaf[2];
    int                 cur = 0;
    long                pos = 0;
};

// one call, as the device runs it: the leaves by a plain float32 loop (the call's first from the carried running leaf), then the emit body over [nq][M]
template <int LEAF, bool HERMITIAN>
static long cpu_call(Carry& c, const float* x, long n, long A, long M, int N, int mean, float* out) {
    const LeafGeom<LEAF> g = leaf_geom<LEAF>(c.pos, n, A);
    std::vector<float>   leaves((size_t)(g.nl * M));
    for (long k = 0; k < g.nl; ++k) {
        long first;
        int  count;
        bool complete;
        leaf_range(g, k, &first, &count, &complete);
        for (long e = 0; e < M; ++e) {
            float a = k == 0 ? c.leaf[c.cur][e] : 0.f;
            for (int j = 0; j < count; ++j) a = a + x[(first + j) * M + e];
            leaves[k * M + e] = a;
        }
    }
    for (long i = 0; i < g.nq * M; ++i)
        leaf_emit_element<LEAF, HERMITIAN>(i, leaves.data(), g, c.acc[c.cur].data(), c.acc[c.cur ^ 1].data(), c.leaf[c.cur ^ 1].data(), out, M, N, mean);
    c.cur ^= 1;
    const long done = (c.pos + n) / A;
    c.pos           = (c.pos + n) % A;
    return done;
}

template <int LEAF, bool HERMITIAN>
static int check_fold(long M, int N, long& shapes) {
    const long lengths[] = {1, LEAF - 1, LEAF, LEAF + 1, 2 * LEAF + 3};
    for (const long A : lengths) {
        // three integrations and the start of a fourth: a complete leaf and three frames of the next where A has room for them
        const long T = 3 * A + std::min<long>(A - 1, LEAF + 3), rows = T / A, tail = T % A;
        for (int mean = 0; mean < 2; ++mean) {
            for (int seq = 0; seq < 5; ++seq, ++shapes) {
                std::vector<float> x((size_t)(T * M));
                for (auto& v : x) { // positive, 17 binades apart: the order of the additions shows in the last bits, and no sum is zero
                    const uint64_t r = rnd();
                    v = (0.5f + (float)(r >> 40) * 0x1p-24f) * std::ldexp(1.f, (int)(r % 17) - 8);
                }
                // the uncut definition: float32 leaf sums from +0, a float64 fold ascending, one rounding; the carry of an unfinished integration
                std::vector<float>  want((size_t)(rows * M)), want_leaf((size_t)M, 0.f);
                std::vector<double> want_acc((size_t)M, 0.0);
                for (long q = 0; q <= rows; ++q) {
                    const long frames = q < rows ? A : tail;
                    for (long e = 0; e < M; ++e) {
                        double acc = 0.0;
                        for (long l0 = 0; l0 < frames; l0 += LEAF) {
                            const long l1 = std::min<long>(l0 + LEAF, A);
                            float      s  = 0.f;
                            for (long f = l0; f < std::min(l1, frames); ++f) s = s + x[(q * A + f) * M + e];
                            if (l1 <= frames) acc = acc + (double)s;
                            else want_leaf[e] = s; // the running leaf
                        }
                        if (q < rows) want[q * M + e] = mean ? (float)(acc / (double)A) : (float)acc;
                        else want_acc[e] = acc;
                    }
                }
                if (HERMITIAN) {
                    for (long q = 0; q < rows; ++q) {
                        for (long i = 0; i < 2; ++i) // S = 2
                            for (long b = 0; b < N; ++b) want[q * M + ((i * (i + 3) / 2) * N + b) * 2 + 1] = 0.f;
                        for (long e = 0; e < M; ++e) {
                            const long p = e / (2 * N);
                            const bool diag_im = (e & 1) && (p == 0 || p == 2);
                            if (!diag_im && bits(want[q * M + e]) << 1 == 0) { std::printf("fold: the definition itself gives 0 at row %ld element %ld\n", q, e); return 1; }
                        }
                    }
                }
                // the cuts: random ones, one at a leaf's end (inside an integration where a leaf is shorter than it) and one at an integration's end
                std::vector<long> cuts{0, T, (A > LEAF ? A + LEAF : A), 2 * A};
                const int         extra = 1 + (int)(rnd() % 6);
                for (int u = 0; u < extra; ++u) cuts.push_back(1 + (long)(rnd() % (uint64_t)(T - 1))); // T >= 3
                std::sort(cuts.begin(), cuts.end());
                cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());

                Carry c;
                for (int h = 0; h < 2; ++h) { c.acc[h].assign((size_t)M, 0.0); c.leaf[h].assign((size_t)M, 0.f); }
                std::vector<float> got((size_t)(rows * M));
                std::memset(got.data(), 0xff, got.size() * sizeof(float)); // (never written would show)
                long row = 0;
                for (size_t u = 0; u + 1 < cuts.size(); ++u)
                    row += cpu_call<LEAF, HERMITIAN>(c, x.data() + cuts[u] * M, cuts[u + 1] - cuts[u], A, M, N, mean, got.data() + row * M);

                const auto where = [&]() {
                    std::printf("fold LEAF=%d hermitian=%d M=%ld A=%ld mean=%d sequence %d, cuts at", LEAF, (int)HERMITIAN, M, A, mean, seq);
                    for (const long cut : cuts) std::printf(" %ld", cut);
                };
                if (row != rows) { where(); std::printf(": %ld rows, expected %ld\n", row, rows); return 1; }
                for (long i = 0; i < rows * M; ++i)
                    if (bits(got[i]) != bits(want[i])) { where(); std::printf(": row %ld element %ld is %08x, the definition %08x\n", i / M, i % M, bits(got[i]), bits(want[i])); return 1; }
                for (long e = 0; e < M; ++e) {
                    if (bits(c.acc[c.cur][e]) != bits(want_acc[e])) { where(); std::printf(": carried sum %ld is %016llx, the definition %016llx\n", e, (unsigned long long)bits(c.acc[c.cur][e]), (unsigned long long)bits(want_acc[e])); return 1; }
                    if (bits(c.leaf[c.cur][e]) != bits(want_leaf[e])) { where(); std::printf(": carried leaf %ld is %08x, the definition %08x\n", e, bits(c.leaf[c.cur][e]), bits(want_leaf[e])); return 1; }
                }
            }
        }
    }
    return 0;
}

template <int LEAF>
static int check_leaf() {
    if (check_geometry<LEAF>()) return 1;
    long shapes = 0;
    if (check_fold<LEAF, false>(6, 0, shapes) || check_fold<LEAF, false>(14, 0, shapes) || check_fold<LEAF, true>(12, 2, shapes)) return 1;
    std::printf("fold LEAF=%d: %ld cut streams ok\n", LEAF, shapes);
    return 0;
}

int main() { return check_leaf<32>() || check_leaf<64>(); }
