// fir_cplx.hip -- complex taps x complex data FIR, direct and decimating, for gfx950 ("complex-tap variant as an option"; COMPLEX_FIR.md).
//
// The reference has no such block (its fir_filter is `requires std::floating_point<T>`): like the interpolating FIR the definition is the project's own and its
// float64 oracle (tests/complex_fir_oracle.py) pins it:
//     y[n] = sum_{k < K} b[k] x[n - k],   b and x complex<float>, every complex product as four real products; decim D: output m = y[m D]
// zero initial history, the last K - 1 inputs carried across calls.  Three kernels:
//  * cfir_mfma_f32_kernel: the realified band form on v_mfma_f32_16x16x4_f32 (exact f32 products, one rounding per product).  With x'[2n] = Re x[n], x'[2n + 1] = Im x[n],
//        y'[2o + p] = sum_{j = -1}^{2K - 1} g_p[j] x'[2 D o + p - j],   g_0[2k] = Re b[k], g_0[2k - 1] = -Im b[k], g_1[2k] = Re b[k], g_1[2k + 1] = Im b[k]
//    a 16 x 16 tile (row i = 2 io + p, column c) holds the 128 complex outputs o0 + 8 c + io and is  Y = sum_r A_r B_r  with
//        A_r[i][u] = g_p[2 D io + p - (16 r + u)],   B_r[u][c] = x'[2 D o0 + 16 (D c + r) + u],   r = floor(-(2K - 1) / 16) .. floor((14 D + 2) / 16)
//    B is the staged stream itself (16-float chunks at a column stride of D chunks: the decimation sits in the tap operand), A holds copies and sign flips of the
//    taps and is built on the host (cf_band below; gr4hip_cfir_band_table hands it out).  A workgroup of four waves owns a tile group of 8 tiles = 1024 outputs, two
//    tiles (two independent accumulators) per wave.  The chunks are staged de-interleaved into D rows (chunk q -> row q % D, index q / D), so the 16 columns of a
//    step read 16 consecutive chunks of one row whatever D is; inside a row bit 2 of the chunk index is folded into the quarter index, which makes the ds_read_b128
//    of the B operand conflict-free (its lane groups mix columns 0-3, 12-15 of k-group 0 with columns 4-11 of k-group 1).  The contraction index inside a chunk is
//    taken as u = 4 kq + s (lane k-group kq, MFMA step s): one 16-byte read per lane feeds the four MFMAs of a step, for B and for A alike.
//    The tap operand sits in LDS up to 256 taps while two workgroups per CU still fit, and is streamed from the L2 (one prefetched 16-byte load per lane and step) otherwise.
//  * cfir_direct_kernel: IEEE float32 multiply-add, k ascending, straight from global memory: K <= 16, K > 1024, D > 16, spans below one tile group, the ragged tail.
//  * cfir_exact_kernel: the guard's second evaluation (include/gr4hip.h, "ONE guard"): float64 sum in ascending k, rounded once, for the segments the main
//    kernels marked -- D P_y < (sum |b|^2 / 128) P_x, or a non-finite sample in what the segment read -- behind the launch on the same stream, no host wait.
#include "common.hpp"
#include "history.hpp"

#include <algorithm>
#include <cmath>

namespace gr4 {

using cf_f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int    kCfSeg   = 1024; // complex outputs per workgroup: the tile group of the matrix-pipe kernel and the guard segment
constexpr size_t kCfMaxK  = 2048, kCfMaxD = 64;
constexpr size_t kCfLdsMax = 160 * 1024;

// stream position pos relative to this call's first sample: the carried history in front, zeros in front of that and past the end
__device__ __forceinline__ float2 cf_sample(const float2* __restrict__ x, const float2* __restrict__ hist, int hcap, long pos, long n_in) {
    if (pos >= 0) return pos < n_in ? x[pos] : make_float2(0.f, 0.f);
    return pos >= -(long)hcap ? hist[hcap + pos] : make_float2(0.f, 0.f);
}
__device__ __forceinline__ bool cf_non_finite(float2 v) { return !(__builtin_isfinite(v.x) && __builtin_isfinite(v.y)); }

// the segment's verdict: every lane brings its share of P_x, P_y and whether it saw a non-finite sample; red: 8 floats of LDS
__device__ __forceinline__ void cf_verdict(float px, float py, bool nf, float thr, int D, unsigned char* __restrict__ flags, unsigned long long* __restrict__ count, long seg, float* red) {
    for (int o = 32; o > 0; o >>= 1) { px += __shfl_xor(px, o); py += __shfl_xor(py, o); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave] = px; red[4 + wave] = py; }
    const int any_nf = __syncthreads_or(nf ? 1 : 0);
    if (threadIdx.x == 0) {
        const float sx = (red[0] + red[1]) + (red[2] + red[3]), sy = (red[4] + red[5]) + (red[6] + red[7]);
        const bool  m  = any_nf != 0 || (float)D * sy < thr * sx;
        flags[seg]     = m ? 1 : 0;
        if (m) atomicAdd(count, 1ull);
    }
}

// tabk: [n_steps][64 lanes] float4 = A_r[lane & 15][4 (lane >> 4) + s], s = 0 .. 3.  xs: D rows of RS floats; row stride and the rows' length TR (chunks) from the host.
template <bool A_LDS>
__global__ __launch_bounds__(256) void cfir_mfma_f32_kernel(const float2* __restrict__ x, const float2* __restrict__ hist, int hcap, const float4* __restrict__ tabk, int n_steps, int r_min,
                                                            int D, int RS, int TR, float2* __restrict__ y, long n_in, float thr, unsigned char* __restrict__ flags, unsigned long long* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) float cf_sm[];
    float*    xs  = cf_sm;
    float*    red = cf_sm + D * RS;
    float4*   al  = reinterpret_cast<float4*>(cf_sm + D * RS + 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, kq = lane >> 4;
    const long o0 = (long)blockIdx.x * kCfSeg;
    float      px = 0.f;
    bool       nf = false;
    { // staging: chunk q' (8 complex samples from stream position D o0 + 8 r_min + 8 q') -> row q' % D, index t = q' / D; a thread walks chunks 32 apart
        const long s0 = (long)D * o0 + 8L * r_min, in0 = (long)D * o0, in1 = in0 + (long)D * kCfSeg;
        const int  w = tid & 7, drow = 32 % D, dt = 32 / D, nch = D * TR;
        int        q = tid >> 3, row = q % D, t = q / D;
#pragma unroll 4
        for (; q < nch; q += 32) {
            const long   pos = s0 + 8L * q + w;
            const float2 v   = cf_sample(x, hist, hcap, pos, n_in);
            nf |= cf_non_finite(v);
            if (pos >= in0 && pos < in1) px = fmaf(v.x, v.x, fmaf(v.y, v.y, px));
            const int off = 16 * t + 2 * w;
            *reinterpret_cast<float2*>(xs + row * RS + (off ^ ((t << 1) & 8))) = v;
            row += drow;
            t += dt;
            if (row >= D) { row -= D; ++t; }
        }
    }
    if constexpr (A_LDS)
        for (int i = tid; i < n_steps * 64; i += 256) al[i] = tabk[i];
    __syncthreads();

    auto lda = [&](int r) -> float4 {
        if constexpr (A_LDS) return al[r * 64 + lane];
        else return tabk[r * 64 + lane];
    };
    cf_f32x4  acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int tl = 16 * (2 * wave) + c; // this lane's column of the wave's first tile (the second: + 16)
    int       row = 0, t0 = 0;
    float4    an = lda(0);
    for (int r = 0; r < n_steps; ++r) {
        const float4 a = an;
        if (r + 1 < n_steps) an = lda(r + 1);
        const float* xr = xs + row * RS;
        const int    b0 = 16 * (tl + t0) + 4 * kq, sw = (b0 >> 3) & 8; // (+ 256 floats for the second tile: bit 6 unchanged)
        const float4 v0 = *reinterpret_cast<const float4*>(xr + (b0 ^ sw));
        const float4 v1 = *reinterpret_cast<const float4*>(xr + ((b0 + 256) ^ sw));
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, v0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, v1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, v0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, v1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, v0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, v1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, v0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, v1.w, acc1, 0, 0, 0);
        if (++row == D) { row = 0; ++t0; }
    }
    // D[row 4 kq + reg][column c]: rows 2 io + p -> registers (0, 1) = output io = 2 kq, (2, 3) = output 2 kq + 1 of column c
    const long o = o0 + 8L * tl + 2 * kq;
    y[o]           = make_float2(acc0[0], acc0[1]);
    y[o + 1]       = make_float2(acc0[2], acc0[3]);
    y[o + 128]     = make_float2(acc1[0], acc1[1]);
    y[o + 128 + 1] = make_float2(acc1[2], acc1[3]);
    if (flags != nullptr) {
        float py = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) py = fmaf(acc0[i], acc0[i], fmaf(acc1[i], acc1[i], py));
        cf_verdict(px, py, nf, thr, D, flags, count, (long)blockIdx.x, red);
    }
}

// one workgroup per segment, four outputs per lane (tid + 256 i)
__global__ __launch_bounds__(256) void cfir_direct_kernel(const float2* __restrict__ x, const float2* __restrict__ hist, int hcap, const float2* __restrict__ taps, int K, int D,
                                                          float2* __restrict__ y, long n_in, long seg_first, float thr, unsigned char* __restrict__ flags, unsigned long long* __restrict__ count) {
    __shared__ float red[8];
    const long seg = seg_first + blockIdx.x, o0 = seg * kCfSeg, n_out = n_in / D;
    float      re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
    const long p0 = (long)D * (o0 + threadIdx.x), dp = (long)D * 256;
    for (int k = 0; k < K; ++k) {
        const float2 b = taps[k]; // wave-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 v = cf_sample(x, hist, hcap, p0 + i * dp - k, n_in);
            re[i] = fmaf(b.x, v.x, re[i]);
            re[i] = fmaf(-b.y, v.y, re[i]);
            im[i] = fmaf(b.x, v.y, im[i]);
            im[i] = fmaf(b.y, v.x, im[i]);
        }
    }
    float py = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long o = o0 + threadIdx.x + 256 * i;
        if (o < n_out) {
            y[o] = make_float2(re[i], im[i]);
            py   = fmaf(re[i], re[i], fmaf(im[i], im[i], py));
        }
    }
    if (flags != nullptr) {
        const long in0 = (long)D * o0, in1 = in0 + (long)D * kCfSeg < n_in ? in0 + (long)D * kCfSeg : n_in;
        float      px = 0.f;
        bool       nf = false;
        for (long pos = in0 - (K - 1) + threadIdx.x; pos < in1; pos += 256) {
            const float2 v = cf_sample(x, hist, hcap, pos, n_in);
            nf |= cf_non_finite(v);
            if (pos >= in0) px = fmaf(v.x, v.x, fmaf(v.y, v.y, px));
        }
        cf_verdict(px, py, nf, thr, D, flags, count, seg, red);
    }
}

__global__ __launch_bounds__(256) void cfir_exact_kernel(const float2* __restrict__ x, const float2* __restrict__ hist, int hcap, const float2* __restrict__ taps, int K, int D,
                                                         float2* __restrict__ y, long n_in, const unsigned char* __restrict__ flags) {
    const long seg = blockIdx.x;
    if (!flags[seg]) return;
    const long n_out = n_in / D;
    for (int i = 0; i < 4; ++i) {
        const long o = seg * kCfSeg + threadIdx.x + 256 * i;
        if (o >= n_out) continue;
        double     re = 0.0, im = 0.0;
        const long p  = (long)D * o;
        for (int k = 0; k < K; ++k) {
            const float2 b = taps[k];
            const float2 v = cf_sample(x, hist, hcap, p - k, n_in);
            re = fma((double)b.x, (double)v.x, re);
            re = fma(-(double)b.y, (double)v.y, re);
            im = fma((double)b.x, (double)v.y, im);
            im = fma((double)b.y, (double)v.x, im);
        }
        y[o] = make_float2((float)re, (float)im);
    }
}

// g_p[j] of the band form (0 outside -1 .. 2K - 1)
static float cf_g(const float* b, long K, int p, long j) {
    if (j < -1 || j > 2 * K - 1) return 0.f;
    if ((j & 1) == 0) return b[j]; // j = 2k: Re b[k]
    const long k = p == 0 ? (j + 1) / 2 : (j - 1) / 2;
    if (k < 0 || k >= K) return 0.f;
    return p == 0 ? -b[2 * k + 1] : b[2 * k + 1];
}
// A: [n_steps][16 rows i = 2 io + p][16 u]
static void cf_band(const float* b, size_t K, size_t D, std::vector<float>& A, int& n_steps, long& r_min) {
    r_min            = -(long)((2 * K + 14) / 16); // floor(-(2K - 1) / 16)
    const long r_max = (long)((14 * D + 2) / 16);
    n_steps          = (int)(r_max - r_min + 1);
    A.assign((size_t)n_steps * 256, 0.f);
    for (long r = r_min; r <= r_max; ++r)
        for (int i = 0; i < 16; ++i)
            for (int u = 0; u < 16; ++u) A[(size_t)(r - r_min) * 256 + i * 16 + u] = cf_g(b, (long)K, i & 1, 2 * (long)D * (i >> 1) + (i & 1) - (16 * r + u));
}

} // namespace gr4

using namespace gr4;

struct gr4hip_cfir {
    size_t             ntaps = 0, D = 1, hcap = 32;
    std::vector<float> taps, tabk_host; // the host images the stream-ordered uploads read: interleaved taps, the kernel-order tap operand
    DeviceBuffer       d_taps, d_tabk, d_flags, d_count;
    CarriedHistory     hist; // hcap complex samples
    int                n_steps = 0, guard_mode = GR4HIP_GUARD_STRICT;
    long               r_min = 0;
    double             tap_power = 0.0;
    bool               taps_dirty = false, counted = false;
    unsigned           last_paths = 0; // bit 0: matrix-pipe kernel, bit 1: direct kernel, bit 2: exact kernel enqueued
    unsigned long long marked_host = 0;
};

static int cf_check_taps(const char* who, const float* h_taps, size_t ntaps, size_t decim) {
    GR4_REQUIRE(h_taps, "%s: null taps", who);
    GR4_REQUIRE(ntaps >= 1, "%s: need at least one tap", who);
    GR4_REQUIRE(decim >= 1, "%s: decim must be >= 1", who);
    for (size_t i = 0; i < 2 * std::min(ntaps, kCfMaxK); ++i) GR4_REQUIRE(std::isfinite(h_taps[i]), "%s: tap %zu is not finite", who, i / 2);
    if (ntaps > kCfMaxK || decim > kCfMaxD) {
        set_error("%s: %zu taps, decim %zu: supported up to %zu taps and decim %zu", who, ntaps, decim, kCfMaxK, kCfMaxD);
        return GR4HIP_UNSUPPORTED;
    }
    return GR4HIP_OK;
}

static int cf_upload(gr4hip_cfir* f) {
    std::vector<float> A;
    cf_band(f->taps.data(), f->ntaps, f->D, A, f->n_steps, f->r_min);
    f->tabk_host.resize(A.size());
    for (int r = 0; r < f->n_steps; ++r)
        for (int lane = 0; lane < 64; ++lane)
            for (int s = 0; s < 4; ++s) f->tabk_host[(size_t)r * 256 + lane * 4 + s] = A[(size_t)r * 256 + (lane & 15) * 16 + 4 * (lane >> 4) + s];
    f->tap_power = 0.0;
    for (float v : f->taps) f->tap_power += (double)v * v;
    int rc = f->d_taps.ensure(f->taps.size() * sizeof(float)); // (growing frees the old table: hipFree waits for the device)
    if (!rc) rc = f->d_tabk.ensure(f->tabk_host.size() * sizeof(float));
    if (rc) return rc;
    f->taps_dirty = true; // uploaded by cf_state_on, on the stream of the next call
    return GR4HIP_OK;
}
static int cf_state_on(gr4hip_cfir* f, hipStream_t st) {
    if (f->taps_dirty) {
        GR4_HIP_TRY(hipMemcpyAsync(f->d_taps.ptr, f->taps.data(), f->taps.size() * sizeof(float), hipMemcpyHostToDevice, st));
        GR4_HIP_TRY(hipMemcpyAsync(f->d_tabk.ptr, f->tabk_host.data(), f->tabk_host.size() * sizeof(float), hipMemcpyHostToDevice, st));
        f->taps_dirty = false;
    }
    return f->hist.on(st);
}

// row length (chunks), row stride (floats) and LDS bytes of the matrix-pipe kernel
static size_t cf_mfma_lds(const gr4hip_cfir* f, bool a_lds, int* TR, int* RS) {
    *TR = 128 + (f->n_steps - 1) / (int)f->D;
    *RS = (16 * *TR + 63) / 64 * 64;
    return (f->D * (size_t)*RS + 16 + (a_lds ? (size_t)f->n_steps * 256 : 0)) * sizeof(float);
}

extern "C" {

size_t gr4hip_cfir_tile(void) { return kCfSeg; }
size_t gr4hip_cfir_segment(void) { return kCfSeg; }

int gr4hip_cfir_band_table(const float* h_taps, size_t ntaps, size_t decim, float* h_out, size_t cap, size_t* n_steps, long* r_min) {
    if (const int rc = cf_check_taps("cfir_band_table", h_taps, ntaps, decim)) return rc;
    std::vector<float> A;
    int                ns = 0;
    long               r0 = 0;
    cf_band(h_taps, ntaps, decim, A, ns, r0);
    if (n_steps) *n_steps = (size_t)ns;
    if (r_min) *r_min = r0;
    if (h_out) {
        GR4_REQUIRE(cap >= A.size(), "cfir_band_table: room for %zu floats, the operand has %zu", cap, A.size());
        std::copy(A.begin(), A.end(), h_out);
    }
    return GR4HIP_OK;
}

int gr4hip_cfir_create(gr4hip_cfir_t** out, const float* h_taps, size_t ntaps, size_t decim) {
    GR4_REQUIRE(out, "cfir: null output handle");
    if (const int rc = cf_check_taps("cfir", h_taps, ntaps, decim)) return rc;
    if (const int rc = have_device("cfir")) return rc;
    auto* f = new (std::nothrow) gr4hip_cfir();
    GR4_REQUIRE(f, "out of host memory");
    f->D     = decim;
    f->ntaps = ntaps;
    f->taps.assign(h_taps, h_taps + 2 * ntaps);
    f->hcap = std::max<size_t>(32, bit_ceil(ntaps));
    int rc  = cf_upload(f);
    if (!rc) rc = f->hist.resize(f->hcap * sizeof(float2));
    if (!rc) rc = f->d_count.ensure(sizeof(unsigned long long));
    if (rc) { delete f; return rc; }
    *out = f;
    return GR4HIP_OK;
}

int gr4hip_cfir_set_taps(gr4hip_cfir_t* f, const float* h_taps, size_t ntaps) {
    GR4_REQUIRE(f, "cfir_set_taps: null handle");
    if (const int rc = cf_check_taps("cfir_set_taps", h_taps, ntaps, f->D)) return rc;
    f->taps.assign(h_taps, h_taps + 2 * ntaps);
    f->ntaps = ntaps;
    if (const int rc = cf_upload(f)) return rc;
    if (ntaps > f->hcap) { // like fir_filter::settingsChanged: the history is replaced (lost) only when it must grow
        f->hcap = bit_ceil(ntaps);
        return f->hist.resize(f->hcap * sizeof(float2));
    }
    return GR4HIP_OK;
}

int gr4hip_cfir_reset(gr4hip_cfir_t* f) {
    GR4_REQUIRE(f, "cfir_reset: null handle");
    f->hist.reset(); // cf_state_on zeroes the history on the stream of the next call
    return GR4HIP_OK;
}

int gr4hip_cfir_set_guard_mode(gr4hip_cfir_t* f, int mode) {
    GR4_REQUIRE(f, "cfir_set_guard_mode: null handle");
    GR4_REQUIRE(mode >= GR4HIP_GUARD_STRICT && mode <= GR4HIP_GUARD_OFF, "cfir_set_guard_mode: unknown mode %d", mode);
    if (mode == GR4HIP_GUARD_DEFERRED) {
        set_error("cfir_set_guard_mode: the redo runs behind every launch, there is nothing to defer (STRICT or OFF)");
        return GR4HIP_UNSUPPORTED;
    }
    f->guard_mode = mode;
    return GR4HIP_OK;
}

int gr4hip_cfir_process(gr4hip_cfir_t* f, const void* d_in, size_t n_in, void* d_out, size_t* n_out_p, gr4hip_stream_t stream) {
    GR4_REQUIRE(f, "cfir_process: null handle");
    GR4_REQUIRE(n_in % f->D == 0, "cfir_process: n_in (%zu) must be a multiple of decim (%zu)", n_in, f->D);
    const size_t n_out = n_in / f->D;
    if (n_out_p) *n_out_p = n_out;
    f->last_paths = 0;
    f->counted    = false;
    if (n_in == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in && d_out, "cfir_process: null device pointer");
    GR4_REQUIRE((uintptr_t)d_in % 8 == 0 && (uintptr_t)d_out % 8 == 0, "cfir_process: buffers must be aligned to 8 bytes");
    {
        const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + n_in * sizeof(float2), b0 = (uintptr_t)d_out, b1 = b0 + n_out * sizeof(float2);
        GR4_REQUIRE(a1 <= b0 || b1 <= a0, "cfir_process: d_in and d_out overlap");
    }
    hipStream_t  st      = as_stream(stream);
    const bool   guarded = f->guard_mode != GR4HIP_GUARD_OFF;
    const size_t n_seg = ceil_div(n_out, (size_t)kCfSeg), n_full = n_out / kCfSeg;
    if (guarded)
        if (const int rc = f->d_flags.ensure(n_seg)) return rc;
    if (const int rc = cf_state_on(f, st)) return rc;
    GR4_HIP_TRY(hipMemsetAsync(f->d_count.ptr, 0, sizeof(unsigned long long), st));
    const float2*       x     = static_cast<const float2*>(d_in);
    float2*             y     = static_cast<float2*>(d_out);
    const float2*       hist  = static_cast<const float2*>(f->hist.current());
    const float2*       taps  = static_cast<const float2*>(f->d_taps.ptr);
    unsigned char*      flags = guarded ? static_cast<unsigned char*>(f->d_flags.ptr) : nullptr;
    unsigned long long* count = static_cast<unsigned long long*>(f->d_count.ptr);
    const float         thr   = (float)(f->tap_power / 128.0);
    const int           K = (int)f->ntaps, D = (int)f->D;

    size_t done = 0; // segments the matrix-pipe kernel took
    if (K >= 17 && K <= 1024 && D <= 16 && n_full >= 1) {
        int          TR = 0, RS = 0;
        bool         a_lds = K <= 256;
        size_t       lds   = cf_mfma_lds(f, a_lds, &TR, &RS);
        if (a_lds && 2 * lds > kCfLdsMax) { a_lds = false; lds = cf_mfma_lds(f, false, &TR, &RS); } // (decimators: the staged stream is D times as long, and a second
                                                                                                   // workgroup per CU -- one stages while the other multiplies -- is worth more than the operand in LDS)
        if (lds <= kCfLdsMax) {
            auto kern = a_lds ? cfir_mfma_f32_kernel<true> : cfir_mfma_f32_kernel<false>;
            if (lds > 48 * 1024) GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)n_full), dim3(256), lds, st, x, hist, (int)f->hcap, static_cast<const float4*>(f->d_tabk.ptr), f->n_steps, (int)f->r_min, D, RS, TR, y,
                               (long)n_in, thr, flags, count);
            GR4_LAUNCH_CHECK();
            done = n_full;
            f->last_paths |= 1u;
        }
    }
    if (done < n_seg) {
        hipLaunchKernelGGL(cfir_direct_kernel, dim3((unsigned)(n_seg - done)), dim3(256), 0, st, x, hist, (int)f->hcap, taps, K, D, y, (long)n_in, (long)done, thr, flags, count);
        GR4_LAUNCH_CHECK();
        f->last_paths |= 2u;
    }
    if (guarded) {
        hipLaunchKernelGGL(cfir_exact_kernel, dim3((unsigned)n_seg), dim3(256), 0, st, x, hist, (int)f->hcap, taps, K, D, y, (long)n_in, flags);
        GR4_LAUNCH_CHECK();
        f->last_paths |= 4u;
    }
    if (const int rc = f->hist.advance(x, n_in, f->hcap, (int)sizeof(float2), st)) return rc;
    f->counted = true;
    return GR4HIP_OK;
}

int gr4hip_cfir_destroy(gr4hip_cfir_t* f) {
    delete f;
    return GR4HIP_OK;
}

// test hooks (exported, not declared in include/gr4hip.h)
int gr4hip_internal_cfir_last_paths(gr4hip_cfir_t* f, unsigned* mask) {
    GR4_REQUIRE(f && mask, "cfir_last_paths: bad arguments");
    *mask = f->last_paths;
    return GR4HIP_OK;
}
int gr4hip_internal_cfir_marked(gr4hip_cfir_t* f, gr4hip_stream_t stream, unsigned long long* n) {
    GR4_REQUIRE(f && n, "cfir_marked: bad arguments");
    *n = 0;
    if (!f->counted) return GR4HIP_OK;
    hipStream_t st = as_stream(stream);
    GR4_HIP_TRY(hipMemcpyAsync(&f->marked_host, f->d_count.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    GR4_HIP_TRY(hipStreamSynchronize(st));
    *n = f->marked_host;
    return GR4HIP_OK;
}

} // extern "C"
