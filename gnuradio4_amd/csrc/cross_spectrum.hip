// cross_spectrum.hip -- the cross-spectrum correlator (X-engine) on gfx950 (CROSS_SPECTRUM.md): C-ABI gr4hip_xcorr_*, its two leaf kernels (streaming VALU form,
// matrix-pipe form) and the coherence kernel.
//
//   S streams of frames X_s[f][c], c < N, complex<float>; baselines j <= i packed p = i (i + 1) / 2 + j; leaf l of integration q: frames q A + [64 l, min(64 (l + 1), A))
//   per leaf, per (i, j), per bin, float32, frames ascending, re = im = +0 at the leaf's start:
//       re = fmaf(xr_i, xr_j, re);   re = fmaf(xi_i, xi_j, re);
//       im = fmaf(xi_i, xr_j, im);   im = fmaf(-xr_i, xi_j, im);
//   acc_re, acc_im: float64, leaves ascending;  V_q[p][c] = (float)acc  or  (float)(acc / A);  the imaginary part of the diagonal is written as +0
//
// The reference has no such block: the definition is this project's, tests/cross_spectrum_oracle.py pins it.  One launch sums the call's leaves (each from +0, the
// call's first from the carried running leaf) into leaves[k][p][c] (interleaved complex), a second small one folds them into the float64 accumulator, writes the
// finished matrices and stores the carry of the next call into the other of two carry buffers -- the leaf integrator (leaf_integrator.hpp) with leaves of 64
// frames, rows of 2 P N floats and the Hermitian rule for the diagonal.
#include "leaf_integrator.hpp"

namespace gr4 {

constexpr int    kXcorrLeaf        = 64;
constexpr int    kXcorrMaxStreams  = 32;
constexpr size_t kXcorrMaxBins     = size_t(1) << 20;
constexpr size_t kXcorrMaxState    = size_t(1) << 24; // P n_bins: the carried state (two float64 and two float32 buffers of 2 P n_bins) stays below 0.8 GB
constexpr size_t kXcorrPieceValues = size_t(1) << 25; // input values (all streams) per piece: the leaf scratch is (S + 1) / 128 of that, 70 MB at S = 32
constexpr int    kXcorrValuMax     = 8;               // the VALU form exists for S <= 8 (72 accumulators)

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct XcorrIn {
    const float* s[kXcorrMaxStreams];
};

__device__ __forceinline__ f32x2 load_stream(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p)); } // read once: the FFT kernels' nt hint

// ---- form 1, streaming VALU: element i of [nl][N], one bin of one call-leaf.  The lane walks the leaf's frames, loads the S values of its bin (coalesced along
// bins) and issues the four fmaf of every pair in the defined order into 2 P float accumulators.
template <int S>
__global__ __launch_bounds__(256) void xcorr_valu_kernel(XcorrIn in, LeafGeom<kXcorrLeaf> g, const float* __restrict__ carry, float* __restrict__ leaves, int N, long total) {
    constexpr int P = S * (S + 1) / 2;
    const long    i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long k = i / N;
    const int  c = (int)(i - k * N);
    long       first;
    int        count;
    bool       complete;
    leaf_range(g, k, &first, &count, &complete);
    float re[P], im[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        re[p] = k == 0 ? carry[((long)p * N + c) * 2] : 0.f;
        im[p] = k == 0 ? carry[((long)p * N + c) * 2 + 1] : 0.f;
    }
    const long at = (first * N + c) * 2;
    for (int f = 0; f < count; ++f) {
        f32x2 x[S];
#pragma unroll
        for (int s = 0; s < S; ++s) x[s] = load_stream(in.s[s] + at + (long)f * N * 2);
#pragma unroll
        for (int a = 0; a < S; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                const int p = a * (a + 1) / 2 + b;
                re[p] = __builtin_fmaf(x[a].x, x[b].x, re[p]);
                re[p] = __builtin_fmaf(x[a].y, x[b].y, re[p]);
                im[p] = __builtin_fmaf(x[a].y, x[b].x, im[p]);
                im[p] = __builtin_fmaf(-x[a].x, x[b].y, im[p]);
            }
        }
    }
    float* o = leaves + ((k * P) * (long)N + c) * 2;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        f32x2 v;
        v.x = re[p];
        v.y = im[p];
        *reinterpret_cast<f32x2*>(o + (long)p * N * 2) = v;
    }
}

// ---- form 2, the f32 matrix pipe.  v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain (subnormals kept); with k = (frame, component) one instruction
// takes two frames, and with the operands
//     A row 2 i     = (xr_i,  xi_i)      "re" row of stream i          B column j = (xr_j, xi_j)
//     A row 2 i + 1 = (xi_i, -xr_i)      "im" row of stream i
// the accumulator chain IS the definition.  A workgroup (4 waves) takes one call-leaf and 16 bins: it stages [streams][8 frames][16 bins] into LDS (zero rows for
// the streams that pad to the tile, zero frames past the leaf's end), each wave owns 4 of the bins and keeps their accumulator tiles -- MT row tiles of 8 streams
// by NT column tiles of 16 streams, the strictly-upper tile skipped (S > 16: 6 of 8) -- so 4 to 24 independent accumulators hide the instruction's 40-cycle
// latency.  Lane l holds A[row l & 15][k = l >> 4], B[k = l >> 4][column l & 15] and D[row 4 (l >> 4) + r][column l & 15], r < 4: the complex sums of streams
// 2 (l >> 4), 2 (l >> 4) + 1 of its row tile against stream l & 15 of its column tile.
// A frame past the leaf's end enters as A = -0, B = +0: the products are -0, and x + (-0) = x for every x, +0 and -0 included -- an identity, bit for bit.
constexpr int kXmBins = 16, kXmFrames = 8, kXmBinsPerWave = 4;
constexpr int kXmFrameStride  = kXmBins * 2;                      // floats
constexpr int kXmStreamStride = kXmFrames * kXmFrameStride + 4;   // floats; + 4: the 8 streams of an A fragment fall into different banks

template <int MT, int NT>
__global__ __launch_bounds__(256) void xcorr_mfma_kernel(XcorrIn in, int S, LeafGeom<kXcorrLeaf> g, const float* __restrict__ carry, float* __restrict__ leaves, int N, int tiles) {
    constexpr int SP = 16 * NT; // staged streams: 8 MT <= 16 NT
    __shared__ float lds[SP * kXmStreamStride];
    const long k  = blockIdx.x / tiles;
    const int  c0 = (int)(blockIdx.x - k * tiles) * kXmBins;
    const int  P  = S * (S + 1) / 2;
    long       first;
    int        count;
    bool       complete;
    leaf_range(g, k, &first, &count, &complete);
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int col = l & 15, quad = l >> 4; // quad = k of the operands, row group of the result

    f32x4 acc[kXmBinsPerWave][MT][NT];
#pragma unroll
    for (int bb = 0; bb < kXmBinsPerWave; ++bb) {
        const int c = c0 + w * kXmBinsPerWave + bb;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
                if (k == 0 && c < N) { // the running leaf the call's first leaf continues
                    const int j = 16 * nt + col;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int i = 8 * mt + 2 * quad + h;
                        if (i < S && j <= i) {
                            const f32x2 v = *reinterpret_cast<const f32x2*>(carry + ((long)(i * (i + 1) / 2 + j) * N + c) * 2);
                            a[2 * h]      = v.x;
                            a[2 * h + 1]  = v.y;
                        }
                    }
                }
                acc[bb][mt][nt] = a;
            }
        }
    }

    // what this lane reads for its operands: stream, frame of the pair, component; the "im" row's second element is negated
    const int  a_stream = (col >> 1), a_im = col & 1, kf = quad >> 1, kc = quad & 1;
    const int  a_off = a_stream * kXmStreamStride + kf * kXmFrameStride + (kc ^ a_im);
    const bool a_neg = a_im && kc;
    const int  b_off = col * kXmStreamStride + kf * kXmFrameStride + kc;

    // Staging: 16 lanes per row of 16 bins; a wave takes rows 4 w .. 4 w + 3 of every group of 16, all four of one stream -- the stream is wave-uniform, its
    // pointer a scalar load from the kernel arguments.  The rows of step n + 1 are fetched into registers before step n is computed and go to LDS after it.
    constexpr int ROWS = SP * kXmFrames / 16;
    f32x2         next[ROWS];
    const auto    fetch = [&](int f0) {
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            const int r = (t >> 4) + 16 * u, b = t & 15, f = r & (kXmFrames - 1);
            const int s = __builtin_amdgcn_readfirstlane(r / kXmFrames);
            f32x2     v = {0.f, 0.f};
            if (s < S && f0 + f < count && c0 + b < N) v = load_stream(in.s[s] + ((first + f0 + f) * N + c0 + b) * 2);
            next[u] = v;
        }
    };
    fetch(0);
    for (int f0 = 0; f0 < count; f0 += kXmFrames) {
        __syncthreads(); // the tile of the step before has been read
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            const int r = (t >> 4) + 16 * u, b = t & 15, f = r & (kXmFrames - 1);
            *reinterpret_cast<f32x2*>(&lds[(r / kXmFrames) * kXmStreamStride + f * kXmFrameStride + b * 2]) = next[u];
        }
        __syncthreads();
        if (f0 + kXmFrames < count) fetch(f0 + kXmFrames);
        const int pairs = count - f0 < kXmFrames ? (count - f0 + 1) / 2 : kXmFrames / 2;
        for (int fp = 0; fp < pairs; ++fp) {
            const bool past = f0 + 2 * fp + kf >= count; // the second frame of a ragged leaf's last pair
#pragma unroll
            for (int bb = 0; bb < kXmBinsPerWave; ++bb) {
                const int at = 2 * fp * kXmFrameStride + (w * kXmBinsPerWave + bb) * 2;
                float     a[MT], b[NT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const float v = lds[a_off + at + mt * 8 * kXmStreamStride];
                    a[mt]         = past ? -0.f : (a_neg ? -v : v);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) b[nt] = lds[b_off + at + nt * 16 * kXmStreamStride];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        if (8 * mt + 7 < 16 * nt) continue; // every i of the row tile below every j of the column tile: strictly upper
                        acc[bb][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[bb][mt][nt], 0, 0, 0);
                    }
                }
            }
        }
    }

    // the wave's 4 bins are neighbours: a lane's sums of one pair are 32 contiguous bytes of the baseline's row (16-byte stores where the rows are aligned to 16)
    const int  cw   = c0 + w * kXmBinsPerWave;
    const bool wide = (N & 1) == 0 && cw + kXmBinsPerWave <= N;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (8 * mt + 7 < 16 * nt) continue;
            const int j = 16 * nt + col;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = 8 * mt + 2 * quad + h;
                if (i >= S || j > i) continue;
                float* row = leaves + ((k * P + (i * (i + 1) / 2 + j)) * (long)N + cw) * 2;
                if (wide) {
#pragma unroll
                    for (int bb = 0; bb < kXmBinsPerWave; bb += 2) {
                        f32x4 v;
                        v.x = acc[bb][mt][nt][2 * h];
                        v.y = acc[bb][mt][nt][2 * h + 1];
                        v.z = acc[bb + 1][mt][nt][2 * h];
                        v.w = acc[bb + 1][mt][nt][2 * h + 1];
                        *reinterpret_cast<f32x4*>(row + bb * 2) = v;
                    }
                } else {
#pragma unroll
                    for (int bb = 0; bb < kXmBinsPerWave; ++bb) {
                        if (cw + bb >= N) continue;
                        f32x2 v;
                        v.x = acc[bb][mt][nt][2 * h];
                        v.y = acc[bb][mt][nt][2 * h + 1];
                        *reinterpret_cast<f32x2*>(row + bb * 2) = v;
                    }
                }
            }
        }
    }
}

// ---- coherence and H1 of one pair from emitted matrices: element idx of [n_spectra][N].  pij: the packed baseline (max, min); conj: i < j, V_ij = conj(V_ji)
__global__ __launch_bounds__(256) void xcorr_coherence_kernel(const float* __restrict__ vis, int N, long P, long pij, int conj, long pii, long pjj, float* __restrict__ msc,
                                                              float* __restrict__ h1, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long   q = idx / N, c = idx - q * N;
    const float* m = vis + q * P * N * 2;
    const double re = (double)m[(pij * N + c) * 2], im = (double)(conj ? -m[(pij * N + c) * 2 + 1] : m[(pij * N + c) * 2 + 1]);
    const double vii = (double)m[(pii * N + c) * 2], vjj = (double)m[(pjj * N + c) * 2];
    if (msc) msc[idx] = (float)((re * re + im * im) / (vii * vjj));
    if (h1) {
        f32x2 v;
        v.x = (float)(re / vjj);
        v.y = (float)(im / vjj);
        *reinterpret_cast<f32x2*>(h1 + idx * 2) = v;
    }
}

} // namespace gr4

using namespace gr4;

struct gr4hip_xcorr {
    size_t                            S = 0, N = 0, P = 0;
    LeafIntegrator<kXcorrLeaf, true>  integ; // M = 2 P N
    int                               last_path  = 0;
    int                               force_path = 0; // test hook: 1 = the VALU form where it exists (S <= 8), 2 = the matrix-pipe form, 0 = the default
};

namespace gr4 {

// The default form: not measured on an MI355X yet (CROSS_SPECTRUM.md) -- the VALU form wherever it exists, the matrix pipe above.
static int xcorr_path(const gr4hip_xcorr* x) {
    if (x->S > (size_t)kXcorrValuMax || x->force_path == 2) return 2;
    return 1;
}

template <int S>
static void xcorr_valu_launch(const XcorrIn& in, const LeafGeom<kXcorrLeaf>& g, const float* carry, float* leaves, int N, hipStream_t st) {
    const long total = g.nl * (long)N;
    hipLaunchKernelGGL(xcorr_valu_kernel<S>, dim3((unsigned)ceil_div(total, 256L)), dim3(256), 0, st, in, g, carry, leaves, N, total);
}

static int xcorr_leaves(int path, int S, const XcorrIn& in, const LeafGeom<kXcorrLeaf>& g, const float* carry, float* leaves, int N, hipStream_t st) {
    if (path == 1) {
        switch (S) {
        case 2: xcorr_valu_launch<2>(in, g, carry, leaves, N, st); break;
        case 3: xcorr_valu_launch<3>(in, g, carry, leaves, N, st); break;
        case 4: xcorr_valu_launch<4>(in, g, carry, leaves, N, st); break;
        case 5: xcorr_valu_launch<5>(in, g, carry, leaves, N, st); break;
        case 6: xcorr_valu_launch<6>(in, g, carry, leaves, N, st); break;
        case 7: xcorr_valu_launch<7>(in, g, carry, leaves, N, st); break;
        case 8: xcorr_valu_launch<8>(in, g, carry, leaves, N, st); break;
        default: set_error("xcorr: internal: no VALU kernel for %d streams", S); return GR4HIP_RUNTIME_ERROR;
        }
    } else {
        const int  tiles  = (N + kXmBins - 1) / kXmBins;
        const long blocks = g.nl * (long)tiles;
        GR4_REQUIRE(blocks <= 0x7fffffffL, "xcorr: %ld leaves of %d bin tiles in one piece", g.nl, tiles);
        const dim3 grid((unsigned)blocks);
        if (S <= 8) hipLaunchKernelGGL((xcorr_mfma_kernel<1, 1>), grid, dim3(256), 0, st, in, S, g, carry, leaves, N, tiles);
        else if (S <= 16) hipLaunchKernelGGL((xcorr_mfma_kernel<2, 1>), grid, dim3(256), 0, st, in, S, g, carry, leaves, N, tiles);
        else if (S <= 24) hipLaunchKernelGGL((xcorr_mfma_kernel<3, 2>), grid, dim3(256), 0, st, in, S, g, carry, leaves, N, tiles);
        else hipLaunchKernelGGL((xcorr_mfma_kernel<4, 2>), grid, dim3(256), 0, st, in, S, g, carry, leaves, N, tiles);
    }
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

// one piece: n frames of every stream, already offset
static int xcorr_fold(gr4hip_xcorr* x, const XcorrIn& in, size_t n_frames, float* d_out, hipStream_t st) {
    LeafGeom<kXcorrLeaf> g;
    const float*         carry;
    float*               leaves;
    if (const int rc = x->integ.begin(n_frames, st, "xcorr", &g, &carry, &leaves)) return rc;
    const int path = xcorr_path(x);
    if (const int rc = xcorr_leaves(path, (int)x->S, in, g, carry, leaves, (int)x->N, st)) return rc;
    if (const int rc = x->integ.finish(g, d_out, st)) return rc;
    x->last_path = path;
    return GR4HIP_OK;
}

} // namespace gr4

extern "C" {

size_t gr4hip_xcorr_leaf(void) { return (size_t)kXcorrLeaf; }

int gr4hip_xcorr_create(gr4hip_xcorr_t** out, size_t n_streams, size_t n_bins, size_t n_integrate, int flags) {
    GR4_REQUIRE(out, "xcorr: null output handle");
    GR4_REQUIRE(n_streams >= 2, "xcorr: n_streams must be >= 2 (got %zu)", n_streams);
    GR4_REQUIRE(n_bins >= 2, "xcorr: n_bins must be >= 2 (got %zu)", n_bins);
    GR4_REQUIRE(n_integrate >= 1 && n_integrate <= kLeafMaxFrames, "xcorr: n_integrate must be in [1, 2^40] (got %zu)", n_integrate);
    GR4_REQUIRE((flags & ~GR4HIP_XCORR_MEAN) == 0, "xcorr: unknown flags %d", flags);
    if (n_streams > (size_t)kXcorrMaxStreams) { set_error("xcorr: %zu streams (supported: up to %d)", n_streams, kXcorrMaxStreams); return GR4HIP_UNSUPPORTED; }
    if (n_bins > kXcorrMaxBins) { set_error("xcorr: %zu bins (supported: up to %zu)", n_bins, kXcorrMaxBins); return GR4HIP_UNSUPPORTED; }
    const size_t P = n_streams * (n_streams + 1) / 2;
    if (P * n_bins > kXcorrMaxState) { set_error("xcorr: %zu baselines of %zu bins (supported: up to %zu values of carried state)", P, n_bins, kXcorrMaxState); return GR4HIP_UNSUPPORTED; }
    auto* x = new (std::nothrow) gr4hip_xcorr();
    GR4_REQUIRE(x, "out of host memory");
    x->S          = n_streams;
    x->N          = n_bins;
    x->P          = P;
    x->integ.M    = 2 * P * n_bins;
    x->integ.N    = n_bins;
    x->integ.A    = n_integrate;
    x->integ.mean = (flags & GR4HIP_XCORR_MEAN) != 0;
    *out          = x; // the device buffers come with the first process call: everything up to there is host code
    return GR4HIP_OK;
}

int gr4hip_xcorr_reset(gr4hip_xcorr_t* x) {
    GR4_REQUIRE(x, "xcorr_reset: null handle");
    x->integ.reset();
    return GR4HIP_OK;
}

int gr4hip_xcorr_set_length(gr4hip_xcorr_t* x, size_t n_integrate) {
    GR4_REQUIRE(x, "xcorr_set_length: null handle");
    GR4_REQUIRE(n_integrate >= 1 && n_integrate <= kLeafMaxFrames, "xcorr_set_length: n_integrate must be in [1, 2^40] (got %zu)", n_integrate);
    x->integ.set_length(n_integrate);
    return GR4HIP_OK;
}

int gr4hip_xcorr_pending(const gr4hip_xcorr_t* x, size_t n_frames, size_t* n_out) {
    GR4_REQUIRE(x && n_out, "xcorr_pending: null argument");
    GR4_REQUIRE(n_frames <= kLeafMaxFrames, "xcorr_pending: %zu frames", n_frames);
    *n_out = x->integ.pending(n_frames);
    return GR4HIP_OK;
}

int gr4hip_xcorr_process(gr4hip_xcorr_t* x, const float* const* d_spectra, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(x, "xcorr_process: null handle");
    GR4_REQUIRE(n_out, "xcorr_process: null n_out");
    if (n_frames == 0) { *n_out = 0; return GR4HIP_OK; }
    GR4_REQUIRE(d_spectra, "xcorr_process: null array of inputs");
    GR4_REQUIRE(n_frames <= kLeafMaxFrames / x->N, "xcorr_process: %zu frames of %zu bins in one call", n_frames, x->N);
    const size_t n = x->integ.pending(n_frames);
    GR4_REQUIRE(d_out || n == 0, "xcorr_process: null output in a call that completes %zu integrations", n);
    GR4_REQUIRE((uintptr_t)d_out % 8 == 0, "xcorr_process: the output must be aligned to 8 bytes");
    XcorrIn         in{};
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + n * x->integ.M * sizeof(float);
    for (size_t s = 0; s < x->S; ++s) {
        GR4_REQUIRE(d_spectra[s], "xcorr_process: null input %zu", s);
        GR4_REQUIRE((uintptr_t)d_spectra[s] % 8 == 0, "xcorr_process: input %zu must be aligned to 8 bytes", s);
        const uintptr_t a0 = (uintptr_t)d_spectra[s], a1 = a0 + n_frames * x->N * 2 * sizeof(float);
        GR4_REQUIRE(n == 0 || a1 <= o0 || o1 <= a0, "xcorr_process: d_out overlaps input %zu", s);
        in.s[s] = d_spectra[s];
    }
    const hipStream_t st    = as_stream(stream);
    const size_t      piece = std::max<size_t>(1, kXcorrPieceValues / (x->N * x->S));
    const int         rc    = x->integ.for_each_piece(n_frames, piece, d_out, [&](size_t f, size_t m, float* out) {
        XcorrIn at{};
        for (size_t s = 0; s < x->S; ++s) at.s[s] = in.s[s] + f * x->N * 2;
        return xcorr_fold(x, at, m, out, st);
    });
    if (rc) return rc;
    *n_out = n;
    return GR4HIP_OK;
}

int gr4hip_xcorr_destroy(gr4hip_xcorr_t* x) {
    delete x;
    return GR4HIP_OK;
}

int gr4hip_xcorr_coherence(const float* d_vis, size_t n_streams, size_t n_bins, size_t n_spectra, size_t i, size_t j, float* d_msc, float* d_h1, gr4hip_stream_t stream) {
    GR4_REQUIRE(d_vis, "xcorr_coherence: null input");
    GR4_REQUIRE(d_msc || d_h1, "xcorr_coherence: both outputs are null");
    GR4_REQUIRE(n_streams >= 2 && n_bins >= 2, "xcorr_coherence: n_streams and n_bins must be >= 2 (got %zu, %zu)", n_streams, n_bins);
    GR4_REQUIRE(i < n_streams && j < n_streams, "xcorr_coherence: pair (%zu, %zu) of %zu streams", i, j, n_streams);
    GR4_REQUIRE((uintptr_t)d_vis % 8 == 0 && (uintptr_t)d_h1 % 8 == 0 && (uintptr_t)d_msc % 4 == 0, "xcorr_coherence: d_vis and d_h1 must be aligned to 8 bytes, d_msc to 4");
    if (n_streams > (size_t)kXcorrMaxStreams || n_bins > kXcorrMaxBins) { set_error("xcorr_coherence: %zu streams of %zu bins", n_streams, n_bins); return GR4HIP_UNSUPPORTED; }
    const size_t P = n_streams * (n_streams + 1) / 2;
    GR4_REQUIRE(n_spectra <= (size_t(1) << 40) / (P * n_bins), "xcorr_coherence: %zu matrices in one call", n_spectra);
    const uintptr_t v0 = (uintptr_t)d_vis, v1 = v0 + n_spectra * P * n_bins * 8;
    const uintptr_t m0 = (uintptr_t)d_msc, m1 = m0 + n_spectra * n_bins * 4, h0 = (uintptr_t)d_h1, h1 = h0 + n_spectra * n_bins * 8;
    GR4_REQUIRE(!d_msc || v1 <= m0 || m1 <= v0, "xcorr_coherence: d_msc overlaps the input");
    GR4_REQUIRE(!d_h1 || v1 <= h0 || h1 <= v0, "xcorr_coherence: d_h1 overlaps the input");
    if (n_spectra == 0) return GR4HIP_OK;
    const size_t hi = std::max(i, j), lo = std::min(i, j);
    const long   total = (long)(n_spectra * n_bins);
    hipLaunchKernelGGL(xcorr_coherence_kernel, dim3((unsigned)ceil_div(total, 256L)), dim3(256), 0, as_stream(stream), d_vis, (int)n_bins, (long)P, (long)(hi * (hi + 1) / 2 + lo),
                       i < j ? 1 : 0, (long)(i * (i + 3) / 2), (long)(j * (j + 3) / 2), d_msc, d_h1, total);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

// test hook (exported, not declared in include/gr4hip.h): which leaf kernel the last call ran -- 1 = the VALU form, 2 = the matrix-pipe form (0: no call yet)
int gr4hip_internal_xcorr_last_path(gr4hip_xcorr_t* x, int* path) {
    GR4_REQUIRE(x && path, "xcorr_last_path: bad arguments");
    *path = x->last_path;
    return GR4HIP_OK;
}

// test hook: 1 = the VALU form where it exists (S <= 8; above that the matrix-pipe form runs and last_path says so), 2 = the matrix-pipe form, 0 = the default
int gr4hip_internal_xcorr_set_path(gr4hip_xcorr_t* x, int path) {
    GR4_REQUIRE(x && path >= 0 && path <= 2, "xcorr_set_path: bad arguments");
    x->force_path = path;
    return GR4HIP_OK;
}

} // extern "C"
