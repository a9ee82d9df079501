// beamformer.hip -- the beamformer (B-engine) on gfx950 (BEAMFORMER.md): C-ABI gr4hip_beamform_*, its two kernels (streaming VALU form, matrix-pipe form), each
// with a voltage entry and an entry that detects and integrates the power through a spectrum integrator handle, and the kernel that arranges the weights into
// the matrix pipe's fragment order.
//
//   S streams of frames X_s[f][c], c < N, complex<float>; B beams; weights W[b][s][c], complex<float>, bin fastest
//   per beam, frame and bin, float32, streams ascending, re = im = +0 at the start:
//       re = fmaf( wr_s, xr_s, re);   re = fmaf(-wi_s, xi_s, re);
//       im = fmaf( wi_s, xr_s, im);   im = fmaf( wr_s, xi_s, im);
//   Y_b[f][c] = (re, im);   p_b[f][c] = fmaf(yr, yr, yi * yi);   integrated: the spectrum integrator's definition on frames [b][c] of B N floats
//
// The reference has no such block: the definition is this project's, tests/beamformer_oracle.py pins it.  The integrating entry writes the float32 sums of the
// integrator's call-leaves (specint_kernels.hpp) into that handle's scratch; its emit kernel folds them, as behind gr4hip_fft_mag2_integrate.
#ifndef GR4_BUF_STORE_AUX
#define GR4_BUF_STORE_AUX 2
#endif
#include "specint_kernels.hpp"

#include <algorithm>

namespace gr4 {

constexpr int    kBfMax         = 32;               // streams, beams
constexpr size_t kBfMaxBins     = size_t(1) << 20;
constexpr size_t kBfMaxWeights  = size_t(1) << 24;  // B S n_bins: the raw weights stay below 128 MiB
constexpr size_t kBfPieceValues = size_t(1) << 25;  // max(S, B) n_bins frames per piece of the integrating entry: the leaf scratch is at most 1 / 32 of that, 4 MiB
constexpr int    kBfValuMaxS = 8, kBfValuMaxB = 8;  // the VALU form exists for S <= 8 with B <= 8 (up to 128 weight registers)
constexpr int    kBfChunk = 64;                     // frames of a voltage call one lane (VALU) or one workgroup (matrix pipe) walks

typedef float bf_f2 __attribute__((ext_vector_type(2)));
typedef float bf_f4 __attribute__((ext_vector_type(4)));

struct BfIn {
    const float* s[kBfMax];
};
struct BfOut {
    float* b[kBfMax];
};

__device__ __forceinline__ bf_f2 bf_load(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const bf_f2*>(p)); } // read once: the FFT kernels' nt hint

// unit k of a launch: the frames [first, first + count) of the call -- a call-leaf of the integrator (POWER) or a chunk of 64 frames
template <bool POWER>
__device__ __forceinline__ void bf_unit(const SpecintGeom& g, long n_frames, long k, long* first, int* count) {
    if constexpr (POWER) {
        bool complete;
        leaf_range(g, k, first, count, &complete);
    } else {
        *first = k * kBfChunk;
        *count = (int)(n_frames - *first < kBfChunk ? n_frames - *first : kBfChunk);
    }
}

// ---- form 1, streaming VALU: element i of [units][N], one bin of one unit.  The lane keeps its bin's 2 S B weight components in registers, walks the unit's
// frames, loads the S values of its bin (coalesced along bins) and issues the 4 S fmaf of every beam in the defined order.  POWER: p_b joins B float leaf sums.
template <int S, int B, bool POWER>
__global__ __launch_bounds__(256) void beamform_valu_kernel(BfIn in, const float* __restrict__ w, int N, long n_frames, BfOut out, long stride, SpecintGeom g,
                                                            const float* __restrict__ carry, float* __restrict__ leaves, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long k = i / N;
    const int  c = (int)(i - k * N);
    long       first;
    int        count;
    bf_unit<POWER>(g, n_frames, k, &first, &count);
    float wr[B][S], wi[B][S];
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const bf_f2 v = *reinterpret_cast<const bf_f2*>(w + ((long)(b * S + s) * N + c) * 2);
            wr[b][s]      = v.x;
            wi[b][s]      = v.y;
        }
    }
    float acc[B];
#pragma unroll
    for (int b = 0; b < B; ++b) acc[b] = (POWER && k == 0) ? carry[(long)b * N + c] : 0.f;
    const long at = (first * N + c) * 2;
    for (int f = 0; f < count; ++f) {
        bf_f2 x[S];
#pragma unroll
        for (int s = 0; s < S; ++s) x[s] = bf_load(in.s[s] + at + (long)f * N * 2);
#pragma unroll
        for (int b = 0; b < B; ++b) {
            float re = 0.f, im = 0.f;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                re = __builtin_fmaf(wr[b][s], x[s].x, re);
                re = __builtin_fmaf(-wi[b][s], x[s].y, re);
                im = __builtin_fmaf(wi[b][s], x[s].x, im);
                im = __builtin_fmaf(wr[b][s], x[s].y, im);
            }
            if constexpr (POWER) {
                acc[b] = acc[b] + __builtin_fmaf(re, re, im * im);
            } else {
                bf_f2 v;
                v.x = re;
                v.y = im;
                *reinterpret_cast<bf_f2*>(out.b[b] + ((first + f) * stride + c) * 2) = v;
            }
        }
    }
    if constexpr (POWER) {
#pragma unroll
        for (int b = 0; b < B; ++b) leaves[(k * B + b) * (long)N + c] = acc[b];
    }
}

// ---- form 2, the f32 matrix pipe.  v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain (subnormals kept); with k = (stream, component) one instruction
// takes two streams, and with the operands
//     A row 2 b     = ( wr_s, -wi_s)     "re" row of beam b          B column f = (xr_s, xi_s) of frame f
//     A row 2 b + 1 = ( wi_s,  wr_s)     "im" row of beam b
// and the k-steps of one accumulator issued in ascending order the accumulator chain IS the definition.  Columns are the frames of one bin (the weights differ
// per bin).  A workgroup (4 waves) takes one unit and 16 bins: per step it stages [streams][16 bins][16 frames] into LDS (coalesced along bins; +0 for the streams
// that pad to a k-step and for frames past the unit's end), each wave owns 4 of the bins and runs their KS = ceil(S / 2) k-steps against MT = ceil(B / 8) row
// tiles -- 4 MT independent accumulators -- with the A fragments read from the fragment-ordered copy of the weights (beamform_arrange_kernel: one coalesced
// 256-byte load per instruction, L2 traffic), then the results go back through the same LDS so that a row of 16 bins is stored with one 128-byte access.
// Lane l holds A[row l & 15][k = l >> 4], B[k = l >> 4][column l & 15] and D[row 4 (l >> 4) + r][column l & 15], r < 4: (re, im) of beams 2 (l >> 4), 2 (l >> 4) + 1
// of its row tile at frame l & 15.
// The padding k-slot of an odd S enters as A = -0, B = +0: the product is -0, and x + (-0) = x for every x, +0 and -0 included -- an identity, bit for bit.
// Frames past the unit's end are computed from zeros and neither stored nor summed.
// LDS, input:  float (s, bin, f, comp) at s 512 + (bin ^ (s & 1)) 32 + ((f + bin) & 15) 2 + comp -- the staging stores (16 lanes along bins) and the operand loads
//              (16 lanes along frames, two streams) both touch every bank once;
//      output: voltage (beam, f, bin) at beam 512 + f 32 + ((bin + f) & 15) 2, power (beam, bin, f) at beam 272 + bin 16 + ((f + bin) & 15).
constexpr int kBmBins = 16, kBmFrames = 16, kBmBinsPerWave = 4, kBmRow = 512, kBmPowerRow = 272;

// wfrag[c][ks][mt][lane]: what lane holds of the A fragment of bin c, k-step ks, row tile mt.  Padding (beam >= B or stream >= S): -0.
__global__ __launch_bounds__(256) void beamform_arrange_kernel(const float* __restrict__ w, float* __restrict__ wfrag, int S, int B, int N, int MT, int KS, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int  l = (int)(i & 63);
    long       r = i >> 6;
    const int  mt = (int)(r % MT);
    r /= MT;
    const int  ks = (int)(r % KS);
    const long c  = r / KS;
    const int  row = l & 15, kk = l >> 4;
    const int  b = 8 * mt + (row >> 1), im = row & 1, s = 2 * ks + (kk >> 1), comp = kk & 1;
    float      v = -0.f;
    if (b < B && s < S) {
        const float wr = w[((long)(b * S + s) * N + c) * 2], wi = w[((long)(b * S + s) * N + c) * 2 + 1];
        v              = im ? (comp ? wr : wi) : (comp ? -wi : wr);
    }
    wfrag[i] = v;
}

template <int MT, int SW, bool POWER> // MT = ceil(B / 8) row tiles, SW = ceil(S / 8): the streams are staged in groups of 8, only the last group tests s < S
__global__ __launch_bounds__(256) void beamform_mfma_kernel(BfIn in, int S, int B, const float* __restrict__ wfrag, int N, long n_frames, BfOut out, long stride,
                                                            SpecintGeom g, const float* __restrict__ carry, float* __restrict__ leaves, int tiles) {
    constexpr int ROWS = 8 * (MT > SW ? MT : SW), SROWS = 8 * SW; // rows of 512 floats: the larger of the staged streams and the beams of the row tiles
    __shared__ float lds[ROWS * kBmRow];
    const long k  = blockIdx.x / tiles;
    const int  c0 = (int)(blockIdx.x - k * tiles) * kBmBins;
    long       first;
    int        count;
    bf_unit<POWER>(g, n_frames, k, &first, &count);
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int col = l & 15, quad = l >> 4;
    const int KS = (S + 1) / 2;
    const int sf = t >> 4, sb = t & 15; // staging and storing: 16 lanes per row of 16 bins, 16 rows (frames) per pass

    // POWER: the leaf sums of this lane's (beam, bin) pairs, in frame order
    constexpr int PU = (ROWS * kBmBins + 255) / 256;
    float         pacc[PU];
#pragma unroll
    for (int u = 0; u < PU; ++u) {
        const int idx = t + 256 * u, beam = idx >> 4, c = c0 + (idx & 15);
        pacc[u]       = (POWER && k == 0 && beam < B && c < N) ? carry[(long)beam * N + c] : 0.f;
    }

    // the weights of the wave's bins; a bin past N reads those of bin N - 1 and is never stored
    const float* wf[kBmBinsPerWave];
#pragma unroll
    for (int bb = 0; bb < kBmBinsPerWave; ++bb) {
        const int c = c0 + w * kBmBinsPerWave + bb;
        wf[bb]      = wfrag + (long)(c < N ? c : N - 1) * KS * MT * 64 + l;
    }

    // The stream of a staging row is uniform: its pointer is a scalar load from the kernel arguments at the row's turn (an index the compiler can see through makes
    // it keep all 32 pointers in scalar registers and spill them), and the test s < S a scalar branch.  A lane outside the unit or past N reads the stream's first
    // value instead -- always there -- and drops it: one address for all streams, no lane mask per stream.
    int opaque0 = 0;
    asm volatile("" : "+s"(opaque0));
    bf_f2      next[SROWS];
    const auto fetch = [&](int f0) {
        const bool ok  = f0 + sf < count && c0 + sb < N;
        const long off = ok ? ((first + f0 + sf) * N + c0 + sb) * 2 : 0;
#pragma unroll
        for (int s = 0; s < SROWS; ++s) {
            bf_f2 v = {0.f, 0.f};
            if (s < SROWS - 8 || s < S) {
                const bf_f2 x = bf_load(in.s[s + opaque0] + off);
                v.x           = ok ? x.x : 0.f;
                v.y           = ok ? x.y : 0.f;
            }
            next[s] = v;
        }
    };
    fetch(0);
    for (int f0 = 0; f0 < count; f0 += kBmFrames) {
        __syncthreads(); // the results of the step before have been read
#pragma unroll
        for (int s = 0; s < SROWS; ++s) *reinterpret_cast<bf_f2*>(&lds[s * kBmRow + ((sb ^ (s & 1)) * 32) + ((sf + sb) & 15) * 2]) = next[s];
        __syncthreads();
        if (f0 + kBmFrames < count) fetch(f0 + kBmFrames);

        bf_f4 acc[kBmBinsPerWave][MT];
#pragma unroll
        for (int bb = 0; bb < kBmBinsPerWave; ++bb) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[bb][mt] = bf_f4{0.f, 0.f, 0.f, 0.f};
        }
        for (int ks = 0; ks < KS; ++ks) {
            const int s = 2 * ks + (quad >> 1), comp = quad & 1;
#pragma unroll
            for (int bb = 0; bb < kBmBinsPerWave; ++bb) {
                const int   bl = w * kBmBinsPerWave + bb;
                const float b  = lds[s * kBmRow + ((bl ^ (s & 1)) * 32) + ((col + bl) & 15) * 2 + comp];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const float a = wf[bb][(long)(ks * MT + mt) * 64];
                    acc[bb][mt]   = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[bb][mt], 0, 0, 0);
                }
            }
        }
        __syncthreads(); // every wave has read its operands: the tile becomes the results'

        const int left = count - f0 < kBmFrames ? count - f0 : kBmFrames;
        if constexpr (POWER) {
#pragma unroll
            for (int bb = 0; bb < kBmBinsPerWave; ++bb) {
                const int bl = w * kBmBinsPerWave + bb;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float re = acc[bb][mt][2 * h], im = acc[bb][mt][2 * h + 1];
                        lds[(8 * mt + 2 * quad + h) * kBmPowerRow + bl * 16 + ((col + bl) & 15)] = __builtin_fmaf(re, re, im * im);
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                const int idx = t + 256 * u, beam = idx >> 4, bin = idx & 15;
                if (beam < B && beam < 8 * MT) {
                    for (int f = 0; f < left; ++f) pacc[u] = pacc[u] + lds[beam * kBmPowerRow + bin * 16 + ((f + bin) & 15)];
                }
            }
        } else {
#pragma unroll
            for (int bb = 0; bb < kBmBinsPerWave; ++bb) {
                const int bl = w * kBmBinsPerWave + bb;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        bf_f2 v;
                        v.x = acc[bb][mt][2 * h];
                        v.y = acc[bb][mt][2 * h + 1];
                        *reinterpret_cast<bf_f2*>(&lds[(8 * mt + 2 * quad + h) * kBmRow + col * 32 + ((bl + col) & 15) * 2]) = v;
                    }
                }
            }
            __syncthreads();
            if (sf < left && c0 + sb < N) {
                for (int b = 0; b < B; ++b) { // (uniform: the beam's pointer is a scalar load)
                    const bf_f2 v = *reinterpret_cast<const bf_f2*>(&lds[b * kBmRow + sf * 32 + ((sb + sf) & 15) * 2]);
                    *reinterpret_cast<bf_f2*>(out.b[b] + ((first + f0 + sf) * stride + c0 + sb) * 2) = v;
                }
            }
        }
    }
    if constexpr (POWER) {
#pragma unroll
        for (int u = 0; u < PU; ++u) {
            const int idx = t + 256 * u, beam = idx >> 4, c = c0 + (idx & 15);
            if (beam < B && beam < 8 * MT && c < N) leaves[(k * B + beam) * (long)N + c] = pacc[u];
        }
    }
}

} // namespace gr4

using namespace gr4;

struct gr4hip_beamform {
    size_t       S = 0, B = 0, N = 0;
    DeviceBuffer d_w, d_frag;       // the weights as given, [B][S][N] complex, and in the matrix pipe's fragment order (made on the first use of that form)
    bool         have_w = false, frag_current = false;
    int          last_path = 0;
    int          force_path = 0; // test hook: 1 = the VALU form where it exists (S <= 8, B <= 8), 2 = the matrix-pipe form, 0 = the default
};

namespace gr4 {

static bool bf_has_valu(const gr4hip_beamform* bf) { return bf->S <= (size_t)kBfValuMaxS && bf->B <= (size_t)kBfValuMaxB; }

// The default form (BEAMFORMER.md, profiles/beamformer_rates.txt, profiles/beamformer_rates_shapes.txt): a form is a shape's default only where its median beat the
// other's by more than both spreads combined.  Measured at N = 1024, 2^27 samples per call, at twelve shapes with S <= 8 and B <= 8: the VALU form wins both
// entries everywhere (the matrix pipe reaches 0.19 .. 0.60 of it on the integrating entry, 0.45 .. 0.95 on the voltage entry), so it is the default wherever it
// exists; above 8 streams or beams the matrix pipe is the only form.
static int bf_path(const gr4hip_beamform* bf) {
    if (!bf_has_valu(bf) || bf->force_path == 2) return 2;
    return 1;
}

struct BfLaunch {
    BfIn         in;
    BfOut        out;
    long         n_frames, stride;
    SpecintGeom  geom;
    const float* carry;
    float*       leaves;
};

template <int S, int B, bool POWER>
static void bf_valu_launch(const gr4hip_beamform* bf, const BfLaunch& L, long units, hipStream_t st) {
    const long total = units * (long)bf->N;
    hipLaunchKernelGGL((beamform_valu_kernel<S, B, POWER>), dim3((unsigned)ceil_div(total, 256L)), dim3(256), 0, st, L.in, static_cast<const float*>(bf->d_w.ptr), (int)bf->N,
                       L.n_frames, L.out, L.stride, L.geom, L.carry, L.leaves, total);
}

template <int S, bool POWER>
static int bf_valu_beams(const gr4hip_beamform* bf, const BfLaunch& L, long units, hipStream_t st) {
    switch (bf->B) {
    case 1: bf_valu_launch<S, 1, POWER>(bf, L, units, st); return GR4HIP_OK;
    case 2: bf_valu_launch<S, 2, POWER>(bf, L, units, st); return GR4HIP_OK;
    case 3: bf_valu_launch<S, 3, POWER>(bf, L, units, st); return GR4HIP_OK;
    case 4: bf_valu_launch<S, 4, POWER>(bf, L, units, st); return GR4HIP_OK;
    case 5: bf_valu_launch<S, 5, POWER>(bf, L, units, st); return GR4HIP_OK;
    case 6: bf_valu_launch<S, 6, POWER>(bf, L, units, st); return GR4HIP_OK;
    case 7: bf_valu_launch<S, 7, POWER>(bf, L, units, st); return GR4HIP_OK;
    case 8: bf_valu_launch<S, 8, POWER>(bf, L, units, st); return GR4HIP_OK;
    default: set_error("beamform: internal: no VALU kernel for %zu beams", bf->B); return GR4HIP_RUNTIME_ERROR;
    }
}

template <bool POWER>
static int bf_valu(const gr4hip_beamform* bf, const BfLaunch& L, long units, hipStream_t st) {
    switch (bf->S) {
    case 1: return bf_valu_beams<1, POWER>(bf, L, units, st);
    case 2: return bf_valu_beams<2, POWER>(bf, L, units, st);
    case 3: return bf_valu_beams<3, POWER>(bf, L, units, st);
    case 4: return bf_valu_beams<4, POWER>(bf, L, units, st);
    case 5: return bf_valu_beams<5, POWER>(bf, L, units, st);
    case 6: return bf_valu_beams<6, POWER>(bf, L, units, st);
    case 7: return bf_valu_beams<7, POWER>(bf, L, units, st);
    case 8: return bf_valu_beams<8, POWER>(bf, L, units, st);
    default: set_error("beamform: internal: no VALU kernel for %zu streams", bf->S); return GR4HIP_RUNTIME_ERROR;
    }
}

template <int MT, int SW, bool POWER>
static void bf_mfma_launch(const gr4hip_beamform* bf, const BfLaunch& L, long units, int tiles, hipStream_t st) {
    hipLaunchKernelGGL((beamform_mfma_kernel<MT, SW, POWER>), dim3((unsigned)(units * tiles)), dim3(256), 0, st, L.in, (int)bf->S, (int)bf->B,
                       static_cast<const float*>(bf->d_frag.ptr), (int)bf->N, L.n_frames, L.out, L.stride, L.geom, L.carry, L.leaves, tiles);
}

template <bool POWER>
static int bf_mfma(gr4hip_beamform* bf, const BfLaunch& L, long units, hipStream_t st) {
    const int MT = (int)(bf->B + 7) / 8, KS = (int)(bf->S + 1) / 2, SW = (int)(bf->S + 7) / 8;
    if (!bf->frag_current) { // once per set_weights, not per launch
        const long total = (long)bf->N * KS * MT * 64;
        if (const int rc = bf->d_frag.ensure((size_t)total * sizeof(float))) return rc;
        hipLaunchKernelGGL(beamform_arrange_kernel, dim3((unsigned)ceil_div(total, 256L)), dim3(256), 0, st, static_cast<const float*>(bf->d_w.ptr), static_cast<float*>(bf->d_frag.ptr),
                           (int)bf->S, (int)bf->B, (int)bf->N, MT, KS, total);
        GR4_LAUNCH_CHECK();
        bf->frag_current = true;
    }
    const int  tiles  = (int)((bf->N + kBmBins - 1) / kBmBins);
    const long blocks = units * (long)tiles;
    GR4_REQUIRE(blocks <= 0x7fffffffL, "beamform: %ld units of %d bin tiles in one launch", units, tiles);
    switch (MT * 10 + SW) {
    case 11: bf_mfma_launch<1, 1, POWER>(bf, L, units, tiles, st); break;
    case 12: bf_mfma_launch<1, 2, POWER>(bf, L, units, tiles, st); break;
    case 13: bf_mfma_launch<1, 3, POWER>(bf, L, units, tiles, st); break;
    case 14: bf_mfma_launch<1, 4, POWER>(bf, L, units, tiles, st); break;
    case 21: bf_mfma_launch<2, 1, POWER>(bf, L, units, tiles, st); break;
    case 22: bf_mfma_launch<2, 2, POWER>(bf, L, units, tiles, st); break;
    case 23: bf_mfma_launch<2, 3, POWER>(bf, L, units, tiles, st); break;
    case 24: bf_mfma_launch<2, 4, POWER>(bf, L, units, tiles, st); break;
    case 31: bf_mfma_launch<3, 1, POWER>(bf, L, units, tiles, st); break;
    case 32: bf_mfma_launch<3, 2, POWER>(bf, L, units, tiles, st); break;
    case 33: bf_mfma_launch<3, 3, POWER>(bf, L, units, tiles, st); break;
    case 34: bf_mfma_launch<3, 4, POWER>(bf, L, units, tiles, st); break;
    case 41: bf_mfma_launch<4, 1, POWER>(bf, L, units, tiles, st); break;
    case 42: bf_mfma_launch<4, 2, POWER>(bf, L, units, tiles, st); break;
    case 43: bf_mfma_launch<4, 3, POWER>(bf, L, units, tiles, st); break;
    case 44: bf_mfma_launch<4, 4, POWER>(bf, L, units, tiles, st); break;
    default: set_error("beamform: internal: no matrix-pipe kernel for %zu streams and %zu beams", bf->S, bf->B); return GR4HIP_RUNTIME_ERROR;
    }
    return GR4HIP_OK;
}

template <bool POWER>
static int bf_run(gr4hip_beamform* bf, const BfLaunch& L, hipStream_t st) {
    const int  path  = bf_path(bf);
    const long units = POWER ? L.geom.nl : ceil_div(L.n_frames, (long)kBfChunk);
    if (const int rc = path == 1 ? bf_valu<POWER>(bf, L, units, st) : bf_mfma<POWER>(bf, L, units, st)) return rc;
    GR4_LAUNCH_CHECK();
    bf->last_path = path;
    return GR4HIP_OK;
}

// rows a + f T and b + g T (f, g < n) of W bytes each, W <= T: whether any two of them share a byte
static bool bf_rows_overlap(uintptr_t a, uintptr_t b, size_t T, size_t W, size_t n) {
    const uintptr_t d = a < b ? b - a : a - b;
    const size_t    m = d / T, r = d % T;
    return (m <= n - 1 && r < W) || (m + 1 <= n - 1 && T - r < W);
}

static int bf_inputs(const gr4hip_beamform* bf, const char* who, const float* const* d_spectra, BfIn* in) {
    GR4_REQUIRE(d_spectra, "%s: null array of inputs", who);
    for (size_t s = 0; s < bf->S; ++s) {
        GR4_REQUIRE(d_spectra[s], "%s: null input %zu", who, s);
        GR4_REQUIRE((uintptr_t)d_spectra[s] % 8 == 0, "%s: input %zu must be aligned to 8 bytes", who, s);
        in->s[s] = d_spectra[s];
    }
    return GR4HIP_OK;
}

} // namespace gr4

extern "C" {

int gr4hip_beamform_create(gr4hip_beamform_t** out, size_t n_streams, size_t n_beams, size_t n_bins) {
    GR4_REQUIRE(out, "beamform: null output handle");
    GR4_REQUIRE(n_streams >= 1, "beamform: n_streams must be >= 1");
    GR4_REQUIRE(n_beams >= 1, "beamform: n_beams must be >= 1");
    GR4_REQUIRE(n_bins >= 2, "beamform: n_bins must be >= 2 (got %zu)", n_bins);
    if (n_streams > (size_t)kBfMax || n_beams > (size_t)kBfMax) { set_error("beamform: %zu streams, %zu beams (supported: up to %d of each)", n_streams, n_beams, kBfMax); return GR4HIP_UNSUPPORTED; }
    if (n_bins > kBfMaxBins) { set_error("beamform: %zu bins (supported: up to %zu)", n_bins, kBfMaxBins); return GR4HIP_UNSUPPORTED; }
    if (n_beams * n_streams * n_bins > kBfMaxWeights) { set_error("beamform: %zu weights (supported: up to %zu)", n_beams * n_streams * n_bins, kBfMaxWeights); return GR4HIP_UNSUPPORTED; }
    auto* bf = new (std::nothrow) gr4hip_beamform();
    GR4_REQUIRE(bf, "out of host memory");
    bf->S = n_streams;
    bf->B = n_beams;
    bf->N = n_bins;
    *out  = bf; // the device buffers come with the first set_weights: everything up to there is host code
    return GR4HIP_OK;
}

int gr4hip_beamform_set_weights(gr4hip_beamform_t* bf, const float* d_weights, gr4hip_stream_t stream) {
    GR4_REQUIRE(bf, "beamform_set_weights: null handle");
    GR4_REQUIRE(d_weights, "beamform_set_weights: null weights");
    GR4_REQUIRE((uintptr_t)d_weights % 8 == 0, "beamform_set_weights: the weights must be aligned to 8 bytes");
    if (const int rc = have_device("beamform")) return rc;
    const size_t bytes = bf->B * bf->S * bf->N * 2 * sizeof(float);
    if (const int rc = bf->d_w.ensure(bytes)) return rc;
    GR4_HIP_TRY(hipMemcpyAsync(bf->d_w.ptr, d_weights, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    bf->have_w       = true;
    bf->frag_current = false; // arranged into fragment order by the first matrix-pipe launch behind this copy
    return GR4HIP_OK;
}

int gr4hip_beamform_process(gr4hip_beamform_t* bf, const float* const* d_spectra, size_t n_frames, float* const* d_beams, size_t out_frame_stride, gr4hip_stream_t stream) {
    GR4_REQUIRE(bf, "beamform_process: null handle");
    if (n_frames == 0) return GR4HIP_OK;
    GR4_REQUIRE(bf->have_w, "beamform_process: no weights yet (gr4hip_beamform_set_weights)");
    GR4_REQUIRE(d_beams, "beamform_process: null array of outputs");
    GR4_REQUIRE(out_frame_stride >= bf->N, "beamform_process: out_frame_stride %zu is below n_bins %zu", out_frame_stride, bf->N);
    GR4_REQUIRE(n_frames <= (size_t(1) << 40) / bf->N && n_frames <= (size_t(1) << 40) / out_frame_stride, "beamform_process: %zu frames of %zu bins (stride %zu) in one call", n_frames, bf->N,
                out_frame_stride);
    BfLaunch L{};
    if (const int rc = bf_inputs(bf, "beamform_process", d_spectra, &L.in)) return rc;
    const size_t T = out_frame_stride * 8, W = bf->N * 8, span = (n_frames - 1) * T + W, in_bytes = n_frames * W;
    for (size_t b = 0; b < bf->B; ++b) {
        GR4_REQUIRE(d_beams[b], "beamform_process: null output %zu", b);
        GR4_REQUIRE((uintptr_t)d_beams[b] % 8 == 0, "beamform_process: output %zu must be aligned to 8 bytes", b);
        const uintptr_t o0 = (uintptr_t)d_beams[b], o1 = o0 + span;
        for (size_t s = 0; s < bf->S; ++s) {
            const uintptr_t a0 = (uintptr_t)d_spectra[s], a1 = a0 + in_bytes;
            GR4_REQUIRE(a1 <= o0 || o1 <= a0, "beamform_process: output %zu overlaps input %zu", b, s);
        }
        for (size_t a = 0; a < b; ++a) GR4_REQUIRE(!bf_rows_overlap((uintptr_t)d_beams[a], o0, T, W, n_frames), "beamform_process: the rows of outputs %zu and %zu overlap", a, b);
        L.out.b[b] = d_beams[b];
    }
    L.n_frames = (long)n_frames;
    L.stride   = (long)out_frame_stride;
    return bf_run<false>(bf, L, as_stream(stream));
}

int gr4hip_beamform_power_integrate(gr4hip_beamform_t* bf, gr4hip_specint_t* si, const float* const* d_spectra, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream) {
    const char* who = "beamform_power_integrate";
    GR4_REQUIRE(bf, "%s: null handle", who);
    const size_t M = bf->B * bf->N;
    if (n_frames == 0) {
        if (const int rc = specint_check(si, who, M, nullptr, 0, 8, 0, d_out, n_out)) return rc;
        *n_out = 0;
        return GR4HIP_OK;
    }
    GR4_REQUIRE(si, "%s: null integrator handle", who);
    GR4_REQUIRE(n_out, "%s: null n_out", who);
    GR4_REQUIRE(bf->have_w, "%s: no weights yet (gr4hip_beamform_set_weights)", who);
    GR4_REQUIRE(n_frames <= (size_t(1) << 40) / bf->N, "%s: %zu frames of %zu bins in one call", who, n_frames, bf->N);
    BfLaunch L{};
    if (const int rc = bf_inputs(bf, who, d_spectra, &L.in)) return rc;
    for (size_t s = 0; s < bf->S; ++s) // the integrator's own refusals, per input: bins, null output, alignment, overlap
        if (const int rc = specint_check(si, who, M, d_spectra[s], bf->N * 8, 8, n_frames, d_out, n_out)) return rc;
    const size_t      n     = si->integ.pending(n_frames);
    const hipStream_t st    = as_stream(stream);
    const size_t      piece = std::max<size_t>(1, kBfPieceValues / (bf->N * std::max(bf->S, bf->B)));
    const BfIn        in0   = L.in;
    const int         rc    = si->integ.for_each_piece(n_frames, piece, d_out, [&](size_t f, size_t m, float* out) {
        for (size_t s = 0; s < bf->S; ++s) L.in.s[s] = in0.s[s] + f * bf->N * 2;
        SpecintLaunch SL;
        if (const int rc = specint_begin(si, m, st, &SL)) return rc;
        L.n_frames = (long)m;
        L.geom     = SL.geom;
        L.carry    = SL.carry;
        L.leaves   = SL.leaves;
        if (const int rc = bf_run<true>(bf, L, st)) return rc;
        return specint_finish(si, SL, out, 1, st);
    });
    if (rc) return rc;
    *n_out = n;
    return GR4HIP_OK;
}

int gr4hip_beamform_destroy(gr4hip_beamform_t* bf) {
    delete bf;
    return GR4HIP_OK;
}

// test hook (exported, not declared in include/gr4hip.h): which kernel the last call ran -- 1 = the VALU form, 2 = the matrix-pipe form (0: no call yet)
int gr4hip_internal_beamform_last_path(gr4hip_beamform_t* bf, int* path) {
    GR4_REQUIRE(bf && path, "beamform_last_path: bad arguments");
    *path = bf->last_path;
    return GR4HIP_OK;
}

// test hook: 1 = the VALU form where it exists (S <= 8 with B <= 8; elsewhere the matrix-pipe form runs and last_path says so), 2 = the matrix-pipe form, 0 = the default
int gr4hip_internal_beamform_set_path(gr4hip_beamform_t* bf, int path) {
    GR4_REQUIRE(bf && path >= 0 && path <= 2, "beamform_set_path: bad arguments");
    bf->force_path = path;
    return GR4HIP_OK;
}

} // extern "C"
