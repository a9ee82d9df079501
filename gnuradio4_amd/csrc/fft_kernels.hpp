// fft_kernels.hpp -- device code of the FFT block shared by fft.hip and fft_fast_pk.hip: small DFTs, the output epilogue and the
// compile-time-plan kernel fft_fast_kernel<log2 N> with its launcher.  (Two translation units because hipcc's SLP vectoriser --
// v_pk_add/mul/fma_f32 on register pairs it has to assemble with v_mov -- costs 7-13 % at N = 1024 / 4096 and GAINS 15-17 % at
// N = 256 / 8192: the library is built with -fno-slp-vectorize except fft_fast_pk.hip, which instantiates those two sizes.)
#pragma once
#include "common.hpp"
#include "buffer_ops.hpp"
#include "fft_radix.hpp"
#include "ewise.hpp"

#include <cfloat>
#include <cmath>
#include <complex>
#include <type_traits>


namespace gr4 {

struct FftPlanDev {
    int N;
    int npass;
    int radix[16];
    int tf;  // threads per frame
    int fpb; // frames per block
    int smooth; // 1: mixed-radix plan of fft_smooth.hpp (radices 2 .. 16, N not a power of two)
};

struct FftOutputs {
    float* spectrum;  // [frames][N][2]
    float* re;        // complex in: [frames][N]; real in: [frames][N/2] (bins N/2..N-1, fft.hpp:221-227)
    float* im;
    float* mag;       // shifted (complex) / first half (real)
    float* phase;     // final phase when !unwrap
    float* phase_raw; // natural-order raw atan2 (only when unwrap; finished by unwrap_kernel)
    float* mag2;      // natural order
    float* ranges;    // fast kernels only: [frames][4][2] {min, max} of magnitude, phase, Re, Im (fft.hpp:229-232); null = not requested
    int    in_db, in_deg, real_input;
    EwiseHook mag2_post; // per-sample float blocks behind a PowerSpectrum (MultiplyConst / AddConst ...: gr4hip_fft_set_epilogue): applied to |X|^2 before its store
};

// every requested output of one natural-order bin k of one frame (fft.hpp:164-166, fft_common.hpp:20-56, 91-123)
__device__ __forceinline__ void emit_bin(const FftOutputs& out, long frame, int N, int k, float2 X) {
    const int half = N / 2;
    const int nout = out.real_input ? half : N;
    if (out.spectrum) reinterpret_cast<float2*>(out.spectrum)[frame * N + k] = X;
    if (out.mag2) {
        float m = fmaf(X.x, X.x, X.y * X.y);
        if (out.mag2_post.n_ops > 0) m = ewise_hook1<float>(m, out.mag2_post, frame * N + k);
        out.mag2[frame * N + k] = m;
    }
    if (out.real_input) {
        if (k >= half) {
            if (out.re) out.re[frame * half + (k - half)] = X.x;
            if (out.im) out.im[frame * half + (k - half)] = X.y;
        }
    } else {
        if (out.re) out.re[frame * N + k] = X.x;
        if (out.im) out.im[frame * N + k] = X.y;
    }
    if (out.real_input && k >= half) return; // computeHalfSpectrum: first N/2 bins, never rotated
    const int ko = out.real_input ? k : (k + N - half) % N; // shiftSpectrum = std::rotate by N/2: bin N/2 comes first (odd N on the Bluestein path)
    if (out.mag) {
        float m = hypotf(X.x, X.y) * 2.f / (float)N;
        if (out.in_db) m = (m > 0.f) ? 20.f * log10f(m) : -FLT_MAX;
        out.mag[frame * nout + ko] = m;
    }
    if (out.phase || out.phase_raw) {
        float ph = atan2f(X.y, X.x);
        if (out.phase_raw) {
            out.phase_raw[frame * nout + k] = ph;
        } else {
            if (out.in_deg) ph = ph * 180.f * 0.318309886183790671538f;
            out.phase[frame * nout + ko] = ph;
        }
    }
}

// ---- the run-time plan (radix 8 / 4 / 2 passes over a frame in LDS): fft_block_kernel, the fused Bluestein kernel (fft.hip) and pfb_block_kernel
template <int R>
__device__ __forceinline__ void load_bfly(float2* v, const float2* __restrict__ src, int i, int NB, int p, int step_unit, const float2* __restrict__ tw) {
    const int k = i & (p - 1);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float2 x = src[i + r * NB];
        if (r > 0 && p > 1) x = cmulf(x, tw[r * k * step_unit]);
        v[r] = x;
    }
}

template <int R>
__device__ __forceinline__ void store_bfly(const float2* v, float2* dst, int i, int p) {
    const int k    = i & (p - 1);
    const int base = (i - k) * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) dst[base + r * p] = v[r];
}

// the Stockham passes of one frame that sits in LDS (natural order in, natural order out); every lane of the workgroup calls it (it synchronises)
__device__ __forceinline__ void lds_passes(float2* buf, int t, int tf, const FftPlanDev& plan, const float2* __restrict__ tw) {
    const int N = plan.N;
    int p = 1;
    for (int pass = 0; pass < plan.npass; ++pass) {
        const int R  = plan.radix[pass];
        const int NB = N / R;
        const int nb = NB / tf > 0 ? NB / tf : 1;
        const int su = N / (p * R); // twiddle index unit: W_{pR}^{rk} = tw[r*k*su]
        float2    v[8];
        if (R == 8) {
            if (t < NB) load_bfly<8>(v, buf, t, NB, p, su, tw);
        } else if (R == 4) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (b < nb && t + b * tf < NB) load_bfly<4>(v + 4 * b, buf, t + b * tf, NB, p, su, tw);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < nb && t + b * tf < NB) load_bfly<2>(v + 2 * b, buf, t + b * tf, NB, p, su, tw);
        }
        __syncthreads();
        if (R == 8) {
            if (t < NB) { fft8(v); store_bfly<8>(v, buf, t, p); }
        } else if (R == 4) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (b < nb && t + b * tf < NB) { fft4(v[4 * b], v[4 * b + 1], v[4 * b + 2], v[4 * b + 3]); store_bfly<4>(v + 4 * b, buf, t + b * tf, p); }
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < nb && t + b * tf < NB) { fft2(v[2 * b], v[2 * b + 1]); store_bfly<2>(v + 2 * b, buf, t + b * tf, p); }
        }
        __syncthreads();
        p *= R;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Fast path for N = 256 ... 8192: compile-time Stockham plan 16 x 16 x R3 (x 2 for 8192), 16 points per lane, 512 lanes =
// 512 / (N/16) frames per workgroup iteration, persistent workgroups (2 per CU).  The first pass reads its 16 points per lane
// straight from global memory (window fused), the last pass emits every output straight from registers (lane t holds bins
// t + j N/16: coalesced), so a frame makes 2 (N <= 4096: 16 x 16 x R3) or 3 LDS round trips instead of log8(N) + 1, all of them
// through a buffer padded by one float2 per 32 (the stride-16 scatter of the first pass is conflict-free).  Twiddles: one or two
// table values per lane and pass live in registers, the powers b^r come from two interleaved chains (depth <= 7).

// REAL = true: a frame of 2N REAL samples is transformed as N complex points z[n] = x[2n] + i x[2n+1] (the float array read as float2,
// window pairs likewise) and split afterwards:  X[k] = (Z[k] + conj Z[N-k]) / 2 + W_2N^k (Z[k] - conj Z[N-k]) / (2i),  k = 0 .. N
// -- half the butterflies of the "imaginary part = 0" form.  tw is then the table of W_2N^j (every second entry is W_N^j), and the
// outputs follow the real-input conventions of the block: magnitude / phase = bins 0..N-1, Re / Im = bins N..2N-1 = conj of bins N..1.
//
// The body of the kernel is fft_fast_frames.inc, included here and by the polyphase filter bank's kernel (pfb_kernels.hpp): the same passes and epilogue
// behind another first-pass load.  FRONT::kFrontEnd = false is the FFT block's load (frame x window); true hands the lane's 16 points to front.load().
struct FftWindowFront {
    static constexpr bool kFrontEnd = false, kSink = false;
    template <int N> __device__ __forceinline__ void load(float2 (&)[16], long, unsigned, int, int) const {}
    __device__ __forceinline__ void sink(const float (&)[16]) const {} // kSink = true: takes the lane's 16 values of |X|^2 instead of their store
    static __device__ __forceinline__ long first_group() { return blockIdx.x; }
    static __device__ __forceinline__ long end_group(long ngroups) { return ngroups; }
    static __device__ __forceinline__ long group_stride() { return gridDim.x; }
    template <int FPB> static __device__ __forceinline__ long group(long g, long) { return g; } // which group of frames workgroup iteration g takes
};
// A front that declares kBinSink = true also takes the lane's 16 register-held bins, with their positions, in place of every store of the epilogue (the inverse
// transform, ifft_kernels.hpp).  The fronts above and the bank's do not name it: for them the body compiles to what it was.
template <class F, class = void> struct front_bin_sink { static constexpr bool value = false; };
template <class F> struct front_bin_sink<F, std::enable_if_t<F::kBinSink>> { static constexpr bool value = true; };
template <int N, int ST, class F>
__device__ __forceinline__ void front_store_bins(const F& front, const float2 (&X)[16], long f0, unsigned nlive, int eN, int nN) {
    if constexpr (front_bin_sink<F>::value) front.template store<N, ST>(X, f0, nlive, eN, nN);
}

template <int LOG2N, bool REAL = false>
__global__ __launch_bounds__(512, 4) void fft_fast_kernel(const float* __restrict__ in, const float* __restrict__ window, const float2* __restrict__ tw,
                                                          FftOutputs out, long n_frames) {
    using FRONT = FftWindowFront;
    const FRONT front{};
#include "fft_fast_frames.inc"
}

template <int LOG2N, bool REAL = false>
static int fft_fast_launch(const float* d_in, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) {
    constexpr int    N = 1 << LOG2N, FPB = 512 / (N / 16);
    constexpr size_t lds = (size_t)FPB * (N + N / 32) * sizeof(float2);
    static PerDevice per_device; // the > 64 KiB LDS opt-in is per device
    bool             first = false;
    int              dev = -1;
    const int        n_cu = per_device.current(&first, &dev);
    GR4_REQUIRE(n_cu != 0, "fft: cannot query the current device");
    if (first) {
        GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fft_fast_kernel<LOG2N, REAL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        per_device.done(dev, -n_cu);
    }
    const long groups = (n_frames + FPB - 1) / FPB;
    // one workgroup per group of frames, not a persistent grid: measured +8 ... 13 % at N <= 1024, +7 % at 8192 (the dispatcher refills a CU as soon as
    // a workgroup retires, and the per-workgroup set-up is two twiddle loads per lane); the frame loop in the kernel only matters beyond 2^31 groups
    const long grid   = groups < 0x7fffffffL ? groups : 0x7fffffffL;
    hipLaunchKernelGGL((fft_fast_kernel<LOG2N, REAL>), dim3((unsigned)grid), dim3(512), lds, st, d_in, d_window, d_tw, o, n_frames);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}


// the two sizes whose kernels are compiled with the SLP vectoriser on (fft_fast_pk.hip)
int fft_fast_launch_256(const float* d_in, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st);
int fft_fast_launch_8192(const float* d_in, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st);

} // namespace gr4
