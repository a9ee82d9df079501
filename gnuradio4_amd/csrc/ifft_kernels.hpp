// ifft_kernels.hpp -- device code of the inverse transform (INVERSE_FFT.md) shared by ifft.hip and fft_fast_pk.hip: the first-pass load and the last-pass
// store that turn the FFT block's forward kernel body (fft_fast_frames.inc) into the unnormalised inverse,
//
//   x[n] = sum_{k < N} X[k] e^{+2 pi i k n / N} = conj( FFT( conj X ) )[n]
//
// A sign flip is exact and round-to-nearest is sign-symmetric, so this is bit for bit a transform with conjugated twiddles: the load conjugates the bins, the
// passes are the forward kernel's own statements, the store conjugates again, scales (GR4HIP_IFFT_SCALE: 1 / N, exact), multiplies by the synthesis window and
// writes.  C2R reads the Hermitian expansion of bins 0 .. N/2 (bin k > N/2 is the conjugate of bin N - k; the imaginary parts of bins 0 and N/2 are dropped)
// and stores the real parts only: the imaginary half of the last pass is dead code there.
#pragma once
#include "fft_kernels.hpp"

namespace gr4 {

// Front end AND bin sink of fft_fast_frames.inc.  Lane t of frame slot fl loads bins t + r N/16, r = 0 .. 15, of frame f0 + fl and, after the passes, holds
// the 16 results X[j] = sample eN + j ST of the group ([FPB][N]; at 8192 points one frame, the lane-pair layout of the body's last radix-2).
// The optimiser must see between the two what it sees in the forward kernel -- values that come out of a load and go into a store as bit patterns -- or it folds
// the sign flips into the first and last butterflies, picks other multiply-add contractions there and the last bits differ.  So the conjugated bins (and the
// results, before they are conjugated) pass through an empty asm as the 8-byte register pairs the forward kernel loads and stores.
__device__ __forceinline__ float2 ifft_opaque(float2 a) {
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    u32x2 d = {__float_as_uint(a.x), __float_as_uint(a.y)};
    asm("" : "+v"(d));
    return make_float2(__uint_as_float(d[0]), __uint_as_float(d[1]));
}

template <bool C2R>
struct IfftFront {
    static constexpr bool kFrontEnd = true, kSink = false, kBinSink = true;
    const float* in;     // [frames][N] complex bins
    float*       out;    // C2C: [frames][N] complex; C2R: [frames][N] float
    const float* window; // N floats or null
    float        scale;  // 1 or 1 / N
    __device__ __forceinline__ void sink(const float (&)[16]) const {}
    static __device__ __forceinline__ long first_group() { return blockIdx.x; }
    static __device__ __forceinline__ long end_group(long ngroups) { return ngroups; }
    static __device__ __forceinline__ long group_stride() { return gridDim.x; }
    template <int FPB> static __device__ __forceinline__ long group(long g, long) { return g; }

    template <int N>
    __device__ __forceinline__ void load(float2 (&v)[16], long f0, unsigned nlive, int fl, int t) const {
        constexpr int T  = N / 16;
        const rsrc_t  rx = make_rsrc(in + f0 * N * 2, nlive * N * 8u); // a frame slot past the call's frames reads zeros
        const int     vN = fl * N + t;
        if constexpr (!C2R) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float2 s = buf_load_f2(rx, vN * 8, r * T * 8);
                v[r]           = ifft_opaque(make_float2(s.x, -s.y));
            }
        } else {
            // bins t + r T: r < 8 lie below N/2 (conjugated like the above), r >= 8 at or above it: bin k >= N/2 is the conjugate of bin N - k = (16 - r) T - t,
            // conjugated twice.  Bins 0 and N/2 (lane 0, r = 0 and 8) are real.  (The whole offset is in the lane part: the range check sees only that.)
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float2 s = buf_load_f2(rx, vN * 8, r * T * 8);
                v[r]           = ifft_opaque(make_float2(s.x, r == 0 && t == 0 ? -0.f : -s.y));
            }
#pragma unroll
            for (int r = 8; r < 16; ++r) {
                const float2 s = buf_load_f2(rx, (fl * N + (16 - r) * T - t) * 8, 0);
                v[r]           = ifft_opaque(make_float2(s.x, r == 8 && t == 0 ? -0.f : s.y));
            }
        }
    }

    // X[j] = sample eN + j ST of the group, sample nN + j ST of its frame
    template <int N, int ST>
    __device__ __forceinline__ void store(const float2 (&X)[16], long f0, unsigned nlive, int eN, int nN) const {
        float2 y[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float2 b = ifft_opaque(X[j]);
            y[j]           = make_float2(b.x * scale, -b.y * scale);
        }
        if (window) {
            const rsrc_t rw = make_rsrc(window, N * 4u);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rw, nN * 4, j * ST * 4, 0)); // (read by every frame: no streaming hint)
                y[j]          = make_float2(y[j].x * w, y[j].y * w);
            }
        }
        if constexpr (C2R) {
            const rsrc_t r = make_rsrc(out + f0 * N, nlive * N * 4u);
#pragma unroll
            for (int j = 0; j < 16; ++j) buf_store_f(r, y[j].x, eN * 4, j * ST * 4);
        } else {
            const rsrc_t r = make_rsrc(out + f0 * N * 2, nlive * N * 8u);
#pragma unroll
            for (int j = 0; j < 16; ++j) buf_store_f2(r, y[j], eN * 8, j * ST * 8);
        }
    }
};

// N = 256 .. 8192: fft_fast_kernel's plans, workgroups and LDS layout between the two
template <int LOG2N, bool C2R>
__global__ __launch_bounds__(512, 4) void ifft_fast_kernel(IfftFront<C2R> front, const float2* __restrict__ tw, long n_frames) {
    using FRONT = IfftFront<C2R>;
    constexpr bool   REAL = false;
    const float *    in = nullptr, *window = nullptr; // the FFT block's own load, window and outputs: not used between a front end and a bin sink
    const FftOutputs out{};
#include "fft_fast_frames.inc"
}

template <int LOG2N, bool C2R>
static int ifft_fast_launch_t(const float* d_in, float* d_out, const float* d_window, float scale, const float2* d_tw, long n_frames, hipStream_t st) {
    constexpr int    N = 1 << LOG2N, FPB = 512 / (N / 16);
    constexpr size_t lds = (size_t)FPB * (N + N / 32) * sizeof(float2);
    static PerDevice per_device; // the > 64 KiB LDS opt-in is per device
    bool             first = false;
    int              dev = -1;
    const int        n_cu = per_device.current(&first, &dev);
    GR4_REQUIRE(n_cu != 0, "ifft: cannot query the current device");
    if (first) {
        GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(ifft_fast_kernel<LOG2N, C2R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        per_device.done(dev, -n_cu);
    }
    const long groups = (n_frames + FPB - 1) / FPB; // one workgroup per group of frame slots, like fft_fast_launch
    const long grid   = groups < 0x7fffffffL ? groups : 0x7fffffffL;
    hipLaunchKernelGGL((ifft_fast_kernel<LOG2N, C2R>), dim3((unsigned)grid), dim3(512), lds, st, IfftFront<C2R>{d_in, d_out, d_window, scale}, d_tw, n_frames);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

template <int LOG2N>
static int ifft_fast_launch(bool c2r, const float* d_in, float* d_out, const float* d_window, float scale, const float2* d_tw, long n_frames, hipStream_t st) {
    return c2r ? ifft_fast_launch_t<LOG2N, true>(d_in, d_out, d_window, scale, d_tw, n_frames, st) : ifft_fast_launch_t<LOG2N, false>(d_in, d_out, d_window, scale, d_tw, n_frames, st);
}

// the two sizes compiled with the SLP vectoriser on, like the FFT block's (fft_fast_pk.hip): the same statements have to give the same values
int ifft_fast_launch_256(bool c2r, const float* d_in, float* d_out, const float* d_window, float scale, const float2* d_tw, long n_frames, hipStream_t st);
int ifft_fast_launch_8192(bool c2r, const float* d_in, float* d_out, const float* d_window, float scale, const float2* d_tw, long n_frames, hipStream_t st);

} // namespace gr4
