// stft_kernels.hpp -- device code of the overlapped / skipped FFT frames (OVERLAPPED_FFT.md) shared by stft.hip and fft_fast_pk.hip: the hop front end that
// replaces the FFT block's first-pass load, the kernels that run the FFT block's own passes and epilogue behind it (fft_fast_frames.inc), and what stft.hip
// needs of the FFT block's handle (fft.hip).
//
//   frame m of a launch = the N complex samples x[m S .. m S + N)   ->   window -> forward DFT -> every output of the FFT block, per frame
#pragma once
#include "fft_kernels.hpp"

struct gr4hip_fft;

namespace gr4 {

// ---- the FFT block as a building block (fft.hip)
struct FftBlockView {
    size_t        N;
    int           in_dtype, kind /* gr4hip_fft_plan's, 3 folded into 0 */, smooth;
    const float*  window; // null: none
    const float2* tw;     // W_N^j, kind 0
};
FftBlockView fft_block_view(const gr4hip_fft* f);
using FftFrontLaunch = int (*)(void* ctx, const FftOutputs& o, long n_frames, hipStream_t st);
int fft_block_run(gr4hip_fft* f, const void* d_in, size_t n_frames, const FftOutputs& o, float* d_phase, float* d_ranges, FftFrontLaunch front, void* ctx, gr4hip_stream_t stream);

constexpr size_t kStftMaxStride = size_t(1) << 20; // the group's span and every lane offset stay 32-bit: 31 strides + 8192 points are 2^28 bytes

// Front end of fft_fast_frames.inc: lane t of frame slot fl gets the points t + r N/16, r = 0 .. 15, of frame f0 + fl, which starts S samples behind its
// predecessor.  One descriptor per group of frame slots with the exact range of the group's span, (nlive - 1) S + N samples; the frame-dependent part of the
// address is in the lane offset, and a slot past the last frame gets an offset beyond every range: it reads 0 and nothing outside the span.  The window multiply
// is the frame loop's own statement (the kernel hands it the window), so the values are those of fft_fast_kernel on the materialised frame.  The loads carry no
// streaming hint: with S < N every sample is read by N / S frames, from the L2 after the first.
struct HopFront {
    static constexpr bool kFrontEnd = true, kSink = false;
    const float* x; // frame 0 of the launch, interleaved complex
    long         S; // samples between frame starts, 1 .. kStftMaxStride
    __device__ __forceinline__ void sink(const float (&)[16]) const {}
    static __device__ __forceinline__ long first_group() { return blockIdx.x; } // one group per workgroup, grid-stride beyond 2^31 groups
    static __device__ __forceinline__ long end_group(long ngroups) { return ngroups; }
    static __device__ __forceinline__ long group_stride() { return gridDim.x; }
    template <int FPB> static __device__ __forceinline__ long group(long g, long) { return g; }

    template <int N>
    __device__ __forceinline__ void load(float2 (&v)[16], long f0, unsigned nlive, int fl, int t) const {
        constexpr int T    = N / 16;
        constexpr int kOut = 0x40000000; // a lane offset beyond every range here (the largest is 31 strides of 2^20 samples + 8192 points: 2^28 bytes)
        const rsrc_t  rx   = make_rsrc(x + f0 * S * 2, (unsigned)(((long)nlive - 1) * S + N) * 8u);
        const int     vo   = (unsigned)fl < nlive ? (int)(((long)fl * S + t) * 8) : kOut;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const auto q = __builtin_amdgcn_raw_buffer_load_b64(rx, vo, r * T * 8, 0);
            v[r]         = make_float2(__uint_as_float(q[0]), __uint_as_float(q[1]));
        }
    }
};

// N = 256 .. 8192: fft_fast_kernel's plans, workgroups, LDS layout, launch bounds and register epilogue behind the hop front end
template <int LOG2N>
__global__ __launch_bounds__(512, 4) void hop_fast_kernel(HopFront front, const float* __restrict__ window, const float2* __restrict__ tw, FftOutputs out, long n_frames) {
    using FRONT = HopFront;
    constexpr bool REAL = false;
    const float*   in   = nullptr; // the FFT block's own load: not used behind a front end
#include "fft_fast_frames.inc"
}

template <int LOG2N>
static int hop_fast_launch(const HopFront& front, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) {
    constexpr int    N = 1 << LOG2N, FPB = 512 / (N / 16);
    constexpr size_t lds = (size_t)FPB * (N + N / 32) * sizeof(float2);
    static PerDevice per_device; // the > 64 KiB LDS opt-in is per device
    bool             first = false;
    int              dev = -1;
    const int        n_cu = per_device.current(&first, &dev);
    GR4_REQUIRE(n_cu != 0, "stft: cannot query the current device");
    if (first) {
        GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(hop_fast_kernel<LOG2N>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        per_device.done(dev, -n_cu);
    }
    const long groups = (n_frames + FPB - 1) / FPB; // one workgroup per group of frame slots, like fft_fast_launch
    const long grid   = groups < 0x7fffffffL ? groups : 0x7fffffffL;
    hipLaunchKernelGGL(hop_fast_kernel<LOG2N>, dim3((unsigned)grid), dim3(512), lds, st, front, d_window, d_tw, o, n_frames);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

// the two sizes compiled with the SLP vectoriser on, like the FFT block's (fft_fast_pk.hip)
int hop_fast_launch_256(const HopFront& front, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st);
int hop_fast_launch_8192(const HopFront& front, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st);

} // namespace gr4
