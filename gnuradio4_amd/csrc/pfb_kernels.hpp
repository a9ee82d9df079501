// pfb_kernels.hpp -- device code of the polyphase filter bank (PFB.md) shared by pfb.hip and fft_fast_pk.hip: the front end that replaces the FFT
// block's windowed load, and the kernels that run the FFT block's own passes behind it (fft_fast_frames.inc / lds_passes, fft_kernels.hpp).
//
//   u_m[i] = sum_{k < P} h[k N + i] x[(m - P + 1 + k) N + i]      float32, k ascending from u = 0: one fma per term and component
//
// Frame m of a call needs the input frames m - P + 1 .. m; frames below 0 are the handle's history ([P - 1][N], oldest first).
#pragma once
#include "fft_kernels.hpp"

namespace gr4 {

// Front end of fft_fast_frames.inc: lane t of frame slot fl gets u[t + r N/16], r = 0 .. 15, of frame f0 + fl.  The simple form (PFB.md): every sample is
// read by the P frames that hold it, every tap by every frame; both come from the L2 after the first read (no streaming hint on these loads).
// Descriptors carry exact ranges: the taps [P N], the history [(P - 1) N], and of the input only the frames this group of frame slots needs and the
// call was given.  The frame-dependent part of an address is in the lane offset, so a frame outside the range reads 0 and nothing outside the spans.
struct PfbFront {
    static constexpr bool kFrontEnd = true, kSink = false;
    const float* x;    // the call's input, n_frames frames of N complex samples
    const float* hist; // the last P - 1 frames before it
    const float* taps; // h[P N]
    int          P;
    __device__ __forceinline__ void sink(const float (&)[16]) const {}

    // Workgroup g -> group of FPB frames.  Workgroups are dealt to the chip's 8 XCDs round-robin (g mod 8), and each XCD has its own L2: with group g itself, the
    // P - 1 frames a group shares with the one before it were read through ANOTHER XCD's L2.  Where those shared frames are at least a group's own (P - 1 >= FPB)
    // XCD x takes the x-th eighth of the groups, in order: the groups in flight on one XCD are neighbours, and a re-read finds its sample in that XCD's L2
    // (measured, PFB.md: N = 8192 P = 4 / 8 + 18 / + 46 %; N = 1024, 8 frames per group, - 4 / - 1 %, P = 1 - 4 %: those keep group g).  A permutation of the
    // groups whatever the hardware does with the workgroups: only the rate depends on the dealing.
    template <int FPB>
    __device__ __forceinline__ long group(long g, long ngroups) const {
        if (P - 1 < FPB) return g;
        constexpr long kXcds = 8;
        const long     x = g % kXcds, q = ngroups / kXcds, r = ngroups % kXcds;
        return x * q + (x < r ? x : r) + g / kXcds;
    }

    static __device__ __forceinline__ long first_group() { return blockIdx.x; } // one group per workgroup, grid-stride beyond 2^31 groups
    static __device__ __forceinline__ long end_group(long ngroups) { return ngroups; }
    static __device__ __forceinline__ long group_stride() { return gridDim.x; }

    static __device__ __forceinline__ float2 ld2(rsrc_t r, int voff, int soff) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
        return make_float2(__uint_as_float(v[0]), __uint_as_float(v[1]));
    }
    static __device__ __forceinline__ float ld1(rsrc_t r, int voff, int soff) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0)); }

    // points r = R0 .. R0 + NR - 1 of the lane: the sum over the P frames that start at frame `first` of the span behind rx (PAST: frames below 0 come from the
    // history behind rp instead: two loads, one of them out of range, and a select -- a descriptor is wave-uniform, the frame slot is not)
    template <int N, int R0, int NR, bool PAST>
    __device__ __forceinline__ void part(float2 (&v)[16], rsrc_t rx, rsrc_t rp, rsrc_t rh, int first, int t) const {
        constexpr int T    = N / 16;
        constexpr int kOut = 0x40000000; // a lane offset beyond every range here (the largest is 63 frames of 8192 points: 4 MiB)
#pragma unroll
        for (int r = R0; r < R0 + NR; ++r) v[r] = make_float2(0.f, 0.f);
        for (int k = 0; k < P; ++k) {
            const int  f    = first + k;
            const bool past = PAST && f < 0;
            const int  ox = past ? kOut : (f * N + t) * 8, op = past ? ((P - 1 + f) * N + t) * 8 : kOut, oh = (k * N + t) * 4;
#pragma unroll
            for (int r = R0; r < R0 + NR; ++r) {
                float2 s = ld2(rx, ox, r * T * 8);
                if constexpr (PAST) {
                    const float2 b = ld2(rp, op, r * T * 8);
                    s = past ? b : s;
                }
                const float h = ld1(rh, oh, r * T * 4);
                v[r] = make_float2(fmaf(h, s.x, v[r].x), fmaf(h, s.y, v[r].y));
            }
        }
    }

    // The lane's 16 points in two halves (four quarters where the history is involved), each with its own loop over the taps: 16 accumulators and the 8 samples
    // and 8 taps of one step are live at a time.  (The sums start from 0, every term an fma: with the first term as a product hipcc peels that step out of the
    // loop and the 8192-point kernel spills 14 registers; this way every size has the registers of its fft_fast_kernel.)
    template <int N>
    __device__ __forceinline__ void load(float2 (&v)[16], long f0, unsigned nlive, int fl, int t) const {
        const rsrc_t rh = make_rsrc(taps, (unsigned)P * N * 4u);
        const long   fb = f0 - (P - 1); // the first input frame this group needs
        if (fb >= 0) {                  // every window of the group lies in the call's input
            const rsrc_t rx = make_rsrc(x + fb * N * 2, (nlive + (unsigned)P - 1u) * N * 8u);
            part<N, 0, 8, false>(v, rx, rx, rh, fl, t);
            part<N, 8, 8, false>(v, rx, rx, rh, fl, t);
        } else { // the first groups of a call (f0 < P - 1): input frame f < 0 is history frame P - 1 + f
            const rsrc_t rx = make_rsrc(x, (unsigned)(f0 + nlive) * N * 8u);
            const rsrc_t rp = make_rsrc(hist, ((unsigned)P - 1u) * N * 8u);
            part<N, 0, 4, true>(v, rx, rp, rh, (int)fb + fl, t);
            part<N, 4, 4, true>(v, rx, rp, rh, (int)fb + fl, t);
            part<N, 8, 4, true>(v, rx, rp, rh, (int)fb + fl, t);
            part<N, 12, 4, true>(v, rx, rp, rh, (int)fb + fl, t);
        }
    }
};

// The run form, N = 8192 (one frame per workgroup iteration) and PT = 2 .. 4 taps per channel: a workgroup walks a run of L consecutive frames and keeps each
// lane's last PT - 1 samples per point in registers (2 (PT - 1) 16 = 96 at PT = 4, beside the transform's 116: 256 registers per lane, one workgroup per CU).
// A frame then costs one read of its own samples and PT N taps; the first frame of a run reads its PT - 1 predecessors again (from the call's input, or from
// the history below frame 0 -- everything here is the same for the whole workgroup, so the descriptor is chosen, not the loaded value).
// The sums are those of PfbFront, term for term: the two forms give the same values.
template <int PT>
struct PfbRunFront {
    static constexpr bool kFrontEnd = true, kSink = false;
    const float* x;
    const float* hist;
    const float* taps;
    long         L;   // frames per workgroup
    float2*      win; // the lane's window [PT - 1][16], oldest first: an array of the kernel, in registers
    __device__ __forceinline__ void sink(const float (&)[16]) const {}

    __device__ __forceinline__ long first_group() const { return (long)blockIdx.x * L; }
    __device__ __forceinline__ long end_group(long ngroups) const { return first_group() + L < ngroups ? first_group() + L : ngroups; }
    static __device__ __forceinline__ long group_stride() { return 1; }
    template <int FPB> static __device__ __forceinline__ long group(long g, long) { return g; }

    template <int N>
    __device__ __forceinline__ void load(float2 (&v)[16], long f0, unsigned nlive, int, int t) const {
        static_assert(N == 8192, "one frame per workgroup iteration");
        constexpr int T = N / 16;
        if (f0 == first_group()) { // a new run: the PT - 1 frames in front of it
#pragma unroll
            for (int j = 0; j < PT - 1; ++j) {
                const long   f  = f0 - (PT - 1) + j; // >= -(PT - 1); below 0: history frame PT - 1 + f
                const rsrc_t rf = make_rsrc(f < 0 ? hist + (PT - 1 + f) * N * 2 : x + f * N * 2, N * 8u);
#pragma unroll
                for (int r = 0; r < 16; ++r) win[j * 16 + r] = PfbFront::ld2(rf, t * 8, r * T * 8);
            }
        }
        const rsrc_t rx = make_rsrc(x + f0 * N * 2, nlive * N * 8u), rh = make_rsrc(taps, PT * N * 4u);
        float2       s[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = PfbFront::ld2(rx, t * 8, r * T * 8);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = make_float2(0.f, 0.f);
#pragma unroll
        for (int k = 0; k < PT; ++k) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float  h = PfbFront::ld1(rh, (k * N + t) * 4, r * T * 4);
                const float2 q = k < PT - 1 ? win[k * 16 + r] : s[r];
                v[r] = make_float2(fmaf(h, q.x, v[r].x), fmaf(h, q.y, v[r].y));
            }
        }
#pragma unroll
        for (int k = 0; k + 1 < PT - 1; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) win[k * 16 + r] = win[(k + 1) * 16 + r];
#pragma unroll
        for (int r = 0; r < 16; ++r) win[(PT - 2) * 16 + r] = s[r];
    }
};

template <int LOG2N, int PT>
__global__ __launch_bounds__(512, 2) void pfb_run_kernel(const float* __restrict__ x, const float* __restrict__ hist, const float* __restrict__ taps, long L,
                                                         const float2* __restrict__ tw, FftOutputs out, long n_frames) {
    float2 win[(PT - 1) * 16];
    using FRONT = PfbRunFront<PT>;
    const FRONT    front{x, hist, taps, L, win};
    constexpr bool REAL = false;
    const float *  in = nullptr, *window = nullptr; // the FFT block's own load and window: not used behind a front end
#include "fft_fast_frames.inc"
}

// L frames per workgroup.  Measured slower than the simple form (PFB.md: one workgroup per CU costs more than the re-reads save), so the library takes it only
// where a run length was asked for (gr4hip_internal_pfb_set_run_length: the tests and the rates tool)
template <int LOG2N, int PT>
static int pfb_run_launch(const float* x, const float* hist, const float* taps, long L, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st, bool* taken) {
    constexpr int    N = 1 << LOG2N;
    constexpr size_t lds = (size_t)(N + N / 32) * sizeof(float2);
    static PerDevice per_device; // the > 64 KiB LDS opt-in is per device
    bool             first = false;
    int              dev = -1;
    const int        n_cu_ = per_device.current(&first, &dev);
    GR4_REQUIRE(n_cu_ != 0, "pfb: cannot query the current device");
    if (first) {
        GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pfb_run_kernel<LOG2N, PT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        per_device.done(dev, -n_cu_);
    }
    *taken = false;
    const long grid = (n_frames + L - 1) / L;
    if (L <= 0 || grid > 0x7fffffffL) return GR4HIP_OK;
    hipLaunchKernelGGL((pfb_run_kernel<LOG2N, PT>), dim3((unsigned)grid), dim3(512), lds, st, x, hist, taps, L, d_tw, o, n_frames);
    GR4_LAUNCH_CHECK();
    *taken = true;
    return GR4HIP_OK;
}
// compiled with the 8192-point kernels (fft_fast_pk.hip); P outside 2 .. 4: not taken
int pfb_run_launch_8192(int P, const float* x, const float* hist, const float* taps, long L, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st, bool* taken);

// N = 256 .. 8192: fft_fast_kernel's plans, workgroups, LDS layout and register epilogue behind the polyphase front end
template <int LOG2N>
__global__ __launch_bounds__(512, 4) void pfb_fast_kernel(PfbFront front, const float2* __restrict__ tw, FftOutputs out, long n_frames) {
    using FRONT = PfbFront;
    constexpr bool REAL = false;
    const float *  in = nullptr, *window = nullptr; // the FFT block's own load and window: not used behind a front end
#include "fft_fast_frames.inc"
}

template <int LOG2N>
static int pfb_fast_launch(const PfbFront& front, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) {
    constexpr int    N = 1 << LOG2N, FPB = 512 / (N / 16);
    constexpr size_t lds = (size_t)FPB * (N + N / 32) * sizeof(float2);
    static PerDevice per_device; // the > 64 KiB LDS opt-in is per device
    bool             first = false;
    int              dev = -1;
    const int        n_cu = per_device.current(&first, &dev);
    GR4_REQUIRE(n_cu != 0, "pfb: cannot query the current device");
    if (first) {
        GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pfb_fast_kernel<LOG2N>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        per_device.done(dev, -n_cu);
    }
    const long groups = (n_frames + FPB - 1) / FPB; // one workgroup per group of frame slots, like fft_fast_launch
    const long grid   = groups < 0x7fffffffL ? groups : 0x7fffffffL;
    hipLaunchKernelGGL(pfb_fast_kernel<LOG2N>, dim3((unsigned)grid), dim3(512), lds, st, front, d_tw, o, n_frames);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

// the two sizes compiled with the SLP vectoriser on, like the FFT block's (fft_fast_pk.hip)
int pfb_fast_launch_256(const PfbFront& front, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st);
int pfb_fast_launch_8192(const PfbFront& front, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st);

} // namespace gr4
