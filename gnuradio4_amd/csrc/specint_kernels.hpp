// specint_kernels.hpp -- the spectrum integrator (SPECTRUM_INTEGRATOR.md) as seen by the transforms: its handle, the begin / finish steps of a call, and the
// kernels that run the FFT block's frame loop (fft_fast_frames.inc) with the |X|^2 store replaced by per-lane leaf sums (the fused sink).  The scheme itself
// -- leaves of 32 frames in float32, folded in float64 -- is leaf_integrator.hpp's: every producer (the stand-alone leaf kernel, the sinks, the beamformer)
// writes the float32 sum of call-leaf k to leaves[k][n_bins], the emit kernel folds them.
#pragma once
#include "leaf_integrator.hpp"
#include "pfb_kernels.hpp"

namespace gr4 {

constexpr int kSpecintLeaf = 32;
using SpecintGeom          = LeafGeom<kSpecintLeaf>;

// what a producer of leaf sums is given for one call
struct SpecintLaunch {
    SpecintGeom  geom;
    const float* carry;  // [n_bins]: the running leaf the call's first leaf starts from (zeros at a leaf's start)
    float*       leaves; // [geom.nl][n_bins]
};

#ifdef __HIPCC__
// ---- the fused sink.  A workgroup's unit is FPB call-leaves, one per frame slot: step j of the frame loop transforms frame j of every slot's leaf (the slots'
// frames are a leaf apart, not neighbours), and the lane adds its 16 values of |X|^2 to 16 float accumulators -- one leaf summed in order in registers, no
// cross-lane traffic.  Frames past a leaf's end or outside the call are read as 0 (an offset beyond the descriptor's range): their |X|^2 is +0, and adding +0 to
// a sum that started from +0 changes nothing.  A unit's frames are consecutive in the call (at most 32 FPB of them), so one descriptor covers them.
struct SinkLane {
    int first; // the slot's first frame, counted from the unit's
    int count; // frames of the slot's leaf in this call; 0: no such leaf
};

template <int N>
__device__ __forceinline__ int sink_bin(int t, int j) { // the bin of X[j] / m[j] in fft_fast_frames.inc
    return N == 8192 ? (t >> 1) + 4096 * (t & 1) + j * 256 : t + j * (N / 16);
}

template <int N>
__device__ __forceinline__ SinkLane sink_begin(const SpecintGeom& g, const float* __restrict__ carry, float (&acc)[16], long* unit_first, unsigned* unit_frames) {
    constexpr int T = N / 16, FPB = 512 / T;
    const long    ku = (long)blockIdx.x * FPB; // < nl: the grid is ceil(nl / FPB)
    long          f;
    int           c;
    bool          done;
    leaf_range(g, ku, unit_first, &c, &done);
    const long room = g.n - *unit_first;
    *unit_frames    = (unsigned)(room < FPB * kSpecintLeaf ? room : FPB * kSpecintLeaf);
    const int  fl = threadIdx.x / T, t = threadIdx.x % T;
    const long k  = ku + fl;
    SinkLane   ln{0, 0};
    if (k < g.nl) {
        leaf_range(g, k, &f, &c, &done);
        ln.first = (int)(f - *unit_first);
        ln.count = c;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = k == 0 ? carry[sink_bin<N>(t, j)] : 0.f;
    return ln;
}

template <int N>
__device__ __forceinline__ void sink_end(const SinkLane& ln, float* __restrict__ leaves, const float (&acc)[16]) {
    constexpr int T = N / 16, FPB = 512 / T;
    if (ln.count == 0) return;
    const int fl = threadIdx.x / T, t = threadIdx.x % T;
    float*    row = leaves + ((long)blockIdx.x * FPB + fl) * N;
#pragma unroll
    for (int j = 0; j < 16; ++j) row[sink_bin<N>(t, j)] = acc[j];
}

// steps of the frame loop a unit needs: no leaf is longer than min(A, 32)
__device__ __forceinline__ int sink_steps(const SpecintGeom& g) { return g.A < kSpecintLeaf ? (int)g.A : kSpecintLeaf; }

constexpr int kSinkOut = 0x40000000; // a lane offset beyond every range here

// the FFT block's load (frame x window: the window is applied by fft_fast_frames.inc, as in fft_fast_kernel) for the frame of the slot's leaf
struct FftLeafFront {
    static constexpr bool kFrontEnd = true, kSink = true;
    const float* x; // the unit's first frame
    unsigned     bytes;
    SinkLane     ln;
    int          steps;
    float*       acc;

    static __device__ __forceinline__ long first_group() { return (long)blockIdx.x * kSpecintLeaf; }
    __device__ __forceinline__ long        end_group(long) const { return first_group() + steps; }
    static __device__ __forceinline__ long group_stride() { return 1; }
    template <int FPB> static __device__ __forceinline__ long group(long g, long) { return g; }

    template <int N>
    __device__ __forceinline__ void load(float2 (&v)[16], long f0, unsigned, int, int t) const {
        constexpr int T = N / 16, FPB = 512 / T;
        const int     j   = (int)(f0 / FPB - first_group());
        const int     off = j < ln.count ? ((ln.first + j) * N + t) * 8 : kSinkOut;
        const rsrc_t  rx  = make_rsrc(x, bytes);
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = buf_load_f2(rx, off, r * T * 8);
    }
    __device__ __forceinline__ void sink(const float (&m)[16]) const {
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = acc[j] + m[j];
    }
};

// the bank's load (PfbFront's sums, term for term) for the frame of the slot's leaf
struct PfbLeafFront : PfbFront {
    static constexpr bool kSink = true;
    long     unit_first;
    unsigned unit_frames;
    SinkLane ln;
    int      steps;
    float*   acc;

    static __device__ __forceinline__ long first_group() { return (long)blockIdx.x * kSpecintLeaf; }
    __device__ __forceinline__ long        end_group(long) const { return first_group() + steps; }
    static __device__ __forceinline__ long group_stride() { return 1; }
    template <int FPB> static __device__ __forceinline__ long group(long g, long) { return g; }

    template <int N>
    __device__ __forceinline__ void load(float2 (&v)[16], long f0, unsigned, int, int t) const {
        constexpr int T = N / 16, FPB = 512 / T;
        constexpr int kOff = 0x20000000 / (N * 8); // a frame whose offsets lie beyond every range here (the largest: 32 FPB + 31 frames, 4 MiB) and stay below 2^31
        const int     j  = (int)(f0 / FPB - first_group());
        const bool    on = j < ln.count;
        const rsrc_t  rh = make_rsrc(taps, (unsigned)P * N * 4u);
        const long    fb = unit_first - (P - 1); // the first input frame this unit needs
        if (fb >= 0) {
            const rsrc_t rx = make_rsrc(x + fb * N * 2, (unit_frames + (unsigned)P - 1u) * N * 8u);
            const int    f  = on ? ln.first + j : kOff;
            part<N, 0, 8, false>(v, rx, rx, rh, f, t);
            part<N, 8, 8, false>(v, rx, rx, rh, f, t);
        } else { // the first unit of a call: input frame f < 0 is history frame P - 1 + f
            const rsrc_t rx = make_rsrc(x, (unsigned)(unit_first + unit_frames) * N * 8u);
            const rsrc_t rp = make_rsrc(hist, ((unsigned)P - 1u) * N * 8u);
            const int    f  = on ? (int)fb + ln.first + j : kOff;
            part<N, 0, 4, true>(v, rx, rp, rh, f, t);
            part<N, 4, 4, true>(v, rx, rp, rh, f, t);
            part<N, 8, 4, true>(v, rx, rp, rh, f, t);
            part<N, 12, 4, true>(v, rx, rp, rh, f, t);
        }
    }
    __device__ __forceinline__ void sink(const float (&m)[16]) const {
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = acc[j] + m[j];
    }
};

// WPE = waves per SIMD the register budget is set for: 4 = fft_fast_kernel's (128 registers, two workgroups per CU), 2 = 256 registers, one workgroup per CU
template <int LOG2N, int WPE>
__global__ __launch_bounds__(512, WPE) void fft_sink_kernel(const float* __restrict__ x, const float* __restrict__ window, const float2* __restrict__ tw, SpecintGeom geom,
                                                            const float* __restrict__ carry, float* __restrict__ leaves, FftOutputs out) {
    float          acc[16];
    long           unit_first;
    unsigned       unit_frames;
    const SinkLane ln = sink_begin<(1 << LOG2N)>(geom, carry, acc, &unit_first, &unit_frames);
    using FRONT = FftLeafFront;
    const FRONT    front{x + unit_first * (2L << LOG2N), unit_frames * (8u << LOG2N), ln, sink_steps(geom), acc};
    constexpr bool REAL = false;
    const float*   in       = nullptr; // the FFT block's own load: not used behind a front end
    const long     n_frames = geom.n;
#include "fft_fast_frames.inc"
    sink_end<(1 << LOG2N)>(ln, leaves, acc);
}

template <int LOG2N, int WPE>
__global__ __launch_bounds__(512, WPE) void pfb_sink_kernel(PfbFront bank, const float2* __restrict__ tw, SpecintGeom geom, const float* __restrict__ carry,
                                                            float* __restrict__ leaves, FftOutputs out) {
    float          acc[16];
    long           unit_first;
    unsigned       unit_frames;
    const SinkLane ln = sink_begin<(1 << LOG2N)>(geom, carry, acc, &unit_first, &unit_frames);
    using FRONT = PfbLeafFront;
    const FRONT    front{bank, unit_first, unit_frames, ln, sink_steps(geom), acc};
    constexpr bool REAL = false;
    const float *  in = nullptr, *window = nullptr;
    const long     n_frames = geom.n;
#include "fft_fast_frames.inc"
    sink_end<(1 << LOG2N)>(ln, leaves, acc);
}

// one workgroup per unit of FPB leaves
template <typename K, typename... Args>
static int sink_launch(K kernel, int log2n, const SpecintGeom& g, hipStream_t st, PerDevice& per_device, Args... args) {
    const int    N = 1 << log2n, FPB = 512 / (N / 16);
    const size_t lds = (size_t)FPB * (N + N / 32) * sizeof(float2);
    bool         first = false;
    int          dev = -1;
    const int    n_cu = per_device.current(&first, &dev);
    GR4_REQUIRE(n_cu != 0, "spectrum integrator: cannot query the current device");
    if (first) {
        GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        per_device.done(dev, -n_cu);
    }
    const long units = (g.nl + FPB - 1) / FPB;
    GR4_REQUIRE(units <= 0x7fffffffL, "spectrum integrator: %ld leaves in one call", g.nl);
    hipLaunchKernelGGL(kernel, dim3((unsigned)units), dim3(512), lds, st, args...);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

template <int LOG2N, int WPE>
static int fft_sink_launch(const float* x, const float* window, const float2* tw, const SpecintLaunch& L, hipStream_t st) {
    static PerDevice per_device;
    FftOutputs       o{};
    o.mag2 = L.leaves; // (marks |X|^2 as the requested output; the sink takes the values)
    return sink_launch(fft_sink_kernel<LOG2N, WPE>, LOG2N, L.geom, st, per_device, x, window, tw, L.geom, L.carry, L.leaves, o);
}
template <int LOG2N, int WPE>
static int pfb_sink_launch(const PfbFront& bank, const float2* tw, const SpecintLaunch& L, hipStream_t st) {
    static PerDevice per_device;
    FftOutputs       o{};
    o.mag2 = L.leaves;
    return sink_launch(pfb_sink_kernel<LOG2N, WPE>, LOG2N, L.geom, st, per_device, bank, tw, L.geom, L.carry, L.leaves, o);
}
// the two sizes compiled with the SLP vectoriser on, like the kernels they have to equal (fft_fast_pk.hip)
int fft_sink_launch_256(const float* x, const float* window, const float2* tw, const SpecintLaunch& L, hipStream_t st);
int fft_sink_launch_8192(const float* x, const float* window, const float2* tw, const SpecintLaunch& L, hipStream_t st);
int pfb_sink_launch_256(const PfbFront& bank, const float2* tw, const SpecintLaunch& L, hipStream_t st);
int pfb_sink_launch_8192(const PfbFront& bank, const float2* tw, const SpecintLaunch& L, hipStream_t st);
#endif // __HIPCC__

} // namespace gr4

struct gr4hip_specint {
    gr4::LeafIntegrator<gr4::kSpecintLeaf, false> integ;  // M = n_bins; begin / finish through specint_begin / specint_finish: one instance of the emit kernel
    gr4::DeviceBuffer                             d_mag2; // the composition's |X|^2 of one piece
    int                                           last_path  = 0;
    int                                           force_path = 0; // test hook: 1 = the sink wherever a kernel exists, 2 = the composition, 0 = the measured default
};

namespace gr4 {

// ---- the handle's side of a call (spectrum_integrator.hip), for the entries that live with their transform's handle (fft.hip, pfb.hip, beamformer.hip)
// argument checks shared by the three entries, before any device work: *n_out = spectra the call completes
int specint_check(const gr4hip_specint* si, const char* who, size_t n_bins, const void* d_in, size_t in_frame_bytes, size_t in_align, size_t n_frames, const float* d_out, size_t* n_out);
int specint_begin(gr4hip_specint* si, size_t n_frames, hipStream_t st, SpecintLaunch* L); // applies a pending reset, sizes the leaf scratch
int specint_finish(gr4hip_specint* si, const SpecintLaunch& L, float* d_out, int path, hipStream_t st); // the emit kernel; advances the position
bool specint_takes_sink(const gr4hip_specint* si, size_t n_bins, size_t bank_taps /* 0: the FFT block */); // whether a fused entry of this shape runs its sink kernel
int  specint_sink_fft(size_t N, const float* x, const float* window, const float2* tw, const SpecintLaunch& L, hipStream_t st);
int  specint_sink_pfb(size_t N, const PfbFront& bank, const float2* tw, const SpecintLaunch& L, hipStream_t st);
// the composition: `produce(first_frame, n, d_mag2)` writes the |X|^2 of n frames; they are integrated in pieces through the handle's bounded scratch
int specint_compose(gr4hip_specint* si, size_t n_frames, float* d_out, hipStream_t st, int (*produce)(void* ctx, size_t first, size_t n, float* d_mag2, hipStream_t st), void* ctx);

} // namespace gr4
