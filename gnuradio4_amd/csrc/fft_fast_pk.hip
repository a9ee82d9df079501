// fft_fast_pk.hip -- the fft_fast_kernel instantiations that are FASTER with hipcc's SLP vectoriser (packed f32 math): N = 256 and 8192.
// build.sh compiles this file without -fno-slp-vectorize; see fft_kernels.hpp.
// (round 5) streaming (nt) hints on the frames' loads and the results' stores, like fft.hip (profiles/r05_streaming_hints.txt: N = 256 |X|^2 442 - 456 -> 472 - 481 Gsamples/s)
#ifndef GR4_BUF_STORE_AUX
#define GR4_BUF_STORE_AUX 2
#endif
#ifndef GR4_BUF_LOAD_AUX
#define GR4_BUF_LOAD_AUX 2
#endif
#include "specint_kernels.hpp"
#include "ifft_kernels.hpp"
#include "stft_kernels.hpp"

namespace gr4 {
int fft_fast_launch_256(const float* d_in, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) {
    return fft_fast_launch<8>(d_in, d_window, d_tw, o, n_frames, st);
}
int fft_fast_launch_8192(const float* d_in, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) {
    return fft_fast_launch<13>(d_in, d_window, d_tw, o, n_frames, st);
}
// the polyphase filter bank's kernels of the same two sizes: the same passes, so the same split (PFB.md)
int pfb_fast_launch_256(const PfbFront& front, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) { return pfb_fast_launch<8>(front, d_tw, o, n_frames, st); }
int pfb_fast_launch_8192(const PfbFront& front, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) { return pfb_fast_launch<13>(front, d_tw, o, n_frames, st); }
int pfb_run_launch_8192(int P, const float* x, const float* hist, const float* taps, long L, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st, bool* taken) {
    switch (P) {
    case 2: return pfb_run_launch<13, 2>(x, hist, taps, L, d_tw, o, n_frames, st, taken);
    case 3: return pfb_run_launch<13, 3>(x, hist, taps, L, d_tw, o, n_frames, st, taken);
    case 4: return pfb_run_launch<13, 4>(x, hist, taps, L, d_tw, o, n_frames, st, taken);
    default: *taken = false; return GR4HIP_OK;
    }
}
// the overlapped-frame kernels of the same two sizes (OVERLAPPED_FFT.md): the same passes behind the hop front end
int hop_fast_launch_256(const HopFront& front, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) { return hop_fast_launch<8>(front, d_window, d_tw, o, n_frames, st); }
int hop_fast_launch_8192(const HopFront& front, const float* d_window, const float2* d_tw, const FftOutputs& o, long n_frames, hipStream_t st) { return hop_fast_launch<13>(front, d_window, d_tw, o, n_frames, st); }
// the spectrum integrator's sinks of the same two sizes (SPECTRUM_INTEGRATOR.md): their values have to equal these kernels' bit for bit.  8192 points: the 16
// accumulators do not fit beside the transform's 116 registers, so that size has 256 registers per lane and one workgroup per CU
int fft_sink_launch_256(const float* x, const float* window, const float2* tw, const SpecintLaunch& L, hipStream_t st) { return fft_sink_launch<8, 2>(x, window, tw, L, st); }
int fft_sink_launch_8192(const float* x, const float* window, const float2* tw, const SpecintLaunch& L, hipStream_t st) { return fft_sink_launch<13, 2>(x, window, tw, L, st); }
int pfb_sink_launch_256(const PfbFront& bank, const float2* tw, const SpecintLaunch& L, hipStream_t st) { return pfb_sink_launch<8, 2>(bank, tw, L, st); }
int pfb_sink_launch_8192(const PfbFront& bank, const float2* tw, const SpecintLaunch& L, hipStream_t st) { return pfb_sink_launch<13, 2>(bank, tw, L, st); }
// the inverse transform's kernels of the same two sizes (INVERSE_FFT.md): the forward kernels' statements, so the forward kernels' values
int ifft_fast_launch_256(bool c2r, const float* d_in, float* d_out, const float* d_window, float scale, const float2* d_tw, long n_frames, hipStream_t st) {
    return ifft_fast_launch<8>(c2r, d_in, d_out, d_window, scale, d_tw, n_frames, st);
}
int ifft_fast_launch_8192(bool c2r, const float* d_in, float* d_out, const float* d_window, float scale, const float2* d_tw, long n_frames, hipStream_t st) {
    return ifft_fast_launch<13>(c2r, d_in, d_out, d_window, scale, d_tw, n_frames, st);
}
} // namespace gr4
