// fir.hip -- time-domain FIR / polyphase decimating FIR / Decimator kernels for gfx950.
//
// Replaces gr::filter::fir_filter<T>::processOne (blocks/filter/.../time_domain_filter.hpp:44-47; per-sample
// HistoryBuffer::push_front + K-term transform_reduce driven by Block.hpp:1723-1761) and the decimating
// BasicFilterProto::processBulk (:190-204) by one launch per work() span:
//   * the input span (+ the K-1 history samples carried in HBM between launches) is staged once into LDS,
//     de-interleaved by polyphase branch when decim > 1, so every input sample is read from HBM exactly once;
//   * each lane owns 8 consecutive output floats and slides a 12-float register window over its LDS row:
//     one ds_read_b128 of samples + one broadcast ds_read of taps feeds 32 (real) / 16 (complex) FMAs;
//   * complex<float> data x real taps is the same kernel on the interleaved float view with a tap stride of 2.
// Bound: FP32 FMA rate (2K flop per real output sample), not HBM -- see DESIGN.md "fir_poly".
// Long spans leave this kernel: float 33..256 taps and polyphase decimators go to the MFMA kernels of fir_batched.hip, complex <= 256 taps
// to the frequency-domain kernel of chain_fused.hip (gr4hip_fir_process below decides).
#include "common.hpp"
#include "history.hpp"
#include "fir_exact.hpp"
#include "ewise.hpp"
#include "fir_window.hpp"
#include "fir_f16_common.hpp" // (hf_wave_sum)

namespace gr4 {

// x: n_in samples; hist: the last `hcap` input samples before x (oldest first); tp: [D][Qpad] phase-major taps
// (tp[p][q] = b[q*D + p], zero padded); y: n_out samples, y[m] = sum_k b[k] x[m*D - k].
// HOOK: the filter's per-sample neighbours ride in this launch (ewise.hpp).  `pre` is applied to every sample of x on its way into LDS (pre.pos = absolute
// stream index of x[0]); the carried history holds what the prologue made of earlier samples and is taken as it lies (the next history this launch writes is
// made of prologue OUTPUTS too) -- exactly the filter's memory when the blocks run one after the other; `post` is applied to every output sample before its
// store (post.pos = absolute index of y[0]).
// gthr > 0: the workgroup judges its own outputs like the matrix-pipe kernels do (fir_f16.hip): output power (of its quietest wave) below gthr x the power of the samples it
// was given = the filter removes nearly everything, where ANY float32 sum -- this one phase by phase, the reference's tap by tap -- shows its rounding against the output
// (measured, complex decimate-by-2, tone near fs / 2: 12 x the reference order's error).  Such a workgroup evaluates its outputs again from the samples it has staged, with
// float64 products and sums (one rounding at the end): no second launch, hooks included (the staged samples are the prologue's outputs).  Non-finite power either side
// compares false: those outputs keep the float32 sums and with them the reference's classes.
template <int S, int BS, bool HOOK>
__global__ __launch_bounds__(BS) void fir_poly_kernel(const float* __restrict__ x, const float* __restrict__ hist, const float* __restrict__ tp,
                                                       float* __restrict__ y, long n_in, long n_out, int hcap, int D, int G, float* __restrict__ new_hist,
                                                       EwiseHook pre, EwiseHook post, float gthr) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float judge_red[2 * (BS / 64)];
    constexpr int R  = kFirR;
    constexpr int E  = 4 / S;
    const int     Lf = BS * R + 4 * G; // floats per phase row
    const int     Qp = G * E;          // padded taps per phase
    float*        xl = smem;           // [D][Lf]
    float*        bl = smem + (size_t)D * Lf; // [D][Qp]
    const int     tid   = threadIdx.x;
    const long    M0    = (long)blockIdx.x * (BS * R / S); // first output sample of this block
    const long    jbase = M0 - (4 * G) / S;                // first phase-stream sample held in LDS
    const int     Ls    = Lf / S;                          // samples per phase row

    for (int i = tid; i < D * Qp; i += BS) bl[i] = tp[i];

    // ---- stage inputs: u enumerates input samples i = i_lo + u; sample i belongs to phase p = (-i) mod D at j = ceil(i/D)
    const long i_lo  = jbase * D - (D - 1);
    const long total = (long)Ls * D;
    if (D == 1 && S == 1) {
        for (long u4 = (long)tid * 4; u4 < total; u4 += (long)BS * 4) { // i_lo is a multiple of 4 here
            const long i = i_lo + u4;
            float4     v;
            if (i >= 0 && i + 3 < n_in) {
                v = *reinterpret_cast<const float4*>(x + i);
                if constexpr (HOOK) {
                    float e[4] = {v.x, v.y, v.z, v.w};
                    ewise_hook<float, 4>(e, pre, i);
                    v = make_float4(e[0], e[1], e[2], e[3]);
                }
            } else {
                float t[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const long ii = i + c;
                    t[c] = (ii >= 0) ? (ii < n_in ? x[ii] : 0.f) : (ii >= -(long)hcap ? hist[hcap + ii] : 0.f);
                    if constexpr (HOOK)
                        if (ii >= 0 && ii < n_in) t[c] = ewise_hook1<float>(t[c], pre, ii);
                }
                v = make_float4(t[0], t[1], t[2], t[3]);
            }
            *reinterpret_cast<float4*>(xl + u4) = v;
        }
    } else if (D == 1 && S == 2) {
        for (long u2 = (long)tid * 2; u2 < total; u2 += (long)BS * 2) { // two complex samples = one float4
            const long i = i_lo + u2;
            float4     v;
            if (i >= 0 && i + 1 < n_in) {
                v = *reinterpret_cast<const float4*>(x + 2 * i);
                if constexpr (HOOK) {
                    float2 e[2] = {make_float2(v.x, v.y), make_float2(v.z, v.w)};
                    ewise_hook<float2, 2>(e, pre, i);
                    v = make_float4(e[0].x, e[0].y, e[1].x, e[1].y);
                }
            } else {
                float t[4];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const long   ii = i + c;
                    const float* p  = (ii >= 0) ? (ii < n_in ? x + 2 * ii : nullptr) : (ii >= -(long)hcap ? hist + 2 * (hcap + ii) : nullptr);
                    float2       q  = p ? make_float2(p[0], p[1]) : make_float2(0.f, 0.f);
                    if constexpr (HOOK)
                        if (p && ii >= 0) q = ewise_hook1<float2>(q, pre, ii);
                    t[2 * c]     = q.x;
                    t[2 * c + 1] = q.y;
                }
                v = make_float4(t[0], t[1], t[2], t[3]);
            }
            *reinterpret_cast<float4*>(xl + 2 * u2) = v;
        }
    } else {
        for (long u = tid; u < total; u += BS) {
            const long   i  = i_lo + u;
            const int    jl = (int)(u / D);
            const int    p  = D - 1 - (int)(u % D);
            const float* src = (i >= 0) ? (i < n_in ? x + S * i : nullptr) : (i >= -(long)hcap ? hist + S * (hcap + i) : nullptr);
            float*       dst = xl + (size_t)p * Lf + (size_t)jl * S;
            if constexpr (HOOK) {
                if (src && i >= 0) {
                    if constexpr (S == 1) dst[0] = ewise_hook1<float>(src[0], pre, i);
                    else { const float2 q = ewise_hook1<float2>(make_float2(src[0], src[1]), pre, i); dst[0] = q.x; dst[S - 1] = q.y; }
                    continue;
                }
            }
#pragma unroll
            for (int c = 0; c < S; ++c) dst[c] = src ? src[c] : 0.f;
        }
    }
    __syncthreads();

    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    const int c0 = tid * R + 4 * G; // local float index of this lane's first output sample's x[m*D] position
    for (int p = 0; p < D; ++p) {
        const float* row = xl + (size_t)p * Lf;
        const float* tg  = bl + (size_t)p * Qp;
        float        w[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(row + c0 - 4 + 4 * q);
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
        int g = 0;
        for (; g + 3 <= G; g += 3) { // window rotation sequence ROT = 0,2,1 (three steps return to ROT 0)
            fir_step<S, 0>(acc, w, tg + (g + 0) * E, row + c0 - 4 * (g + 0) - 8, (g + 1) < G);
            fir_step<S, 2>(acc, w, tg + (g + 1) * E, row + c0 - 4 * (g + 1) - 8, (g + 2) < G);
            fir_step<S, 1>(acc, w, tg + (g + 2) * E, row + c0 - 4 * (g + 2) - 8, (g + 3) < G);
        }
        if (g < G) {
            fir_step<S, 0>(acc, w, tg + g * E, row + c0 - 4 * g - 8, (g + 1) < G);
            if (g + 1 < G) fir_step<S, 2>(acc, w, tg + (g + 1) * E, row + c0 - 4 * (g + 1) - 8, false);
        }
    }

    if (gthr > 0.f) {
        float px = 0.f, py = 0.f;
        for (int p = 0; p < D; ++p) { // the samples this lane's outputs sit on: every staged sample of the workgroup's own span exactly once
            const float4 a = *reinterpret_cast<const float4*>(xl + (size_t)p * Lf + c0), b = *reinterpret_cast<const float4*>(xl + (size_t)p * Lf + c0 + 4);
            px += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w) + (b.x * b.x + b.y * b.y) + (b.z * b.z + b.w * b.w);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (M0 * S + (long)tid * R + r < n_out * S) py = fmaf(acc[r], acc[r], py); // (outputs past the span do not exist: the filter's transient into the zero-staged samples behind a truncated tone is not output power)
        px = hf_wave_sum(px);
        py = hf_wave_sum(py);
        if ((tid & 63) == 0) { judge_red[tid >> 6] = px; judge_red[BS / 64 + (tid >> 6)] = py; }
        __syncthreads();
        //  only waves whose 64 R outputs all exist vote: a wave past n_out sees zero-staged samples, its output power is 0 and the quietest-wave
        // statistic sent the last workgroup of EVERY call -- and every call shorter than 3/4 of a workgroup -- through the float64 loop.  A workgroup without one
        // complete wave (a span shorter than 64 R outputs) is judged on wave 0 alone, whose input sum counts the real samples only.
        px = 0.f;
        py = 3.4e38f;
        int  nc = 0;
        bool finite = true;
#pragma unroll
        for (int w = 0; w < BS / 64; ++w)
            if (M0 * S + (long)(w + 1) * 64 * R <= n_out * S) {
                ++nc;
                px += judge_red[w];
                py = fminf(py, judge_red[BS / 64 + w]); // (fminf drops a NaN: the test below sees it through px, or the wave's outputs are NaN anyway)
                finite = finite && judge_red[BS / 64 + w] < 3.0e38f;
            }
        if (nc == 0) { nc = 1; px = judge_red[0]; py = judge_red[BS / 64]; finite = py < 3.0e38f; }
        if (finite && py * (float)nc * (float)D < gthr * px) { // (uniform over the workgroup)
            double a64[R];
#pragma unroll
            for (int r = 0; r < R; ++r) a64[r] = 0.0;
            for (int p = 0; p < D; ++p) {
                const float* row = xl + (size_t)p * Lf + c0;
                const float* tg  = bl + (size_t)p * Qp;
                for (int q = 0; q < Qp; ++q) { // tap b[q D + p] meets the phase-p sample q places back
                    const double t = (double)tg[q];
#pragma unroll
                    for (int r = 0; r < R; ++r) a64[r] = __builtin_fma(t, (double)row[r - q * S], a64[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = (float)a64[r];
        }
    }
    const long of    = M0 * S + (long)tid * R; // first output float of this lane
    const long nf    = n_out * S;
    if constexpr (HOOK) {
        if (post.n_ops > 0) {
            if constexpr (S == 1) ewise_hook<float, R>(acc, post, of);
            else {
                float2 e[R / 2];
#pragma unroll
                for (int r = 0; r < R / 2; ++r) e[r] = make_float2(acc[2 * r], acc[2 * r + 1]);
                ewise_hook<float2, R / 2>(e, post, of / 2);
#pragma unroll
                for (int r = 0; r < R / 2; ++r) { acc[2 * r] = e[r].x; acc[2 * r + 1] = e[r].y; }
            }
        }
    }
    if (of + R <= nf) {
        *reinterpret_cast<float4*>(y + of)     = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(y + of + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (of + r < nf) y[of + r] = acc[r];
    }
    // a span served by this launch alone: workgroup 0 also writes the block's next history (the other half of the ping-pong pair; nobody reads it in this
    // launch), which saves the separate update launch -- a scheduler's 4 Ki .. 64 Ki-sample work() chunks cost launches, not arithmetic
    if (new_hist != nullptr && blockIdx.x == 0) {
        if constexpr (HOOK) { // the next history is made of what the prologue produces
            for (int h = tid; h < hcap; h += BS) {
                const long i = n_in - hcap + h;
                if constexpr (S == 1) new_hist[h] = i >= 0 ? ewise_hook1<float>(x[i], pre, i) : hist[hcap + i];
                else {
                    const float2 q = i >= 0 ? ewise_hook1<float2>(make_float2(x[2 * i], x[2 * i + 1]), pre, i) : make_float2(hist[2 * (hcap + i)], hist[2 * (hcap + i) + 1]);
                    new_hist[2 * h]     = q.x;
                    new_hist[2 * h + 1] = q.y;
                }
            }
        } else {
            for (int t = tid; t < hcap * S; t += BS) {
                const long h = t / S, c = t % S, i = n_in - hcap + h;
                new_hist[t]  = (i >= 0) ? x[i * S + c] : hist[(hcap + i) * S + c];
            }
        }
    }
}

// the shape no tiled kernel takes (decimation x taps beyond every LDS tiling, e.g. complex data decimated by 100): one output per lane, the reference's sum term for term
// (time_domain_filter.hpp:44-47 -- taps ascending, float32 fma), samples through the caches.  Slow and always there.
template <int S>
__global__ __launch_bounds__(256) void fir_generic_kernel(const float* __restrict__ x, const float* __restrict__ hist, int hcap, const float* __restrict__ b, int ntaps, long D,
                                                          float* __restrict__ y, long n_out, long n_in) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= n_out) return;
    float acc[S];
#pragma unroll
    for (int c = 0; c < S; ++c) acc[c] = 0.f;
    for (int k = 0; k < ntaps; ++k) {
        const long   i = m * D - k;
        const float* p = i >= 0 ? (i < n_in ? x + i * S : nullptr) : (i >= -(long)hcap ? hist + ((long)hcap + i) * S : nullptr);
        if (p == nullptr) continue;
#pragma unroll
        for (int c = 0; c < S; ++c) acc[c] = fmaf(b[k], p[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < S; ++c) y[m * S + c] = acc[c];
}

// the stored history changes its meaning (a prologue gain moves into or out of the taps): every sample times `factor`
__global__ void fir_hist_scale_kernel(float* __restrict__ hist, int nfloats, float factor) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nfloats) hist[t] *= factor;
}

template <typename V>
__global__ void decimate_kernel(const V* __restrict__ in, V* __restrict__ out, long n_out, long decim) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < n_out; m += stride) out[m] = in[m * decim];
}

} // namespace gr4

namespace gr4 { // chain_fused.hip: fast-convolution path for long complex inputs
struct ChainFused;
int  chain_fused_create(ChainFused** out, const float* taps, size_t ntaps, size_t fft_size, int window, int algo);
int  chain_fused_fir(ChainFused* c, const float* d_in, const float* d_hist256, size_t n_frames, float* d_y, hipStream_t st);
void chain_fused_set_measure(ChainFused* c, bool on);
int  chain_fused_power_ratio(ChainFused* c, bool wait, bool fir_output, float* ratio, float* marked_fraction = nullptr, float* float64_fraction = nullptr);
void chain_fused_destroy(ChainFused* c);

// fir_decim_fd.hip: decimate-by-8 real FIR (<= 1024 taps) as overlap-save blocks in the frequency domain
struct FirDecimFd;
int  fir_decim_fd_supported(size_t ntaps, size_t decim);
int  fir_decim_fd_create(FirDecimFd** out, const float* taps, size_t ntaps);
void fir_decim_fd_destroy(FirDecimFd* c);
struct DecimFdIir { const float* tab; int nsec; const float* state_in; float* state_out; int warm_blocks; };
int  fir_decim_fd_run(FirDecimFd* c, const float* d_in, size_t n_in, const float* d_hist, int hcap, float* d_out, hipStream_t st, bool measure, const DecimFdIir* iir = nullptr);
int  fir_decim_fd_power_ratio(FirDecimFd* c, bool wait, float* ratio);

// fir_batched.hip: block-Toeplitz FIR on the f32 MFMA units (real, <= 256 taps)
void fir_mfma_make_afrag(const float* taps, size_t ntaps, size_t nch, int* Kp_out, int* KS_out, std::vector<float>* af_out);
int  fir_mfma_launch(int KS, const float* x, long in_stride, const float* hist, const float* afrag, float* y, long out_stride, long n, unsigned nch, hipStream_t st, float* new_hist);
int  fir_mfma_c32_launch(int KS, const float* x, long n, const float* hist, const float* afrag, float* y, hipStream_t st, float* new_hist);
void fir_decim_band_make_row(const float* taps, size_t ntaps, size_t D, int* Kp_out, std::vector<float>* row);
void fir_bf16_make_afrag(const float* taps, size_t ntaps, int* KS_out, std::vector<unsigned short>* af, size_t nch, int force_ks);
int  fir_bf16_launch(int KS, const float* x, long n, const float* hist, int Kh, const void* afrag, float* y, hipStream_t st, float* new_hist, long in_stride, long out_stride, unsigned nch, int delay, int accum);
bool fir_f16_make_afrag(const float* taps, size_t ntaps, int* KS_out, std::vector<unsigned short>* af, size_t nch, int force_ks); // fir_f16.hip
bool fir_decim_f16_make_table(const float* taps, size_t ntaps, size_t D, int* KQ_out, std::vector<unsigned short>* tab, bool cplx); // fir_decim_f16.hip
int  fir_decim_f16_launch(int D, int KQ, const float* x, long n_in, const float* hist, int Kh, const void* table, float* y, long n_out, hipStream_t st, float* new_hist, int guard, unsigned char* flags, int cplx,
                          const EwiseHook* pre, const EwiseHook* post);
int  fir_f16_c32_launch(int KS, const float* x, long n, const float* hist, int Kh, const void* table, float* y, hipStream_t st, float* new_hist, int guard, unsigned char* flags, int delay = 0, int accum = 0, float gthr = 0.f);
int  fir_f16_launch(int KS, const float* x, long n, const float* hist, int Kh, const void* table, float* y, hipStream_t st, float* new_hist, long in_stride, long out_stride, unsigned nch, int delay, int accum, int guard,
                    unsigned char* flags, long flags_stride, float gthr);
int  fir_bf16_c32_launch(int KS, const float* x, long n, const float* hist, int Kh, const void* afrag, float* y, hipStream_t st, float* new_hist);
void fir_decim_bf16_make_afrag(const float* taps, size_t ntaps, size_t D, int* KS_out, int* Hb_out, std::vector<unsigned short>* af, bool cplx);
int  fir_decim_bf16_launch(int KS, int D, int Hb, const float* x, long n_in, const float* hist, int Kh, const void* afrag, float* y, long n_out, hipStream_t st, float* new_hist,
                           const EwiseHook* pre, const EwiseHook* post, bool cplx, unsigned char* flags, float gthr, int* seg_out);
int  fir_decim_band_launch(int D, int Kp, const float* x, const float* hist, int hcap, const float* row, float* y, long n_out, long n_in, hipStream_t st);
void fir_mfma_make_afrag_decim(const float* taps, size_t ntaps, size_t D, int* Kp_out, int* KS_out, std::vector<float>* af_out);
int  fir_mfma_decim_launch(int KS, int D, const float* x, const float* hist, const float* afrag, float* y, long n_out, hipStream_t st);

// out[h] = sample at stream position -len + h (h < len), from the hcap-sample history (zeros before it)
template <typename T>
__global__ void fir_hist_widen_kernel(const T* __restrict__ hist, int hcap, T* __restrict__ out, int len) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h < len) out[h] = h >= len - hcap ? hist[h - (len - hcap)] : T{};
}
} // namespace gr4

using namespace gr4;

constexpr size_t kFdFrame     = 8192;
// the per-segment guard of the split-product kernels (fir_f16.hip, fir_decim_f16.hip, fir_bf16.hip's decimators): a segment is marked for the second evaluation when its output
// power is below this x (sum b^2) x its input power -- 21 dB more rejected than white noise would lose.  Where it comes from: the two-term f16 products' error is ~1.3e-7 rms of
// the PRODUCTS' level sqrt(sum b^2) rms(x), its largest values ~4 x that; at an output 2^-3.5 = 1 / 11.3 of that level they reach 6e-6 of the output -- inside the 1e-5 bar with
// margin (measured with tools/tone_ratio.py: at the 36 dB threshold of round 4 unmarked segments reached 4.4e-5).  The tables of fir_f16.hip / fir_decim_f16.hip carry the same number.
constexpr double kGuardSegmentRatio = 1.0 / 128.0;
constexpr size_t kMfmaMinSamples = 1 << 16;
constexpr size_t kFdMinFrames = 64; // below this the direct-form kernel is as fast (the persistent FD grid wants >= 1 frame per CU)
constexpr size_t kDfHopS = 7168, kDfMinBlocks = 64; // the decimate-by-8 frequency-domain kernel (fir_decim_fd.hip): new samples per block, and the fewest blocks it takes

struct gr4hip_fir {
    int                dtype = GR4HIP_F32;
    int                S     = 1;
    size_t             ntaps = 0, decim = 1;
    size_t             hcap  = 32; // HistoryBuffer capacity (time_domain_filter.hpp:36: inputHistory{32})
    std::vector<float> taps;
    int                G = 0;      // tap groups per phase
    DeviceBuffer       d_taps;     // [D][Qpad]
    DeviceBuffer       d_tapsf;    // the taps as they are (what fir_exact_kernel multiplies with)
    double             tap_power = 0; // sum b^2 of `taps` (the guard's thresholds are multiples of it)
    double             guard_ratio = kGuardSegmentRatio; // (library-internal callers may tighten it: the chain's kernel pair squares this filter's output -- chain.hip)
    DeviceBuffer       d_flags_fd; // the same for the frequency-domain kernels' spans (judged behind their launch at their own thresholds)
    DeviceBuffer       d_flags;    // one byte per segment of the f16 matrix-pipe kernels' last launch: the segments fir_exact_kernel evaluates again behind it
    CarriedHistory     hist;       // hcap samples (S interleaved floats each)
    int                algo = GR4HIP_FIR_AUTO; // gr4hip_fir_set_algo
    bool               f32_user = false;       // (what gr4hip_fir_set_algo asked for: a reset re-arms the guard and goes back to it)
    bool               bf16_user = false;      // GR4HIP_FIR_TIME_DOMAIN_BF16X3: the three-term bf16 products where the default would take the two-term f16 ones
    bool               f32_products = false;   // GR4HIP_FIR_TIME_DOMAIN_F32, or a stream the dynamic-range guard has moved: no three-term bf16 products (the f32 matrix-pipe kernels instead)
    int                guard_mode = GR4HIP_GUARD_STRICT; // gr4hip_fir_set_guard_mode
    gr4::ChainFused*   fd  = nullptr; // complex, decim 1, ntaps <= 256: frequency-domain plan (created on first use)
    // dynamic-range guard of GR4HIP_FIR_AUTO (same policy as the chain's, include/gr4hip.h): the fast convolution's error floor is ~2e-6 of the INPUT rms;
    // below an output / input power ratio of 0.04 the direct form takes over (first use: probed synchronously; later: from finished measurements)
    bool               fd_probed = false, fd_blocked = false;
    float              fd_ratio  = -1.f;
    gr4::FirDecimFd*   dfd = nullptr; // float, decim 8, <= 1024 taps: frequency-domain decimator (created on first use)
    // tables built on first use, each with its host image (the stream rule, common.hpp: the copy on the call's stream may read it after the call returns)
    DeviceBuffer       d_band;        // float, decim >= 10: tap row of fir_decim_band_kernel
    std::vector<float> band_host;
    int                bandKp = 0;
    DeviceBuffer       d_bfrag;       // 33 .. 256 taps (float: also slices of 256 for 384 .. 1024): the three bf16 tap-fragment tables of fir_mfma_bf16x3_kernel
    std::vector<unsigned short> bfrag_host;
    int                bfKS = 0;
    DeviceBuffer       d_hfrag;       // 33 .. 256 taps and the 256-tap slices beyond (float: up to 3840, complex: up to 1792): the two-term f16 tables of fir_mfma_f16x2_kernel (fir_f16.hip)
    std::vector<unsigned short> hfrag_host;
    int                hfKS = 0;      // < 0: taps that form cannot carry
    DeviceBuffer       d_dhtab;       // decimate by 4 / 8 / 16 / 32, <= 1025 taps: the table of the f16 band-form decimators (fir_decim_f16.hip)
    std::vector<unsigned short> dhtab_host;
    int                dhKQ = 0;      // < 0: a shape that kernel does not carry
    std::vector<size_t> hf_off;       // per slice: offset into d_hfrag (in 16-bit units) ...
    std::vector<int>    hf_ks;        // ... and window size
    DeviceBuffer       d_bdfrag;      // float, decim 2 .. 12, complex, decim 3 .. 16, short branches: band-form bf16 fragments (fir_decim_bf16x3_kernel)
    std::vector<unsigned short> bdfrag_host;
    int                bdKS = 0, bdHb = 0; // bdKS < 0: the window does not fit that kernel
    std::vector<size_t> bf_off;       // per slice: offset into d_bfrag (in bf16 elements) ...
    std::vector<int>    bf_ks;        // ... and window size
    DeviceBuffer       d_hist256, d_histc;
    DeviceBuffer       d_afrag;       // 33 .. 256 taps without decimation, 16 .. 256 taps per phase with it: f32 MFMA A fragments
    std::vector<float> afrag_host;
    int                mKp = 0, mKS = 0;
    // per-sample neighbours executed in this filter's launch (gr4hip_fir_set_prologue / _epilogue): private copies of the programs
    gr4hip_ewise*      pre = nullptr, *post = nullptr;
    bool               pre_is_gain = false, post_is_gain = false; // nothing but real gains: folded into the taps (a FIR filter is linear)
    double             pre_gain = 1.0, post_gain = 1.0;
    double             folded = 1.0;   // the gain the device tap tables currently carry: `taps` = folded x `user_taps`
    std::vector<float> user_taps;      // the block's setting `b` as given
    long               pos = 0;        // input samples consumed since create / reset: the absolute index a rotator op's phase is a function of
    double             hist_gain = 1.0; // the stored history times this = what the prologue made of those samples (a folded prologue gain keeps RAW samples in the
                                        // history -- the taps carry the gain --, a hooked prologue keeps its outputs there: 1)
    DeviceBuffer       d_mid;          // gr4hip_fir_iir_process, two-launch path: the decimated stream between the filter and the cascade
    DeviceBuffer       d_pre;          // long spans of filters that take a matrix-pipe kernel: the prologue's output (one element-wise launch in front of it)
    // the stream rule (common.hpp): create / reset / set_taps / set_prologue only note what the device state has to become; fir_state_on() enqueues it on the stream of
    // the next call that needs it, behind whatever that stream still has in flight for this handle
    std::vector<float> tp_host;        // d_taps' image ([D][Qpad]) as fir_upload_taps laid it out
    bool               taps_dirty = false; // d_taps / d_tapsf do not hold tp_host / taps yet
    double             hist_rescale = 1.0; // the current history is to be multiplied by this (a prologue gain that moved into or out of the taps)
    unsigned           last_paths = 0;     // which paths served the last gr4hip_fir_process call (gr4hip_internal_fir_last_paths)
    ~gr4hip_fir() { delete pre; delete post; }
};

static int fir_upload_taps(gr4hip_fir* f) {
    const size_t D = f->decim, K = f->ntaps;
    const int    E = 4 / f->S;
    const size_t Q = ceil_div(K, D);
    f->G           = (int)ceil_div(Q, (size_t)E);
    const size_t Qp = (size_t)f->G * E;
    std::vector<float>& tp = f->tp_host;
    tp.assign(D * Qp, 0.f);
    for (size_t k = 0; k < K; ++k) tp[(k % D) * Qp + (k / D)] = f->taps[k];
    int rc = f->d_taps.ensure(tp.size() * sizeof(float)); // (growing frees the old table: hipFree waits for the device, nothing in flight loses its taps)
    if (rc) return rc;
    rc = f->d_tapsf.ensure(K * sizeof(float));
    if (rc) return rc;
    f->tap_power = 0;
    for (float b : f->taps) f->tap_power += (double)b * b;
    f->taps_dirty = true; // uploaded by fir_state_on, on the stream of the next call
    return GR4HIP_OK;
}

// The handle's device state as the call about to be enqueued on `st` must see it: pending tap upload, pending zeroing / rescaling of the carried history.
// Everything goes onto `st`, so it is ordered behind the earlier launches of this handle on that stream (Block.hpp:606, 916-917: reset() / settingsChanged() run
// between two work() calls of the block's own worker) and in front of the launch that follows.
static int fir_state_on(gr4hip_fir* f, hipStream_t st) {
    if (f->taps_dirty) {
        GR4_HIP_TRY(hipMemcpyAsync(f->d_taps.ptr, f->tp_host.data(), f->tp_host.size() * sizeof(float), hipMemcpyHostToDevice, st));
        GR4_HIP_TRY(hipMemcpyAsync(f->d_tapsf.ptr, f->taps.data(), f->ntaps * sizeof(float), hipMemcpyHostToDevice, st));
        f->taps_dirty = false;
    }
    if (f->hist.zero) f->hist_rescale = 1.0; // (a pending zeroing cancels a pending rescale)
    if (const int rc = f->hist.on(st)) return rc;
    if (f->hist_rescale != 1.0) {
        const int nf = (int)(f->hcap * f->S);
        hipLaunchKernelGGL(fir_hist_scale_kernel, dim3((unsigned)ceil_div(nf, 256)), dim3(256), 0, st, (float*)f->hist.current(), nf, (float)f->hist_rescale);
        GR4_LAUNCH_CHECK();
        f->hist_rescale = 1.0;
    }
    return GR4HIP_OK;
}
// a table built on first use: onto the call's stream, behind the launches that may still read the buffer's earlier contents.  The image is the handle's own.
template <class T>
static int fir_upload_table(DeviceBuffer& d, const std::vector<T>& image, hipStream_t st) {
    if (const int rc = d.ensure(image.size() * sizeof(T))) return rc;
    const hipError_t e = hipMemcpyAsync(d.ptr, image.data(), image.size() * sizeof(T), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { set_error("fir: upload failed: %s", hipGetErrorString(e)); return GR4HIP_RUNTIME_ERROR; }
    return GR4HIP_OK;
}

struct FirHooks { EwiseHook pre, post; bool any = false; };

template <int S, int BS, bool HOOK>
static int fir_launch_h(const gr4hip_fir* f, const float* x, const float* hist, float* y, long n_in, long n_out, size_t lds, hipStream_t st, float* new_hist, const FirHooks& hk) {
    auto kern = fir_poly_kernel<S, BS, HOOK>;
    if (lds > 48 * 1024) GR4_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long TOs  = BS * kFirR / S;
    const long grid = ceil_div(n_out, TOs);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BS), lds, st, x, hist, (const float*)f->d_taps.ptr, y, n_in, n_out,
                       (int)f->hcap, (int)f->decim, f->G, new_hist, hk.pre, hk.post, f->guard_mode != GR4HIP_GUARD_OFF && f->ntaps > 1 ? (float)(f->tap_power * f->guard_ratio) : 0.f);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}
template <int S, int BS>
static int fir_launch(const gr4hip_fir* f, const float* x, const float* hist, float* y, long n_in, long n_out, size_t lds, hipStream_t st, float* new_hist, const FirHooks& hk) {
    return hk.any ? fir_launch_h<S, BS, true>(f, x, hist, y, n_in, n_out, lds, st, new_hist, hk) : fir_launch_h<S, BS, false>(f, x, hist, y, n_in, n_out, lds, st, new_hist, hk);
}

// every device table derived from the taps is rebuilt on next use
static void fir_invalidate_tables(gr4hip_fir* f) {
    if (f->fd) { chain_fused_destroy(f->fd); f->fd = nullptr; }
    if (f->dfd) { fir_decim_fd_destroy(f->dfd); f->dfd = nullptr; }
    f->mKS = 0;
    f->bandKp = 0;
    f->bfKS = 0;
    f->hfKS = 0;
    f->dhKQ = 0;
    f->bdKS = 0;
}
// `taps` = gain x `user_taps` (float64 product, rounded once), uploaded
static int fir_apply_gain(gr4hip_fir* f, double gain) {
    f->taps.resize(f->user_taps.size());
    for (size_t k = 0; k < f->taps.size(); ++k) f->taps[k] = (float)(gain * (double)f->user_taps[k]);
    f->folded = gain;
    fir_invalidate_tables(f);
    return fir_upload_taps(f);
}
// the stored history follows a change of its meaning: hist_gain -> g (a prologue gain that moves into or out of the taps)
static int fir_rescale_history(gr4hip_fir* f, double g) {
    if (g == f->hist_gain) return GR4HIP_OK;
    if (f->pos > 0) f->hist_rescale *= f->hist_gain / g; // applied by fir_state_on on the next call's stream (in float64 until then: two changes in a row round once)
    f->hist_gain = g;
    return GR4HIP_OK;
}
// what this call does with the neighbours: gains ride in the taps, the rest are hooks (or, in front of / behind a matrix-pipe kernel, element-wise launches)
static int fir_prepare_hooks(gr4hip_fir* f, FirHooks* hk, hipStream_t st) {
    const bool   fold_pre = f->pre && f->pre_is_gain, fold_post = f->post && f->post_is_gain;
    const double want     = (fold_pre ? f->pre_gain : 1.0) * (fold_post ? f->post_gain : 1.0);
    if (want != f->folded) { if (const int rc = fir_apply_gain(f, want)) return rc; }
    if (f->pre && !fold_pre) {
        f->pre->pos = f->pos;
        if (const int rc = ewise_device_ops(f->pre, &hk->pre, st)) return rc;
    }
    if (f->post && !fold_post) {
        f->post->pos = f->pos / (long)f->decim;
        if (const int rc = ewise_device_ops(f->post, &hk->post, st)) return rc;
    }
    hk->any = hk->pre.n_ops > 0 || hk->post.n_ops > 0;
    return GR4HIP_OK;
}
static int fir_set_hook(gr4hip_fir* f, const gr4hip_ewise_t* prog, bool prologue) {
    GR4_REQUIRE(f, "fir_set_%s: null handle", prologue ? "prologue" : "epilogue");
    if (prog && prog->dtype != f->dtype) { set_error("fir_set_%s: the program's dtype %d is not the filter's (%d)", prologue ? "prologue" : "epilogue", prog->dtype, f->dtype); return GR4HIP_UNSUPPORTED; }
    gr4hip_ewise* copy = nullptr;
    if (prog && !prog->user.empty()) {
        copy = ewise_clone(prog);
        GR4_REQUIRE(copy, "out of host memory");
    }
    if (prologue) {
        // the history keeps what the OUTGOING prologue made of the samples in it (the filter's memory when the blocks run one after the other): with a hooked
        // prologue it holds those outputs already, with a folded gain it holds raw samples and is brought to the new prologue's convention here
        double     g       = 1.0;
        const bool is_gain = copy && ewise_as_real_gain(copy, &g);
        if (const int rc = fir_rescale_history(f, is_gain ? g : 1.0)) { delete copy; return rc; }
        delete f->pre;
        f->pre         = copy;
        f->pre_is_gain = is_gain;
        f->pre_gain    = is_gain ? g : 1.0;
    } else {
        delete f->post;
        f->post         = copy;
        f->post_is_gain = copy && ewise_as_real_gain(copy, &f->post_gain);
    }
    return GR4HIP_OK;
}

extern "C" {

int gr4hip_fir_create(gr4hip_fir_t** out, int dtype, const float* h_taps, size_t ntaps, size_t decim) {
    GR4_REQUIRE(out, "fir: null output handle");
    GR4_REQUIRE(dtype == GR4HIP_F32 || dtype == GR4HIP_C32, "fir: dtype must be F32 or C32 (got %d)", dtype);
    GR4_REQUIRE(h_taps && ntaps >= 1, "fir: need at least one tap");
    GR4_REQUIRE(decim >= 1, "fir: decim must be >= 1");
    auto* f = new (std::nothrow) gr4hip_fir();
    GR4_REQUIRE(f, "out of host memory");
    f->dtype = dtype;
    f->S     = dtype == GR4HIP_C32 ? 2 : 1;
    f->decim = decim;
    f->ntaps = ntaps;
    f->taps.assign(h_taps, h_taps + ntaps);
    f->user_taps = f->taps;
    if (ntaps > f->hcap) f->hcap = bit_ceil(ntaps); // time_domain_filter.hpp:38-42
    int rc = fir_upload_taps(f);
    if (!rc) rc = f->hist.resize(f->hcap * f->S * sizeof(float));
    if (rc) { delete f; return rc; }
    *out = f;
    return GR4HIP_OK;
}

int gr4hip_fir_set_taps(gr4hip_fir_t* f, const float* h_taps, size_t ntaps) {
    GR4_REQUIRE(f && h_taps && ntaps >= 1, "fir_set_taps: bad arguments");
    f->user_taps.assign(h_taps, h_taps + ntaps);
    f->ntaps = ntaps;
    f->fd_probed = f->fd_blocked = false;
    f->f32_products = f->f32_user;
    f->fd_ratio  = -1.f;
    int rc   = fir_apply_gain(f, f->folded); // every table derived from the taps is rebuilt on next use
    if (rc) return rc;
    if (ntaps > f->hcap) { // the reference replaces the HistoryBuffer (history is lost) only when it must grow
        f->hcap = bit_ceil(ntaps);
        return f->hist.resize(f->hcap * f->S * sizeof(float));
    }
    return GR4HIP_OK;
}

int gr4hip_fir_reset(gr4hip_fir_t* f) {
    GR4_REQUIRE(f, "fir_reset: null handle");
    f->fd_probed = f->fd_blocked = false;
    f->f32_products = f->f32_user;
    f->fd_ratio  = -1.f;
    f->pos = 0;
    f->hist.reset();
    return GR4HIP_OK;
}

int gr4hip_fir_set_prologue(gr4hip_fir_t* f, const gr4hip_ewise_t* prog) { return fir_set_hook(f, prog, true); }
int gr4hip_fir_set_epilogue(gr4hip_fir_t* f, const gr4hip_ewise_t* prog) { return fir_set_hook(f, prog, false); }

int gr4hip_fir_set_algo(gr4hip_fir_t* f, int algo) {
    GR4_REQUIRE(f, "fir_set_algo: null handle");
    GR4_REQUIRE(algo >= GR4HIP_FIR_AUTO && algo <= GR4HIP_FIR_TIME_DOMAIN_BF16X3, "fir_set_algo: unknown algo %d", algo);
    f->algo         = algo == GR4HIP_FIR_TIME_DOMAIN_F32 ? (int)GR4HIP_FIR_TIME_DOMAIN : (algo == GR4HIP_FIR_TIME_DOMAIN_BF16X3 ? (f->S == 2 ? (int)GR4HIP_FIR_TIME_DOMAIN : (int)GR4HIP_FIR_AUTO) : algo); // (float filters take their matrix-pipe kernels under AUTO)
    f->f32_products = f->f32_user = algo == GR4HIP_FIR_TIME_DOMAIN_F32;
    f->bf16_user    = algo == GR4HIP_FIR_TIME_DOMAIN_BF16X3;
    return GR4HIP_OK;
}
int gr4hip_fir_set_guard_mode(gr4hip_fir_t* f, int mode) {
    GR4_REQUIRE(f, "fir_set_guard_mode: null handle");
    GR4_REQUIRE(mode >= GR4HIP_GUARD_STRICT && mode <= GR4HIP_GUARD_OFF, "fir_set_guard_mode: unknown mode %d", mode);
    f->guard_mode = mode;
    if (f->fd) chain_fused_set_measure(f->fd, mode != GR4HIP_GUARD_OFF && f->ntaps > 1);
    return GR4HIP_OK;
}
} // extern "C"

// ------------------------------------------------------------------------------------------------ gr4hip_fir_process: which kernel takes a call

// Crossover thresholds of the dispatch: developer knobs read from the environment when the library is loaded (tools/decim_d4_rates.py, tools/cfir_bf16_threshold.py)
static size_t env_size(const char* name, size_t dflt) {
    const char* e = std::getenv(name);
    return e ? (size_t)std::atoi(e) : dflt;
}
// taps from which the f16 band-form decimator takes a call.  Measured (G input samples/s, bf16 band kernel / f16 one), float decimate by 8: 64 taps 1037 / 998,
// 100 taps 984 / 999, 128 taps 963 / 998
static const size_t kDecimF16MinTaps8  = env_size("GR4HIP_FIR_DECIM_F16_MIN_TAPS", 97);
static const size_t kDecimF16MinTapsW  = env_size("GR4HIP_FIR_DECIM_F16_MIN_TAPS_WIDE", 33); // (decimate by 16 / 32)
static const size_t kDecimF16MinTapsC8 = env_size("GR4HIP_FIR_DECIM_F16_MIN_TAPS_C8", 64);   // (complex, decimate by 8)
static const size_t kDecimF16MinTaps4  = env_size("GR4HIP_FIR_DECIM_F16_MIN_TAPS_D4", 33);   // (decimate by 4, float and complex)
// complex taps from which the three-term bf16 kernel takes over from the f32 MFMA.  65 puts 33 .. 64 taps back on the f32 MFMA (measured 5-8 % slower: 299-316
// against 322-333 Gsamples/s); below 33 taps the register-window kernel is ahead up to 27 taps and within 3 % from there (tools/cfir_bf16_threshold.py)
static const size_t kCBf16MinTaps = env_size("GR4HIP_CFIR_BF16_MIN_TAPS", 33);
static const size_t kBandMinDecim = env_size("GR4HIP_FIR_BAND_MIN_DECIM", 10); // where the band form takes over from the polyphase form

// the handle moves past a span of n_in input samples: its next history is the span's last hcap samples (unless the launch that took it has written them)
static int fir_advance(gr4hip_fir* f, const float* x, size_t n_in, hipStream_t st, bool hist_written) {
    if (hist_written) f->hist.flip();
    else if (const int rc = f->hist.advance(x, n_in * f->S, f->hcap * f->S, sizeof(float), st)) return rc; // (the S interleaved floats of a sample as one flat run of floats)
    f->pos += (long)n_in;
    return GR4HIP_OK;
}

// one gr4hip_fir_process call as the paths below see it
struct FirCall {
    gr4hip_fir*     f;
    const float*    x;
    float*          y;
    size_t          n_in, n_out;
    hipStream_t     st;
    const FirHooks& hk;
    bool            plain; // no hooks: the matrix-pipe and frequency-domain kernels are for plain filters
    int             algo;  // f->algo; GR4HIP_FIR_EXACT_F32 (= the register-window kernel only) for a hooked call
    const float*    hist;  // the hcap samples in front of x + done
    size_t          done = 0; // input samples already produced (only the fast convolution leaves a remainder)
    // a kernel that does not judge its own segments (f32 matrix-pipe and three-term bf16 direct forms, band, generic) notes where its part of the span starts and
    // which samples lie in front of it: the judge and the second evaluation follow it at the end of the call
    size_t          unj_from = SIZE_MAX;
    const float*    unj_hist = nullptr;
    bool            hist_written = false; // the launch that finished the span wrote the next history
    float* next_hist() const { return (float*)f->hist.next(); }
    int    took(bool wrote_hist) { done = n_in; hist_written = wrote_hist; return GR4HIP_OK; }
    int    took_unjudged(bool wrote_hist) { unj_from = done; unj_hist = hist; return took(wrote_hist); }
};

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the three-term bf16 kernels are off for this handle (GR4HIP_FIR_EXACT_F32: IEEE float32 multiply-add, the reference's Inf / NaN behaviour) or for the process (developer switch)
static bool no_bf16x3(const gr4hip_fir_t* f) { return f->algo == GR4HIP_FIR_EXACT_F32 || f->f32_products || dev_switch(kDevFirNoBf16x3); }
// May the two-term f16 kernels (fir_f16.hip) take the call?  The complex and the float form differ on purpose.
// complex: not EXACT_F32 (TIME_DOMAIN included) and f32_user, not f32_products: a stream moved by the guard stays on the self-judging f16 kernel
static bool fir_cf16_ok(const FirCall& c) {
    const gr4hip_fir* f = c.f;
    return c.plain && c.algo != GR4HIP_FIR_EXACT_F32 && !f->f32_user && !f->bf16_user && !dev_switch(kDevFirNoBf16x3) && !dev_switch(kDevFirNoF16x2) && f->hfKS >= 0;
}
// float: AUTO only (TIME_DOMAIN keeps the f32 matrix pipe); no guard moves a float filter without decimation, so f32_products is the user's choice here
static bool fir_rf16_ok(const FirCall& c) {
    const gr4hip_fir* f = c.f;
    return c.plain && c.algo == GR4HIP_FIR_AUTO && !no_bf16x3(f) && !f->bf16_user && !dev_switch(kDevFirNoF16x2) && f->hfKS >= 0;
}

// (first use) the two-term f16 tables (fir_f16_make_afrag) in slices of 256 taps, one after the other in d_hfrag.  hfKS < 0: taps that form cannot carry.
// pad9: a slice of 8 K-steps runs the 9-step kernel on zero-padded taps (the complex sliced kernel at 8 K-steps would keep two registers in scratch).
// thr_in_header: the last slice's header carries a tighter guard ratio of a library-internal caller -- a second verdict on the segment's WHOLE output power; the
// quietest-column statistic keeps its 21 dB (at 15 dB it dips below on narrow-band noise alone: 1 % pass band, half of all segments marked).
static int fir_f16_tables(gr4hip_fir* f, hipStream_t st, bool pad9, bool thr_in_header) {
    if (f->hfKS != 0) return GR4HIP_OK;
    const size_t                 nslice = ceil_div(f->ntaps, (size_t)256);
    std::vector<unsigned short>& all    = f->hfrag_host;
    all.clear();
    f->hf_off.assign(nslice, 0);
    f->hf_ks.assign(nslice, 0);
    for (size_t p = 0; p < nslice; ++p) {
        std::vector<unsigned short> af;
        const size_t                len = std::min<size_t>(256, f->ntaps - 256 * p);
        const int                   nat = std::max(3, (int)((len - 1 + 16 + 31) / 32));
        if (!fir_f16_make_afrag(f->taps.data() + 256 * p, len, &f->hf_ks[p], &af, 1, pad9 && nat == 8 ? 9 : 0)) { f->hfKS = -1; return GR4HIP_OK; }
        if (thr_in_header && p + 1 == nslice && f->guard_ratio != kGuardSegmentRatio) {
            const float g = (float)(f->tap_power * f->guard_ratio);
            std::memcpy(af.data() + (size_t)f->hf_ks[p] * 1536 + 6, &g, 4);
        }
        f->hf_off[p] = all.size();
        all.insert(all.end(), af.begin(), af.end());
    }
    if (const int rc = fir_upload_table(f->d_hfrag, all, st)) return rc;
    f->hfKS = f->hf_ks[0];
    return GR4HIP_OK;
}
// (first use) the three-term bf16 fragments (fir_bf16_make_afrag) in slices of 256 taps, one after the other in d_bfrag
static int fir_bf16_tables(gr4hip_fir* f, hipStream_t st) {
    if (f->bfKS != 0) return GR4HIP_OK;
    const size_t                 nslice = ceil_div(f->ntaps, (size_t)256);
    std::vector<unsigned short>& all    = f->bfrag_host;
    all.clear();
    f->bf_off.assign(nslice, 0);
    f->bf_ks.assign(nslice, 0);
    for (size_t p = 0; p < nslice; ++p) {
        std::vector<unsigned short> af;
        fir_bf16_make_afrag(f->taps.data() + 256 * p, std::min<size_t>(256, f->ntaps - 256 * p), &f->bf_ks[p], &af, 1, 0);
        f->bf_off[p] = all.size();
        all.insert(all.end(), af.begin(), af.end());
    }
    if (const int rc = fir_upload_table(f->d_bfrag, all, st)) return rc;
    f->bfKS = f->bf_ks[0];
    return GR4HIP_OK;
}
// (first use) the A fragments of the f32 MFMA kernels (fir_batched.hip): the block-Toeplitz form without decimation, the polyphase form with it
static int fir_mfma_table(gr4hip_fir* f, hipStream_t st) {
    if (f->mKS != 0) return GR4HIP_OK;
    if (f->decim == 1) fir_mfma_make_afrag(f->taps.data(), f->ntaps, 1, &f->mKp, &f->mKS, &f->afrag_host);
    else fir_mfma_make_afrag_decim(f->taps.data(), f->ntaps, f->decim, &f->mKp, &f->mKS, &f->afrag_host);
    const int rc = fir_upload_table(f->d_afrag, f->afrag_host, st);
    if (rc) f->mKS = 0;
    return rc;
}

// does the f16 band-form decimator (fir_decim_f16.hip: D = 4 / 8 / 16 / 32, two-term f16 products, carries the filter's programs) take this call?
static bool fir_decim_f16_shape(const gr4hip_fir_t* f, size_t n_in, const void* d_in, const void* d_out, bool hooked) {
    if (hooked && f->decim == 4 && (f->S == 2 ? 2 * f->ntaps - 1 : f->ntaps) > 577) return false; // (decimate by 4 with more than five K-steps per wave AND programs: 256 registers do not hold it without spills; the bf16 band kernel takes it)
    const size_t D = f->decim, K = f->ntaps;
    const bool   taps_ok = (f->S == 1 && ((D == 8 && K >= kDecimF16MinTaps8) || ((D == 16 || D == 32) && K >= kDecimF16MinTapsW) || (D == 4 && K >= kDecimF16MinTaps4))) ||
                           (f->S == 2 && (((D == 16 || D == 32) && K >= kDecimF16MinTapsW) || (D == 8 && K >= kDecimF16MinTapsC8) || (D == 4 && K >= kDecimF16MinTaps4)));
    return taps_ok && K <= 1025 && n_in * f->S >= (1u << 17) && al16(d_out) && al16(d_in) && f->algo == GR4HIP_FIR_AUTO && !f->f32_user && !f->bf16_user &&
           !dev_switch(kDevFirNoBf16x3) && !dev_switch(kDevFirNoF16x2) && !dev_switch(kDevFirNoDecimF16) && f->dhKQ >= 0;
}
// does the band-form bf16 decimator (fir_bf16.hip) take this call?  Builds its fragments on first use.
static bool fir_decim_bf16_ready(gr4hip_fir_t* f, size_t n_in, const void* d_in, const void* d_out, int* rc, hipStream_t st) {
    *rc = GR4HIP_OK;
    if (!(f->decim >= (f->S == 1 ? (size_t)2 : (size_t)3) && f->decim <= (f->S == 1 ? (size_t)12 : (size_t)16) && n_in / f->decim >= (1u << 14) && f->algo == GR4HIP_FIR_AUTO && f->bdKS >= 0 &&
          al16(d_out) && al16(d_in) && !no_bf16x3(f)))
        return false;
    if (f->bdKS == 0) {
        int ks = 0;
        fir_decim_bf16_make_afrag(f->taps.data(), f->ntaps, f->decim, &ks, &f->bdHb, &f->bdfrag_host, f->S == 2);
        if (ks == 0 || (f->S == 1 && f->decim == 8 && ks > 9 && f->ntaps <= 1024)) f->bdKS = -1; // the window does not fit -- or decimate-by-8 with a long window, where the
                                                                                                  // frequency-domain kernel is faster (762 against 305 G input samples/s at 1024 taps)
        else {
            if ((*rc = fir_upload_table(f->d_bdfrag, f->bdfrag_host, st))) return false;
            f->bdKS = ks;
        }
    }
    return f->bdKS > 0;
}
// the band form of the decimating contraction (fir_batched.hip: samples in stream order, the decimation in the A operand).  Declines when its tile does not fit the LDS.
static int fir_band(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (f->bandKp == 0) {
        fir_decim_band_make_row(f->taps.data(), f->ntaps, f->decim, &f->bandKp, &f->band_host);
        if (const int rc = fir_upload_table(f->d_band, f->band_host, c.st)) { f->bandKp = 0; return rc; }
    }
    const int rc = fir_decim_band_launch((int)f->decim, f->bandKp, c.x, c.hist, (int)f->hcap, (const float*)f->d_band.ptr, c.y, (long)c.n_out, (long)c.n_in, c.st);
    if (rc == GR4HIP_UNSUPPORTED) return GR4HIP_OK;
    return rc ? rc : c.took_unjudged(false);
}

// ---- the paths, in the order fir_process_core tries them.  Each returns GR4HIP_OK having taken the span (c.done == n_in) or, the fast convolution, its first part --
// or having declined (c.done as it was); anything else is an error.

// complex, no decimation, 33 .. 256 taps, long 16-byte-aligned span: the f16 direct form (path 2) takes it
static bool fir_cf16_shape(const FirCall& c) {
    const gr4hip_fir* f = c.f;
    return f->S == 2 && f->decim == 1 && f->ntaps > 32 && f->ntaps <= 256 && c.n_in - c.done >= kMfmaMinSamples / 2 && al16(c.x + c.done * 2) && al16(c.y + c.done * 2) && fir_cf16_ok(c);
}

// 1. complex, no decimation, 97 .. 256 taps, long input path 2 does not take (unaligned, developer switches, TIME_DOMAIN_BF16X3): whole 8192-sample frames through
// the fused FFT -> xH -> inverse kernel (chain_fused.hip: 2 transforms per frame instead of 1024 flop per sample); the direct form finishes the remainder.  (<= 96 taps
// the direct form is faster and has no dynamic-range floor: 300 .. 356 Gsamples/s up to 64 taps, 311 .. 275 at 65 .. 96 on the bf16 matrix pipe, against 248 at every
// tap count here, tools/cfir_taps_sweep.py.  Path 2 is as fast at 256 taps and faster below -- 129 / 192 / 256 taps 288 / 255 / 237 against 241 / 242 / 240 --, its
// error is relative to the output and the call stays asynchronous.)  Guard (the chain's policy, include/gr4hip.h): the error floor is ~2e-6 of the INPUT rms, so it
// shows below an output / input power ratio of 0.04.  Strict: every frame judged behind the launch, the marked ones evaluated again in float64 (fir_judge_kernel +
// fir_exact_kernel).  Deferred: a stream's first call probes eight frames synchronously.  An earlier launch's measurement, once it has arrived, moves a stream that
// rejects most of its input to the direct form for good.
static int fir_path_cfast(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(f->S == 2 && f->decim == 1 && f->ntaps > 96 && f->ntaps <= 256 && c.n_in >= kFdMinFrames * kFdFrame && c.algo == GR4HIP_FIR_AUTO && !f->fd_blocked &&
          !fir_cf16_shape(c)))
        return GR4HIP_OK;
    int rc = GR4HIP_OK;
    if (!f->fd) {
        rc = chain_fused_create(&f->fd, f->taps.data(), f->ntaps, kFdFrame, GR4HIP_WIN_NONE, GR4HIP_CHAIN_FUSED_FD);
        if (!rc && f->ntaps > 1 && f->guard_mode != GR4HIP_GUARD_OFF) chain_fused_set_measure(f->fd, true);
    }
    if (!rc) rc = f->d_hist256.ensure(256 * sizeof(float2));
    if (rc) return rc;
    const float* h256 = (const float*)f->d_hist256.ptr;
    hipLaunchKernelGGL(fir_hist_widen_kernel<float2>, dim3(1), dim3(256), 0, c.st, (const float2*)c.hist, (int)f->hcap, (float2*)f->d_hist256.ptr, 256);
    GR4_LAUNCH_CHECK();
    const size_t frames  = c.n_in / kFdFrame; // >= kFdMinFrames: more than a probe
    const bool   guarded = f->ntaps > 1 && f->guard_mode != GR4HIP_GUARD_OFF;
    const bool   strict  = guarded && f->guard_mode == GR4HIP_GUARD_STRICT;
    float        ratio;
    if (chain_fused_power_ratio(f->fd, false, true, &ratio)) f->fd_ratio = ratio; // a finished earlier launch: no waiting
    size_t probe = 0;
    if (guarded && !strict && !f->fd_probed) {
        probe = std::min<size_t>(frames, 8);
        if ((rc = chain_fused_fir(f->fd, c.x, h256, probe, c.y, c.st))) return rc;
        if (chain_fused_power_ratio(f->fd, true, true, &ratio)) f->fd_ratio = ratio;
    }
    if (guarded) f->fd_probed = true;
    if (guarded && f->fd_ratio >= 0.f && f->fd_ratio < 0.04f) {
        f->fd_blocked = f->f32_products = true; // the direct form takes the span, the probed frames too (float32 products from here on)
        return GR4HIP_OK;
    }
    const long nfd = (long)(frames * kFdFrame);
    rc = chain_fused_fir(f->fd, c.x + probe * kFdFrame * 2, probe ? c.x + (probe * kFdFrame - 256) * 2 : h256, frames - probe, c.y + probe * kFdFrame * 2, c.st);
    if (!rc && strict) {
        rc = f->d_flags_fd.ensure(frames);
        if (!rc) rc = fir_judge_launch(c.x, nfd, c.y, nfd, 1, 1, 13, 0.04f, (unsigned char*)f->d_flags_fd.ptr, c.st);
        if (!rc) rc = fir_exact_launch(c.x, nfd, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, 1, 1, c.y, nfd, (const unsigned char*)f->d_flags_fd.ptr, 13, nullptr, c.st);
    }
    if (rc) return rc;
    c.done = (size_t)nfd;
    c.hist = c.x + (c.done - f->hcap) * 2; // the hcap samples in front of the remainder are part of the input itself
    return GR4HIP_OK;
}

// 2. complex, no decimation, 33 .. 256 taps, what the fast convolution did not take: the block-Toeplitz product on the f16 matrix pipe, two-term splits under a
// per-segment block exponent (fir_f16.hip).  Every segment judges itself; the marked ones get float64 products behind the launch (FP64 matrix pipe, fir_exact.hip).
static int fir_path_cf16(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!fir_cf16_shape(c)) return GR4HIP_OK;
    if (const int rc = fir_f16_tables(f, c.st, false, true)) return rc;
    if (f->hfKS <= 0) return GR4HIP_OK;
    float*       nh   = c.done == 0 ? c.next_hist() : nullptr;
    const long   nrem = (long)(c.n_in - c.done);
    const float* xr   = c.x + c.done * 2;
    float*       yr   = c.y + c.done * 2;
    int          rc   = f->d_flags.ensure((size_t)ceil_div(nrem, 2048L));
    if (!rc) rc = fir_f16_c32_launch(f->hfKS, xr, nrem, c.hist, (int)f->hcap, f->d_hfrag.ptr, yr, c.st, nh, f->guard_mode != GR4HIP_GUARD_OFF, (unsigned char*)f->d_flags.ptr);
    if (!rc) rc = fir_exact_launch(xr, nrem, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, 1, 1, yr, nrem, (const unsigned char*)f->d_flags.ptr, 11, nullptr, c.st);
    return rc ? rc : c.took(nh != nullptr);
}

// 3. complex, no decimation, 257 .. 1792 taps (seven slices: a slice's window and its delay must fit the kernel's 2048-sample segment): slices of 256 taps on the
// same kernel, each a pass over the input delayed by 256 p samples that adds to y (the f32 matrix pipe at its peak managed 512 taps 36 Gsamples/s, 1024 taps 17).
// The last slice judges the sums against the whole filter's threshold; marked segments again with all the taps on the FP64 matrix pipe.
static int fir_path_cf16_slices(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(f->S == 2 && f->decim == 1 && f->ntaps > 256 && f->ntaps <= 1792 && c.done == 0 && c.n_in >= kMfmaMinSamples / 2 && al16(c.x) && al16(c.y) && fir_cf16_ok(c)))
        return GR4HIP_OK;
    if (const int rc = fir_f16_tables(f, c.st, true, true)) return rc;
    if (f->hfKS <= 0) return GR4HIP_OK;
    const size_t nslice = ceil_div(f->ntaps, (size_t)256);
    const bool   judged = f->guard_mode != GR4HIP_GUARD_OFF;
    int          rc     = f->d_flags.ensure((size_t)ceil_div((long)c.n_in, 2048L));
    for (size_t p = 0; p < nslice && !rc; ++p)
        rc = fir_f16_c32_launch(f->hf_ks[p], c.x, (long)c.n_in, c.hist, (int)f->hcap, (const unsigned short*)f->d_hfrag.ptr + f->hf_off[p], c.y, c.st, p == 0 ? c.next_hist() : nullptr,
                                p + 1 == nslice && judged, (unsigned char*)f->d_flags.ptr, (int)(256 * p), p > 0, (float)(f->tap_power * kGuardSegmentRatio));
    if (!rc) rc = fir_exact_launch(c.x, (long)c.n_in, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, 1, 1, c.y, (long)c.n_in, (const unsigned char*)f->d_flags.ptr, 11, nullptr, c.st);
    return rc ? rc : c.took(true);
}

// 4. complex, no decimation, kCBf16MinTaps .. 256 taps, long 16-byte-aligned span the f16 kernels do not take: the three-term bf16 form of the same product (fir_bf16.hip)
static int fir_path_cbf16(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(f->S == 2 && f->decim == 1 && f->ntaps >= kCBf16MinTaps && f->ntaps <= 256 && c.n_in - c.done >= kMfmaMinSamples / 2 && al16(c.x + c.done * 2) &&
          al16(c.y + c.done * 2) && !no_bf16x3(f) && c.plain))
        return GR4HIP_OK;
    if (const int rc = fir_bf16_tables(f, c.st)) return rc;
    float* nh = c.done == 0 ? c.next_hist() : nullptr;
    if (const int rc = fir_bf16_c32_launch(f->bfKS, c.x + c.done * 2, (long)(c.n_in - c.done), c.hist, (int)f->hcap, f->d_bfrag.ptr, c.y + c.done * 2, c.st, nh)) return rc;
    return c.took_unjudged(nh != nullptr);
}

// 5. complex, no decimation, 33 .. 256 taps, long span with a 16-byte-aligned output: the same product on the f32 MFMA units (fir_mfma_c32_kernel)
static int fir_path_cmfma(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(c.algo != GR4HIP_FIR_EXACT_F32 && f->S == 2 && f->decim == 1 && f->ntaps > 32 && f->ntaps <= 256 && c.n_in - c.done >= kMfmaMinSamples / 2 && al16(c.y + c.done * 2)))
        return GR4HIP_OK;
    if (const int rc = fir_mfma_table(f, c.st)) return rc;
    const float* hw = c.hist; // (hcap = bit_ceil(ntaps) is Kp for 33 .. 256 taps: read in place; a span served by this launch alone also gets its next history from it)
    if ((int)f->hcap != f->mKp) {
        if (const int rc = f->d_histc.ensure(256 * sizeof(float2))) return rc;
        hipLaunchKernelGGL(fir_hist_widen_kernel<float2>, dim3(1), dim3(256), 0, c.st, (const float2*)c.hist, (int)f->hcap, (float2*)f->d_histc.ptr, f->mKp);
        GR4_LAUNCH_CHECK();
        hw = (const float*)f->d_histc.ptr;
    }
    float* nh = (c.done == 0 && (int)f->hcap == f->mKp) ? c.next_hist() : nullptr;
    if (const int rc = fir_mfma_c32_launch(f->mKS, c.x + c.done * 2, (long)(c.n_in - c.done), hw, (const float*)f->d_afrag.ptr, c.y + c.done * 2, c.st, nh)) return rc;
    return c.took_unjudged(nh != nullptr);
}

// 6. float, no decimation, 33 .. 3840 taps, long 16-byte-aligned span: the block-Toeplitz product on the f16 matrix pipe, two-term splits under a per-segment block
// exponent (fir_f16.hip: three products per tap instead of the bf16 form's six); beyond 256 taps slices of 256, each a pass over the input delayed by 256 p samples
// that adds to y (fifteen slices: a slice's window and delay must fit the kernel's 4096-sample segment; 257 / 300 / 383 taps 167 / 148 / 119 Gsamples/s on the other
// kernels, 1100 taps 44).  The last slice judges the sums it leaves in y against the whole filter's threshold; marked segments -- rejected, or with samples the
// block exponent cannot carry in ANY slice -- are evaluated again with all the taps on the FP64 matrix pipe.
static int fir_path_rf16(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(f->S == 1 && f->decim == 1 && f->ntaps > 32 && f->ntaps <= 3840 && c.n_in >= kMfmaMinSamples && al16(c.x) && al16(c.y) && fir_rf16_ok(c))) return GR4HIP_OK;
    if (const int rc = fir_f16_tables(f, c.st, false, false)) return rc;
    if (f->hfKS <= 0) return GR4HIP_OK;
    const size_t nslice = ceil_div(f->ntaps, (size_t)256);
    const float  gthr   = (nslice > 1 || f->guard_ratio != kGuardSegmentRatio) ? (float)(f->tap_power * f->guard_ratio) : 0.f;
    int          rc     = f->d_flags.ensure(ceil_div(c.n_in, (size_t)4096));
    for (size_t p = 0; p < nslice && !rc; ++p)
        rc = fir_f16_launch(f->hf_ks[p], c.x, (long)c.n_in, c.hist, (int)f->hcap, (const unsigned short*)f->d_hfrag.ptr + f->hf_off[p], c.y, c.st, p == 0 ? c.next_hist() : nullptr, 0, 0, 1,
                            (int)(256 * p), p > 0, p + 1 == nslice && f->guard_mode != GR4HIP_GUARD_OFF, (unsigned char*)f->d_flags.ptr, 0, gthr);
    if (!rc) rc = fir_exact_launch(c.x, (long)c.n_in, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, 1, 0, c.y, (long)c.n_in, (const unsigned char*)f->d_flags.ptr, 12, nullptr, c.st);
    return rc ? rc : c.took(true);
}

// 7. float, no decimation, 33 .. 256 or 384 .. 1024 taps, long 16-byte-aligned span the f16 kernel does not take: the product on the bf16 matrix pipe with three-term
// splits of samples and taps (fir_bf16.hip: float32 accuracy, 2.4 times less matrix-pipe time than the f32 MFMA), slices of 256 taps beyond 256 (512 taps 115 instead
// of 90 Gsamples/s on the register-window kernel, 1024 taps 50.5 instead of 47; below 384 and above 1024 taps the extra passes cost more than they save)
static int fir_path_rbf16(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(c.done == 0 && f->S == 1 && f->decim == 1 && f->ntaps > 32 && (f->ntaps <= 256 || (f->ntaps >= 384 && f->ntaps <= 1024)) && c.n_in >= kMfmaMinSamples && al16(c.x) &&
          al16(c.y) && c.algo == GR4HIP_FIR_AUTO && !no_bf16x3(f) && c.plain))
        return GR4HIP_OK;
    if (const int rc = fir_bf16_tables(f, c.st)) return rc;
    const size_t nslice = ceil_div(f->ntaps, (size_t)256);
    int          rc     = GR4HIP_OK;
    for (size_t p = 0; p < nslice && !rc; ++p)
        rc = fir_bf16_launch(f->bf_ks[p], c.x, (long)c.n_in, c.hist, (int)f->hcap, (const unsigned short*)f->d_bfrag.ptr + f->bf_off[p], c.y, c.st, p == 0 ? c.next_hist() : nullptr, 0, 0,
                             1, (int)(256 * p), p > 0);
    return rc ? rc : c.took_unjudged(true);
}

// 8. float, no decimation, 33 .. 256 taps, long span with a 16-byte-aligned output: block-Toeplitz product on the f32 MFMA units (about twice the rate of the
// register-window VALU kernel, which is FP32-issue bound from ~48 taps on)
static int fir_path_rmfma(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(c.algo != GR4HIP_FIR_EXACT_F32 && c.done == 0 && f->S == 1 && f->decim == 1 && f->ntaps > 32 && f->ntaps <= 256 && c.n_in >= kMfmaMinSamples && al16(c.y)))
        return GR4HIP_OK;
    if (const int rc = fir_mfma_table(f, c.st)) return rc;
    // hcap = bit_ceil(ntaps) IS Kp for 33 .. 256 taps: the block's history is read as it lies, and the launch writes the next one (one launch per call instead of
    // three: what a scheduler's 64 Ki-sample chunks cost is launches)
    const float* hw = c.hist;
    if ((int)f->hcap != f->mKp) {
        if (const int rc = f->d_hist256.ensure(256 * sizeof(float2))) return rc;
        hipLaunchKernelGGL(fir_hist_widen_kernel<float>, dim3(1), dim3(256), 0, c.st, c.hist, (int)f->hcap, (float*)f->d_hist256.ptr, f->mKp);
        GR4_LAUNCH_CHECK();
        hw = (const float*)f->d_hist256.ptr;
    }
    float* nh = (int)f->hcap == f->mKp ? c.next_hist() : nullptr;
    if (const int rc = fir_mfma_launch(f->mKS, c.x, (long)c.n_in, hw, (const float*)f->d_afrag.ptr, c.y, (long)((c.n_in + 3) & ~(size_t)3), (long)c.n_in, 1, c.st, nh)) return rc;
    return c.took_unjudged(nh != nullptr);
}

// 9. float or complex, decimate by 4 / 8 / 16 / 32 (BASELINE configs[2]: float, by 8, 1024 taps), long 16-byte-aligned span: the band form on the f16 matrix pipe,
// two-term splits under a per-segment block exponent, the K-steps split over the four waves (fir_decim_f16.hip).  Every segment is judged in the launch; the marked
// ones are evaluated again on the FP64 matrix pipe behind it (in samples: a complex segment is half as many outputs).  Its error is relative to the output, so it
// needs no host-side guard and the call stays asynchronous.  Hooked calls too: the kernel carries the programs, fir_exact_kernel<true> runs them again.
static int fir_path_decim_f16(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(c.done == 0 && fir_decim_f16_shape(f, c.n_in, c.x, c.y, c.hk.any))) return GR4HIP_OK;
    if (f->dhKQ == 0) {
        if (!fir_decim_f16_make_table(f->taps.data(), f->ntaps, f->decim, &f->dhKQ, &f->dhtab_host, f->S == 2)) f->dhKQ = -1;
        else if (const int rc = fir_upload_table(f->d_dhtab, f->dhtab_host, c.st)) { f->dhKQ = 0; return rc; }
    }
    if (f->dhKQ <= 0) return GR4HIP_OK;
    const long segf = 8192 / (long)f->decim; // the kernel's segment: 8192 input floats = this many output floats
    int        rc   = f->d_flags.ensure((size_t)ceil_div((long)(c.n_out * f->S), segf));
    if (!rc)
        rc = fir_decim_f16_launch((int)f->decim, f->dhKQ, c.x, (long)(c.n_in * f->S), c.hist, (int)(f->hcap * f->S), f->d_dhtab.ptr, c.y, (long)(c.n_out * f->S), c.st, c.next_hist(),
                                  f->guard_mode != GR4HIP_GUARD_OFF, (unsigned char*)f->d_flags.ptr, f->S == 2, &c.hk.pre, &c.hk.post);
    if (!rc)
        rc = fir_exact_launch(c.x, (long)c.n_in, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, (int)f->decim, f->S == 2, c.y, (long)c.n_out, (const unsigned char*)f->d_flags.ptr,
                              ilog2((size_t)(segf / f->S)), nullptr, c.st, 1, 0, 0, 0, 0, &c.hk.pre, &c.hk.post);
    return rc ? rc : c.took(true);
}

// 10. float, decimate by 2 .. 12, or complex, by 3 .. 16, window <= 1152 samples, long 16-byte-aligned span: the band form with three-term bf16 products
// (fir_bf16.hip; complex: the rows of a tile alternate between the re and im phases of the window).  The register-window kernel stages a decimator's samples one by
// one (decimate by 8, 64 taps: 171 G input samples/s against 483 here; by 16: 97 against 445; by 2 it is ahead: 389 / 307 against 348 / 252 at 16 / 64 taps).  The
// kernels carry the neighbours' programs and judge every segment; the marked ones are evaluated again on the FP64 matrix pipe, programs included.
static int fir_path_decim_bf16(FirCall& c) {
    gr4hip_fir* f  = c.f;
    int         rc = GR4HIP_OK;
    if (c.done != 0 || !fir_decim_bf16_ready(f, c.n_in, c.x, c.y, &rc, c.st)) return rc;
    const bool judged  = f->guard_mode != GR4HIP_GUARD_OFF && f->ntaps > 1;
    int        seg_out = 0;
    if (judged) { if ((rc = f->d_flags.ensure((size_t)ceil_div((long)(c.n_out * f->S), 512L)))) return rc; }
    rc = fir_decim_bf16_launch(f->bdKS, (int)f->decim, f->bdHb, c.x, (long)(c.n_in * f->S), c.hist, (int)(f->hcap * f->S), f->d_bdfrag.ptr, c.y, (long)(c.n_out * f->S), c.st, c.next_hist(),
                               c.hk.pre.n_ops > 0 ? &c.hk.pre : nullptr, c.hk.post.n_ops > 0 ? &c.hk.post : nullptr, f->S == 2, judged ? (unsigned char*)f->d_flags.ptr : nullptr,
                               (float)(f->tap_power * f->guard_ratio), &seg_out);
    if (rc == GR4HIP_OK && judged)
        rc = fir_exact_launch(c.x, (long)c.n_in, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, (int)f->decim, f->S == 2, c.y, (long)c.n_out, (const unsigned char*)f->d_flags.ptr,
                              ilog2((size_t)(seg_out / f->S)), nullptr, c.st, 1, 0, 0, 0, 0, &c.hk.pre, &c.hk.post);
    if (rc == GR4HIP_OK) return c.took(true);
    if (rc != GR4HIP_UNSUPPORTED) return rc;
    f->bdKS = -1; // (the staged segment does not fit: do not ask again)
    return GR4HIP_OK;
}

// 11. float, decimate by 8, <= 1024 taps, long span with a 16-byte-aligned input: overlap-save blocks of 8192 samples in the frequency domain (fir_decim_fd.hip: ~35
// lane-operations per input sample instead of 2 K / 8 flop), the partial last block in the same launch (through the polyphase kernel it cost a 44 us launch behind
// a 164 us transform kernel).  The guard of path 1 at kDecimFdMinPowerRatio (an anti-alias filter is where strong out-of-band power is removed): strict, segments
// of 2048 outputs judged behind the launch and the marked ones evaluated again in float64; an earlier launch's measurement moves the stream off for good.
static int fir_path_decim_fd(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(c.done == 0 && f->S == 1 && c.algo == GR4HIP_FIR_AUTO && !f->fd_blocked && fir_decim_fd_supported(f->ntaps, f->decim) && f->ntaps <= 1024 && c.n_in >= kDfMinBlocks * kDfHopS &&
          al16(c.x) && !dev_switch(kDevFirNoDecimFd)))
        return GR4HIP_OK;
    int rc = GR4HIP_OK;
    if (!f->dfd && (rc = fir_decim_fd_create(&f->dfd, f->taps.data(), f->ntaps))) return rc;
    const bool guarded = f->guard_mode != GR4HIP_GUARD_OFF && f->ntaps > 1;
    float      ratio;
    if (guarded && fir_decim_fd_power_ratio(f->dfd, false, &ratio)) f->fd_ratio = ratio;
    if (guarded && f->fd_ratio >= 0.f && f->fd_ratio < kDecimFdMinPowerRatio) f->fd_blocked = f->f32_products = true;
    if (f->fd_blocked) return GR4HIP_OK;
    if ((rc = fir_decim_fd_run(f->dfd, c.x, c.n_in, c.hist, (int)f->hcap, c.y, c.st, guarded))) return rc;
    c.took(false);
    if (guarded && f->guard_mode == GR4HIP_GUARD_STRICT) {
        rc = f->d_flags_fd.ensure((size_t)ceil_div((long)c.n_out, 2048L));
        if (!rc) rc = fir_judge_launch(c.x, (long)c.n_in, c.y, (long)c.n_out, (int)f->decim, 0, 11, kDecimFdMinPowerRatio, (unsigned char*)f->d_flags_fd.ptr, c.st);
        if (!rc)
            rc = fir_exact_launch(c.x, (long)c.n_in, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, (int)f->decim, 0, c.y, (long)c.n_out, (const unsigned char*)f->d_flags_fd.ptr,
                                  11, nullptr, c.st);
        if (rc && rc != GR4HIP_UNSUPPORTED) return rc;
    }
    return GR4HIP_OK;
}

// 12. float, decimate by kBandMinDecim .. 128, long span: the band form
static int fir_path_band(FirCall& c) {
    const gr4hip_fir* f = c.f;
    if (!(c.done == 0 && f->S == 1 && f->decim >= kBandMinDecim && f->decim <= 128 && c.n_out >= (1u << 14) && c.algo == GR4HIP_FIR_AUTO)) return GR4HIP_OK;
    return fir_band(c);
}

// 13. float polyphase decimator with 16 .. 256 taps per phase and a long span with a 16-byte-aligned output: the f32 MFMA contraction with the D phase products summed
// in one accumulator tile.  Declines when the de-interleaved segment does not fit the LDS.
static int fir_path_decim_mfma(FirCall& c) {
    gr4hip_fir* f = c.f;
    if (!(c.algo != GR4HIP_FIR_EXACT_F32 && c.done == 0 && f->S == 1 && f->decim >= 2 && ceil_div(f->ntaps, f->decim) >= 16 && ceil_div(f->ntaps, f->decim) <= 256 &&
          c.n_out >= (1u << 14) && al16(c.y)))
        return GR4HIP_OK;
    if (const int rc = fir_mfma_table(f, c.st)) return rc;
    const int hl = f->mKp * (int)f->decim; // history the kernel wants: Kp D samples
    if (const int rc = f->d_hist256.ensure((size_t)hl * sizeof(float))) return rc;
    const int hu = (int)std::min<size_t>(f->hcap, (size_t)hl); // newest hu samples of the block's history are what the kernel can see
    hipLaunchKernelGGL(fir_hist_widen_kernel<float>, dim3((unsigned)ceil_div(hl, 256)), dim3(256), 0, c.st, c.hist + (f->hcap - hu), hu, (float*)f->d_hist256.ptr, hl);
    GR4_LAUNCH_CHECK();
    const int rc = fir_mfma_decim_launch(f->mKS, (int)f->decim, c.x, (const float*)f->d_hist256.ptr, (const float*)f->d_afrag.ptr, c.y, (long)c.n_out, c.st);
    if (rc == GR4HIP_UNSUPPORTED) return GR4HIP_OK;
    return rc ? rc : c.took_unjudged(false);
}

// 14. the register-window kernel of this file at the largest workgroup size whose D phase rows fit the LDS; the only kernel that takes the rest of a span, and
// hooked calls of every shape the band-form decimators do not take.  It judges itself.
static int fir_path_window(FirCall& c) {
    const gr4hip_fir* f = c.f;
    const int         E = 4 / f->S;
    for (int bs : {256, 128, 64}) {
        const size_t Lf  = (size_t)bs * kFirR + 4 * (size_t)f->G;
        const size_t lds = f->decim * (Lf + (size_t)f->G * E) * sizeof(float);
        if (lds > 150 * 1024) continue;
        const float* xr = c.x + c.done * f->S;
        float*       yr = c.y + (c.done / f->decim) * f->S;
        const long   ni = (long)(c.n_in - c.done), no = (long)((c.n_in - c.done) / f->decim);
        float*       nh = c.done == 0 ? c.next_hist() : nullptr; // the whole span in this launch: it writes the next history itself
        int          rc;
        if (f->S == 1) rc = bs == 256 ? fir_launch<1, 256>(f, xr, c.hist, yr, ni, no, lds, c.st, nh, c.hk) : bs == 128 ? fir_launch<1, 128>(f, xr, c.hist, yr, ni, no, lds, c.st, nh, c.hk) : fir_launch<1, 64>(f, xr, c.hist, yr, ni, no, lds, c.st, nh, c.hk);
        else rc = bs == 256 ? fir_launch<2, 256>(f, xr, c.hist, yr, ni, no, lds, c.st, nh, c.hk) : bs == 128 ? fir_launch<2, 128>(f, xr, c.hist, yr, ni, no, lds, c.st, nh, c.hk) : fir_launch<2, 64>(f, xr, c.hist, yr, ni, no, lds, c.st, nh, c.hk);
        return rc ? rc : c.took(nh != nullptr);
    }
    return GR4HIP_OK;
}

// 15. float decimator whose D phase rows do not fit the LDS at any workgroup size: the band form at any span length
static int fir_path_band_fallback(FirCall& c) {
    if (!(c.done == 0 && c.f->S == 1 && c.f->decim >= 2 && c.plain)) return GR4HIP_OK;
    return fir_band(c);
}

// 16. no tiling fits (decimation x taps beyond every LDS tiling, e.g. complex data decimated by 100): the one-output-per-lane kernel
static int fir_path_generic(FirCall& c) {
    const gr4hip_fir* f = c.f;
    if (!(c.done == 0 && c.plain)) return GR4HIP_OK;
    const unsigned g = (unsigned)ceil_div((long)c.n_out, 256L);
    if (f->S == 1) hipLaunchKernelGGL(fir_generic_kernel<1>, dim3(g), dim3(256), 0, c.st, c.x, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, (long)f->decim, c.y, (long)c.n_out, (long)c.n_in);
    else hipLaunchKernelGGL(fir_generic_kernel<2>, dim3(g), dim3(256), 0, c.st, c.x, c.hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, (long)f->decim, c.y, (long)c.n_out, (long)c.n_in);
    GR4_LAUNCH_CHECK();
    return c.took_unjudged(false);
}

static int fir_process_core(gr4hip_fir_t* f, const void* d_in, size_t n_in, void* d_out, gr4hip_stream_t stream, const FirHooks& hk) {
    static int (*const kPaths[])(FirCall&) = {fir_path_cfast, fir_path_cf16, fir_path_cf16_slices, fir_path_cbf16, fir_path_cmfma, fir_path_rf16, fir_path_rbf16, fir_path_rmfma,
                                              fir_path_decim_f16, fir_path_decim_bf16, fir_path_decim_fd, fir_path_band, fir_path_decim_mfma, fir_path_window, fir_path_band_fallback,
                                              fir_path_generic};
    // hooks run in the register-window kernel and the band-form decimators only: the matrix-pipe and frequency-domain kernels are for plain filters
    FirCall c{f, static_cast<const float*>(d_in), static_cast<float*>(d_out), n_in, n_in / f->decim, as_stream(stream), hk, !hk.any, hk.any ? (int)GR4HIP_FIR_EXACT_F32 : f->algo,
              (const float*)f->hist.current()};
    for (size_t p = 0; p < sizeof(kPaths) / sizeof(kPaths[0]); ++p) {
        if (c.done == n_in) break;
        const size_t before = c.done;
        if (const int rc = kPaths[p](c)) return rc;
        if (c.done != before) f->last_paths |= 1u << (p + 1);
    }
    if (c.done != n_in) { set_error("fir_process: ntaps=%zu decim=%zu does not fit the LDS tiling", f->ntaps, f->decim); return GR4HIP_UNSUPPORTED; }
    // the guard's verdict and second evaluation behind a kernel that does not judge itself
    if (c.unj_from != SIZE_MAX && f->guard_mode != GR4HIP_GUARD_OFF && f->ntaps > 1) {
        const long   ni = (long)(n_in - c.unj_from), no = ni / (long)f->decim;
        const int    shift = f->S == 2 ? 10 : 11;
        const float* xr = c.x + c.unj_from * f->S;
        float*       yr = c.y + (c.unj_from / f->decim) * f->S;
        if (no > 0) {
            if (const int rc = f->d_flags.ensure((size_t)ceil_div(no, 1L << shift))) return rc;
            if (const int rc = fir_judge_launch(xr, ni, yr, no, (int)f->decim, f->S == 2, shift, (float)(f->tap_power * kGuardSegmentRatio), (unsigned char*)f->d_flags.ptr, c.st,
                                                f->guard_ratio != kGuardSegmentRatio ? (float)(f->tap_power * f->guard_ratio) : 0.f)) // (a tighter ratio: on the segment's whole output power -- the quietest quarter dips on narrow-band noise)
                return rc;
            const int rc = fir_exact_launch(xr, ni, c.unj_hist, (int)f->hcap, (const float*)f->d_tapsf.ptr, (int)f->ntaps, (int)f->decim, f->S == 2, yr, no, (const unsigned char*)f->d_flags.ptr, shift, nullptr, c.st);
            f->last_paths |= 1u;
            if (rc && rc != GR4HIP_UNSUPPORTED) return rc; // (UNSUPPORTED: decimation x taps beyond what the second evaluation stages -- the float32 sums stand)
        }
    }
    return fir_advance(f, c.x, n_in, c.st, c.hist_written);
}

extern "C" int gr4hip_fir_process(gr4hip_fir_t* f, const void* d_in, size_t n_in, void* d_out, size_t* n_out_p, gr4hip_stream_t stream) {
    GR4_REQUIRE(f, "fir_process: null handle");
    GR4_REQUIRE(n_in % f->decim == 0, "fir_process: n_in=%zu is not a multiple of decim=%zu", n_in, f->decim);
    const size_t n_out = n_in / f->decim;
    if (n_out_p) *n_out_p = n_out;
    f->last_paths = 0;
    if (n_in == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in && d_out, "fir_process: null device pointer");
    FirHooks hk;
    if (f->pre || f->post || f->folded != 1.0) { if (const int rc = fir_prepare_hooks(f, &hk, as_stream(stream))) return rc; }
    if (const int rc = fir_state_on(f, as_stream(stream))) return rc; // pending reset / tap upload / history rescale: onto this call's stream, in front of its launches
    // Neighbours that do not fold into the taps are load / store hooks of the register-window kernel.  Where a plain filter of this shape takes a matrix-pipe or
    // frequency-domain kernel instead (more than 32 taps on a long span, the float decimators), that kernel is worth more than the saved pass: add -> 256-tap FIR
    // measured 165 Gsamples/s hooked against 277 as an element-wise launch + the bf16 kernel.  There the program runs as ONE element-wise launch in front of
    // (behind) the filter's own -- same results, same history (the filter sees, and remembers, the prologue's output); everything else stays one launch.
    // (where the crossover lies, float, 2^27 samples: add -> 64 taps 432 hooked / 347 as two launches; -> 256 taps 165 / 258; the register-window kernel is FP32-bound
    // from ~48 taps per output on, the element-wise launch costs one pass at ~740 Gsamples/s)
    const size_t per_out    = ceil_div(f->ntaps, f->decim); // taps per computed output
    const bool   fast_shape = f->algo == GR4HIP_FIR_AUTO && ((f->decim == 1 && f->ntaps > (f->S == 2 ? (size_t)64 : (size_t)96) && f->ntaps <= (f->S == 2 ? (size_t)256 : (size_t)1024) && n_in >= kMfmaMinSamples) ||
                                                               (f->S == 1 && f->decim >= 2 && per_out > 12 && n_out >= ((size_t)1 << 14)));
    int        brc  = GR4HIP_OK;
    const bool band = hk.any && (fir_decim_f16_shape(f, n_in, d_in, d_out, true) || fir_decim_bf16_ready(f, n_in, d_in, d_out, &brc, as_stream(stream))); // (those kernels carry the hooks themselves)
    if (brc) return brc;
    auto around = [&]() -> int { // the programs as element-wise launches in front of / behind the plain filter
        hipStream_t st  = as_stream(stream);
        const void* src = d_in;
        if (hk.pre.n_ops > 0) {
            if (const int rc = f->d_pre.ensure(n_in * f->S * sizeof(float))) return rc;
            if (const int rc = ewise_run(hk.pre, f->dtype, d_in, f->d_pre.ptr, (long)n_in, st)) return rc;
            src = f->d_pre.ptr;
        }
        FirHooks none;
        if (const int rc = fir_process_core(f, src, n_in, d_out, stream, none)) return rc;
        if (hk.post.n_ops > 0) return ewise_run(hk.post, f->dtype, d_out, d_out, (long)n_out, st);
        return GR4HIP_OK;
    };
    if (hk.any && fast_shape && !band) { f->last_paths |= 1u << 17; return around(); }
    const int rc = fir_process_core(f, d_in, n_in, d_out, stream, hk);
    //  a hooked decimator whose phase rows do not fit the register-window kernel's LDS at any workgroup size (decimation ~100 with few taps) -- the one kernel
    // that carries hooks there -- is served like the fast shapes: nothing has been launched or moved when the core says UNSUPPORTED
    if (rc == GR4HIP_UNSUPPORTED && hk.any) { f->last_paths |= 1u << 17; return around(); }
    return rc;
}

// Test hook, not ABI (declared in no header): the paths that served the last gr4hip_fir_process call -- bit p (1 .. 16) for each path of fir_process_core's
// kPaths that advanced the span, bit 0 when the common tail judged an unjudged part and evaluated its marked segments again, bit 17 when the call ran as
// element-wise launches around the plain filter
extern "C" int gr4hip_internal_fir_last_paths(const gr4hip_fir_t* f, unsigned* mask) {
    GR4_REQUIRE(f && mask, "fir_last_paths: null argument");
    *mask = f->last_paths;
    return GR4HIP_OK;
}

// ------------------------------------------------------------------------------------------------ decimating FIR -> IIR cascade (BASELINE configs[2])
int  gr4hip_internal_iir_fusable(gr4hip_iir_t* f, const float** d_tab, int* nsec, const float** d_state_in, float** d_state_out, int* warm_blocks, hipStream_t st); // iir.hip
void gr4hip_internal_iir_commit(gr4hip_iir_t* f);

extern "C" int gr4hip_fir_iir_process(gr4hip_fir_t* f, gr4hip_iir_t* iir, const float* d_in, size_t n_in, float* d_out, size_t* n_out_p, int mode, gr4hip_stream_t stream) {
    GR4_REQUIRE(f && iir, "fir_iir_process: null handle");
    GR4_REQUIRE(mode >= GR4HIP_FIR_IIR_AUTO && mode <= GR4HIP_FIR_IIR_TWO_LAUNCHES, "fir_iir_process: unknown mode %d", mode);
    GR4_REQUIRE(f->dtype == GR4HIP_F32, "fir_iir_process: a float filter in front of the float cascade");
    GR4_REQUIRE(n_in % f->decim == 0, "fir_iir_process: n_in=%zu is not a multiple of decim=%zu", n_in, f->decim);
    const size_t n_out = n_in / f->decim;
    if (n_out_p) *n_out_p = n_out;
    if (n_in == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in && d_out, "fir_iir_process: null device pointer");
    hipStream_t  st = as_stream(stream);
    const auto two_launches = [&](const float* x, size_t n, float* y) -> int { // the decimated stream through HBM (f->d_pre as scratch)
        if (const int rc = f->d_mid.ensure(std::max<size_t>(n / f->decim, 1) * sizeof(float))) return rc;
        float* mid = static_cast<float*>(f->d_mid.ptr);
        if (const int rc = gr4hip_fir_process(f, x, n, mid, nullptr, stream)) return rc;
        return gr4hip_iir_process(iir, mid, n / f->decim, y, stream);
    };
    const float*     tab = nullptr;
    const float*     st_in = nullptr;
    float*           st_out = nullptr;
    int              nsec = 0, warm = 0;
    const size_t     whole = n_in / kDfHopS * kDfHopS;
    if (f->folded != 1.0 && !f->pre && !f->post) { // (a gain prologue / epilogue that was taken off again left its factor in the taps on this path: gr4hip_fir_process undoes it
                                                   // through fir_prepare_hooks, the fused launch below never came by there)
        FirHooks hk0;
        if (const int rc = fir_prepare_hooks(f, &hk0, st)) return rc;
    }
    if (const int rc = fir_state_on(f, st)) return rc;
    const bool       fusable = mode == GR4HIP_FIR_IIR_ONE_LAUNCH && f->S == 1 && f->decim == 8 && f->algo == GR4HIP_FIR_AUTO && !f->fd_blocked && !f->pre && !f->post && fir_decim_fd_supported(f->ntaps, f->decim) && f->ntaps <= 1024 &&
                         whole >= kDfMinBlocks * kDfHopS && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 7) == 0 && !dev_switch(kDevFirNoDecimFd) &&
                         gr4hip_internal_iir_fusable(iir, &tab, &nsec, &st_in, &st_out, &warm, st);
    if (!fusable) return two_launches(d_in, n_in, d_out);
    int rc = GR4HIP_OK;
    if (!f->dfd) rc = fir_decim_fd_create(&f->dfd, f->taps.data(), f->ntaps);
    if (rc) return rc;
    // the decimator's dynamic-range guard as in gr4hip_fir_process: its own measurement decides (strict: before this call returns -- nothing of the launch is kept, the
    // cascade's state included), a finished earlier launch decides (deferred)
    const bool      guarded = f->guard_mode != GR4HIP_GUARD_OFF && f->ntaps > 1;
    float           ratio;
    if (guarded && fir_decim_fd_power_ratio(f->dfd, false, &ratio)) f->fd_ratio = ratio;
    if (guarded && f->guard_mode == GR4HIP_GUARD_DEFERRED && f->fd_ratio >= 0.f && f->fd_ratio < kDecimFdMinPowerRatio) { f->fd_blocked = f->f32_products = true; return two_launches(d_in, n_in, d_out); }
    const float*     hist = (const float*)f->hist.current();
    const DecimFdIir fuse{tab, nsec, st_in, st_out, warm};
    rc = fir_decim_fd_run(f->dfd, d_in, whole, hist, (int)f->hcap, d_out, st, guarded, &fuse);
    if (rc) return rc;
    if (guarded && f->guard_mode == GR4HIP_GUARD_STRICT) {
        if (fir_decim_fd_power_ratio(f->dfd, true, &ratio)) f->fd_ratio = ratio;
        if (f->fd_ratio >= 0.f && f->fd_ratio < kDecimFdMinPowerRatio) { f->fd_blocked = f->f32_products = true; return two_launches(d_in, n_in, d_out); } // (neither handle has moved)
    }
    gr4hip_internal_iir_commit(iir);
    if (const int rc = fir_advance(f, d_in, whole, st, false)) return rc; // the filter's history moves behind the whole blocks
    if (whole < n_in) return two_launches(d_in + whole, n_in - whole, d_out + whole / 8); // what is left of the span (< one block): the polyphase kernel and the cascade's own
    return GR4HIP_OK;
}

// (library-internal, chain.hip) make `d_last256` -- the 256 complex samples in front of the next input sample -- this filter's history: the fused chain
// hands its stream over to the direct-form kernels when the dynamic-range guard switches algorithms
// (library-internal, chain.hip) the per-segment guard's threshold as a multiple of (sum b^2): before the first call (the matrix-pipe kernels' tables carry it).  Non-decimating filters only
int gr4hip_internal_fir_set_guard_ratio(gr4hip_fir_t* f, double ratio) {
    GR4_REQUIRE(f && f->decim == 1 && ratio > 0 && ratio <= 1.0, "fir_set_guard_ratio: a non-decimating filter and a ratio in (0, 1] expected");
    f->guard_ratio = ratio;
    if (f->hfKS > 0) f->hfKS = 0; // (a table built already is built again with the new threshold)
    return GR4HIP_OK;
}
int gr4hip_internal_fir_load_history(gr4hip_fir_t* f, const float* d_last256, hipStream_t st) {
    GR4_REQUIRE(f && f->S == 2 && f->hcap <= 256, "fir_load_history: complex filter with <= 256 samples of history expected");
    f->hist.keep(); // (what was pending for the history is superseded; the taps go up with the next call)
    f->hist_rescale = 1.0;
    GR4_HIP_TRY(hipMemcpyAsync(f->hist.current(), d_last256 + (256 - f->hcap) * 2, f->hcap * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return GR4HIP_OK;
}

extern "C" {

int gr4hip_fir_destroy(gr4hip_fir_t* f) {
    if (f && f->fd) chain_fused_destroy(f->fd);
    if (f && f->dfd) fir_decim_fd_destroy(f->dfd);
    delete f;
    return GR4HIP_OK;
}

int gr4hip_decimate(int dtype, const void* d_in, size_t n_in, size_t decim, void* d_out, size_t* n_out_p, gr4hip_stream_t stream) {
    const size_t es = dtype_size(dtype);
    GR4_REQUIRE(es, "decimate: unknown dtype %d", dtype);
    GR4_REQUIRE(decim >= 1, "decimate: decim must be >= 1");
    const size_t n_out = ceil_div(n_in, decim); // i % decim == 0 for i in [0, n_in)
    if (n_out_p) *n_out_p = n_out;
    if (n_out == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_in && d_out, "decimate: null device pointer");
    const unsigned grid = (unsigned)std::min<size_t>(ceil_div(n_out, (size_t)256), 4096);
    hipStream_t    st   = as_stream(stream);
    switch (es) {
    case 1: hipLaunchKernelGGL(decimate_kernel<uint8_t>, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_in, (uint8_t*)d_out, (long)n_out, (long)decim); break;
    case 2: hipLaunchKernelGGL(decimate_kernel<uint16_t>, dim3(grid), dim3(256), 0, st, (const uint16_t*)d_in, (uint16_t*)d_out, (long)n_out, (long)decim); break;
    case 4: hipLaunchKernelGGL(decimate_kernel<uint32_t>, dim3(grid), dim3(256), 0, st, (const uint32_t*)d_in, (uint32_t*)d_out, (long)n_out, (long)decim); break;
    case 8: hipLaunchKernelGGL(decimate_kernel<uint64_t>, dim3(grid), dim3(256), 0, st, (const uint64_t*)d_in, (uint64_t*)d_out, (long)n_out, (long)decim); break;
    default: hipLaunchKernelGGL(decimate_kernel<ulonglong2>, dim3(grid), dim3(256), 0, st, (const ulonglong2*)d_in, (ulonglong2*)d_out, (long)n_out, (long)decim); break;
    }
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

} // extern "C"
