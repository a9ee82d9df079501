// iq_demod.hip -- IQDemodulator<T> (blocks/filter/.../FrequencyEstimator.hpp:356-653), T = float / double: a digital lock-in amplifier.
//
// Per sample the block runs a DC-blocking high-pass on each input, a derivative FIR on the reference, five products and five one-pole low-passes; at the last
// sample of every chunk of C inputs it reads amplitude, phase and frequency off the low-pass states (include/gr4hip.h "IQ demodulator", IQ_DEMOD.md).  Every
// state is float64, the coefficients are the reference's, computed in T.  Both recurrences are linear with constant coefficients, so a lane's run of J samples
// maps its start state c to A^J c + z (z: the run from zero state) and a segment of S = 256 J samples to A^S c + z, A^J and A^S from the host.  Carries are
// exact: no warm-up, no look-back window.  A call is five launches on its stream:
//   iqd_hp_reduce_kernel   per segment but the last: the zero-state high-pass of both inputs, its last 6 (reference) / 3 (response) values;
//   iqd_carry_scan_kernel  one workgroup: the two high-pass states in front of every segment, seeded from the handle;
//   iqd_mix_kernel         per segment: lane carries by an in-block scan, the true high-pass, the derivative (its halo: the previous lane's or segment's true
//                          last values), the products, every lane's zero-state low-pass end (kept) and the segment's;
//   iqd_carry_scan_kernel  the five low-pass states in front of every segment;
//   iqd_out_kernel         per segment: the same again, the low-passes from their true lane carries, the outputs at every chunk end, the handle's next state.
// A non-finite input poisons the states for good, as in the reference: NaN stays in every multiply-add carry chain, every later `> eps` test fails, the
// outputs are 0.  Where the reference's float arithmetic is ill-conditioned (DC-only input, whose high-passed value decays below rounding; |ratio / G| near 1
// in the asin) the device gives the float64 result, not the float32 noise.
#include "common.hpp"

#include <cmath>

namespace gr4 {

constexpr int  kIqdLanes = 256;
constexpr int  kIqdJ     = 32;                       // samples per lane
constexpr long kIqdS     = (long)kIqdLanes * kIqdJ;  // samples per segment (one workgroup)
constexpr int  kIqdScan  = 1024;                     // lanes of the carry scan
constexpr int  kIqdState = 16;                       // doubles of a handle state (below)

// Handle state (double[16]): [0..5] h_ref at the last sample - j (j = 0: the high-pass state), [6..8] h_resp likewise, [9] / [10] the last ref / resp input,
// [11..15] the low-pass states I, Q, Pr, Pd, Px.
struct IqdCoef {
    double ahp, alp;     // alpha_hp, alpha_lp (computed in T)
    double tap[7];       // tap[k] multiplies h_ref[n - k] (the reference's time-reversed kernel)
    double hpJ[8];       // alpha_hp^(J 2^k)
    double lpJ[8];       // (1 - alpha_lp)^(J 2^k)
    double hpTailJ[6];   // alpha_hp^(J - j)
    double hpTailS[6];   // alpha_hp^(S - j)
    double lpS;          // (1 - alpha_lp)^S
    double eps, fs, g0;  // epsilon (T), sample rate (T), the DC gain factor
    double g08, g02, pi; // T(0.8), T(0.2), pi_v<T>
    int    degrees, invert;
};

__device__ __forceinline__ double iqd_sel4(const double v[4], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3]; }

// 4 samples from p on (p - lane start a multiple of 4, lane starts multiples of 32): one or two 16-byte loads where the span is whole and aligned
template <typename T>
__device__ __forceinline__ void iqd_load4(const T* __restrict__ x, long p, long n, bool vec, double v[4]) {
    if (vec && p + 4 <= n) {
        if constexpr (sizeof(T) == 4) {
            const float4 q = *reinterpret_cast<const float4*>(x + p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const double2 a = *reinterpret_cast<const double2*>(x + p), b = *reinterpret_cast<const double2*>(x + p + 2);
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p + k < n ? (double)x[p + k] : 0.0;
    }
}

// inclusive scan over the block's lanes of  v <- A^J v_prev + v  for NCH channels (pw[k] = A^(J 2^k)); sh is [NCH][256]
template <int NCH>
__device__ __forceinline__ void iqd_block_scan(double (*sh)[kIqdLanes], double v[NCH], const double* pw) {
    const int t = threadIdx.x;
    __syncthreads(); // (sh may still be read by an earlier use)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) sh[ch][t] = v[ch];
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
        const int off = 1 << k;
        double    q[NCH];
        if (t >= off) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) q[ch] = pw[k] * sh[ch][t - off];
        }
        __syncthreads();
        if (t >= off) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) { v[ch] += q[ch]; sh[ch][t] = v[ch]; }
        }
        __syncthreads();
    }
}

// the zero-state high-pass over a lane's m samples from input v[p0 - 1] = vr / vx: its last values (zr[j]: sample p0 + m - 1 - j)
template <typename T>
__device__ __forceinline__ void iqd_hp_zero(const T* __restrict__ r, const T* __restrict__ x, long p0, int m, long n, bool vec, double vr, double vx, double a,
                                            double zr[6], double zx[3]) {
    double hr = 0.0, hx = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) zr[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) zx[j] = 0.0;
    if (vec && m == kIqdJ) { // a whole lane (the first touch of the input in every pass): all loads of a half-lane in flight before the first use
#pragma unroll
        for (int h = 0; h < kIqdJ; h += 16) {
            double br[16], bx[16];
#pragma unroll
            for (int q = 0; q < 16; q += 4) {
                iqd_load4(r, p0 + h + q, n, true, br + q);
                iqd_load4(x, p0 + h + q, n, true, bx + q);
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                hr = a * (hr + br[k] - vr);
                vr = br[k];
                hx = a * (hx + bx[k] - vx);
                vx = bx[k];
                if (h + k >= kIqdJ - 6) zr[kIqdJ - 1 - h - k] = hr;
                if (h + k >= kIqdJ - 3) zx[kIqdJ - 1 - h - k] = hx;
            }
        }
        return;
    }
#pragma unroll 1
    for (int g = 0; g < m; g += 4) {
        double br[4], bx[4];
        iqd_load4(r, p0 + g, n, vec, br);
        iqd_load4(x, p0 + g, n, vec, bx);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (g + k < m) {
                hr = a * (hr + br[k] - vr);
                vr = br[k];
                hx = a * (hx + bx[k] - vx);
                vx = bx[k];
#pragma unroll
                for (int j = 5; j > 0; --j) zr[j] = zr[j - 1];
#pragma unroll
                for (int j = 2; j > 0; --j) zx[j] = zx[j - 1];
                zr[0] = hr;
                zx[0] = hx;
            }
        }
    }
}

__device__ __forceinline__ double iqd_clamp1(double v) { return v < -1.0 ? -1.0 : (1.0 < v ? 1.0 : v); } // std::clamp: NaN stays NaN

template <int M>
__device__ __forceinline__ double iqd_gain(double om, const IqdCoef& c) { // computeGainFactor (:590-598)
    if constexpr (M == 0) return 2.0;
    const double cs = cos(om);
    if constexpr (M == 1) return c.g08 * cs + c.g02;
    return (6.0 * cs * cs + 2.0 * cs - 1.0) / 7.0;
}

// step 5 (:571-640) in float64 on the low-pass states s = {I, Q, Pr, Pd, Px}
template <int M>
__device__ __forceinline__ void iqd_extract(const double s[5], const IqdCoef& c, double& amp, double& ph, double& fr) {
    const double I = s[0], Q = s[1], Pr = s[2], Pd = s[3], Px = s[4], eps = c.eps;
    amp = (Pr > eps && Px > eps) ? sqrt(Px / Pr) : 0.0;
    fr  = 0.0;
    ph  = 0.0;
    if (Pr > eps && Pd > eps) {
        const double ratio = sqrt(Pd / Pr);
        double       om0   = asin(iqd_clamp1(ratio / c.g0));
#pragma unroll 1
        for (int it = 0; it < 3; ++it) { // three rounds of three iterations and an Aitken step
            const double om1 = asin(iqd_clamp1(ratio / iqd_gain<M>(om0, c)));
            const double om2 = asin(iqd_clamp1(ratio / iqd_gain<M>(om1, c)));
            const double om3 = asin(iqd_clamp1(ratio / iqd_gain<M>(om2, c)));
            const double den = om3 - 2.0 * om2 + om1;
            if (fabs(den) > eps) {
                const double dl = om2 - om1;
                om0 = om1 - dl * dl / den;
            } else {
                om0 = om3;
            }
        }
        fr = om0 * c.fs / (2.0 * c.pi);
        if (fabs(I) > eps || fabs(Q) > eps) ph = atan2(Q, I * ratio);
    }
    if (c.invert) ph = -ph;
    if (c.degrees) ph *= 180.0 / c.pi;
}

// The true chain over a lane's m samples from the high-pass rings hr (h_ref[p0 - 1 - j] in hr[j], j < 6) / hx (j < 3), the inputs v[p0 - 1] = vr / vx and
// the low-pass states s.  On return the rings, vr / vx and s are the states after the lane's last sample.  OUT: the outputs of every chunk ending in the lane.
template <typename T, int M, bool OUT>
__device__ __forceinline__ void iqd_true_run(const T* __restrict__ r, const T* __restrict__ x, long p0, int m, long n, bool vec, long seen, const IqdCoef& c,
                                             double hr[7], double hx[4], double& vr, double& vx, double s[5], long C, T* __restrict__ amp,
                                             T* __restrict__ ph, T* __restrict__ fr) {
    constexpr int K = M == 0 ? 3 : M == 1 ? 5 : 7, D = M + 1; // taps, delay (:480-501)
    const double  a = c.ahp, al = c.alp;
    long          e = OUT ? (p0 / C + 1) * C - 1 : 0; // the next chunk end
#pragma unroll 1
    for (int g = 0; g < m; g += 4) {
        double br[4], bx[4];
        iqd_load4(r, p0 + g, n, vec, br);
        iqd_load4(x, p0 + g, n, vec, bx);
        const int cnt = min(4, m - g);
#pragma unroll 1
        for (int k = 0; k < cnt; ++k) {
            const long   p   = p0 + g + k;
            const double ur  = iqd_sel4(br, k), ux = iqd_sel4(bx, k);
            const double h_r = a * (hr[0] + ur - vr), h_x = a * (hx[0] + ux - vx); // (:527-531)
            vr = ur;
            vx = ux;
#pragma unroll
            for (int j = 6; j > 0; --j) hr[j] = hr[j - 1];
#pragma unroll
            for (int j = 3; j > 0; --j) hx[j] = hx[j - 1];
            hr[0] = h_r;
            hx[0] = h_x;
            double rq = 0.0;
            if (seen + p + 1 >= K) { // _ref_history.size() >= kernel size (:548-551)
                rq = c.tap[0] * hr[0];
#pragma unroll
                for (int j = 1; j < K; ++j) rq = fma(c.tap[j], hr[j], rq);
            }
            const double ri = hr[D], xi = hx[D]; // (:554-555: 0 before d samples -- the zeroed history of a fresh state)
            s[0] += al * (xi * ri - s[0]);
            s[1] += al * (xi * rq - s[1]);
            s[2] += al * (ri * ri - s[2]);
            s[3] += al * (rq * rq - s[3]);
            s[4] += al * (xi * xi - s[4]);
            if (OUT && p == e) {
                double A, P, F;
                iqd_extract<M>(s, c, A, P, F);
                const long j = (p + 1) / C - 1;
                amp[j] = (T)A;
                ph[j]  = (T)P;
                fr[j]  = (T)F;
                e += C;
            }
        }
    }
}

// A lane's high-pass start: the zero-state run, the in-block scan seeded with the segment's carries chp[s], this lane's true last values into LDS, and the
// rings from the previous lane's (lane 0: the previous segment's true last values, from its carry and zero-state tail hpz; segment 0: the handle's).
template <typename T>
__device__ __forceinline__ void iqd_hp_start(const T* __restrict__ r, const T* __restrict__ x, long s, long p0, int m, long n, bool vec, const double* __restrict__ st,
                                             const IqdCoef& c, const double* __restrict__ hpz, const double* __restrict__ chp, double (*sh)[kIqdLanes],
                                             double (*tl)[kIqdLanes], double hr[7], double hx[4], double& vr, double& vx) {
    const int t = threadIdx.x;
    vr = p0 == 0 ? st[9] : m > 0 ? (double)r[p0 - 1] : 0.0;
    vx = p0 == 0 ? st[10] : m > 0 ? (double)x[p0 - 1] : 0.0;
    double zr[6], zx[3];
    iqd_hp_zero(r, x, p0, m, n, vec, vr, vx, c.ahp, zr, zx);
    const double cr = chp[2 * s], cx = chp[2 * s + 1];
    double       v[2] = {zr[0], zx[0]};
    if (t == 0) {
        v[0] += c.hpJ[0] * cr;
        v[1] += c.hpJ[0] * cx;
    }
    iqd_block_scan<2>(sh, v, c.hpJ);
    const double inr = t ? sh[0][t - 1] : cr, inx = t ? sh[1][t - 1] : cx; // this lane's start state
#pragma unroll
    for (int j = 0; j < 6; ++j) tl[j][t] = c.hpTailJ[j] * inr + zr[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) tl[6 + j][t] = c.hpTailJ[j] * inx + zx[j];
    __syncthreads();
    if (t > 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) hr[j] = tl[j][t - 1];
#pragma unroll
        for (int j = 0; j < 3; ++j) hx[j] = tl[6 + j][t - 1];
    } else if (s == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) hr[j] = st[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) hx[j] = st[6 + j];
    } else { // hpz[s - 1]: {ref end, resp end, ref j = 1..5, resp j = 1..2}
        const double  pr = chp[2 * (s - 1)], px = chp[2 * (s - 1) + 1];
        const double* z  = hpz + (s - 1) * 9;
        hr[0] = c.hpTailS[0] * pr + z[0];
        hx[0] = c.hpTailS[0] * px + z[1];
#pragma unroll
        for (int j = 1; j < 6; ++j) hr[j] = c.hpTailS[j] * pr + z[1 + j];
#pragma unroll
        for (int j = 1; j < 3; ++j) hx[j] = c.hpTailS[j] * px + z[6 + j];
    }
    hr[6] = 0.0;
    hx[3] = 0.0;
}

__device__ __forceinline__ int iqd_lane_count(long p0, long n) { return p0 >= n ? 0 : (int)min((long)kIqdJ, n - p0); }

// pass 1: per segment, the zero-state high-pass tail {ref end, resp end, ref j = 1..5, resp j = 1..2} (samples S - 1 - j of the segment)
template <typename T>
__global__ __launch_bounds__(kIqdLanes) void iqd_hp_reduce_kernel(const T* __restrict__ r, const T* __restrict__ x, long n, bool vec, const double* __restrict__ st,
                                                                  IqdCoef c, double* __restrict__ hpz) {
    __shared__ double sh[2][kIqdLanes];
    const int    t  = threadIdx.x;
    const long   p0 = (long)blockIdx.x * kIqdS + (long)t * kIqdJ;
    const int    m  = iqd_lane_count(p0, n);
    const double vr = p0 == 0 ? st[9] : m > 0 ? (double)r[p0 - 1] : 0.0, vx = p0 == 0 ? st[10] : m > 0 ? (double)x[p0 - 1] : 0.0;
    double       zr[6], zx[3];
    iqd_hp_zero(r, x, p0, m, n, vec, vr, vx, c.ahp, zr, zx);
    double v[2] = {zr[0], zx[0]};
    iqd_block_scan<2>(sh, v, c.hpJ);
    if (t == kIqdLanes - 1) {
        const double pr = sh[0][t - 1], px = sh[1][t - 1]; // the segment's zero-state at the start of the last lane
        double*      o  = hpz + (long)blockIdx.x * 9;
        o[0] = v[0];
        o[1] = v[1];
        for (int j = 1; j < 6; ++j) o[1 + j] = c.hpTailJ[j] * pr + zr[j];
        for (int j = 1; j < 3; ++j) o[6 + j] = c.hpTailJ[j] * px + zx[j];
    }
}

// passes 2 / 4: carry[0] = seed, carry[i + 1] = A carry[i] + z[i] for i < nz (NCH channels; z[i * zs + ch], seed[ch * sstride]).  1024 lanes, a run of
// segments each, and a scan of the runs' affine maps (P, b) across the lanes.
template <int NCH>
__global__ __launch_bounds__(kIqdScan) void iqd_carry_scan_kernel(const double* __restrict__ z, int zs, long nz, double A, const double* __restrict__ seed, int sstride,
                                                                  double* __restrict__ carry) {
    __shared__ double sp[kIqdScan], sb[NCH][kIqdScan];
    const int  u   = threadIdx.x;
    const long per = (nz + kIqdScan - 1) / kIqdScan;
    const long i0 = min(nz, (long)u * per), i1 = min(nz, i0 + per);
    double     P = 1.0, b[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) b[ch] = 0.0;
    for (long i = i0; i < i1; ++i) {
        P *= A;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) b[ch] = A * b[ch] + z[i * zs + ch];
    }
    sp[u] = P;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) sb[ch][u] = b[ch];
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < kIqdScan; off <<= 1) { // (P, b) after (Pp, bp): x -> P (Pp x + bp) + b
        double qp = P, qb[NCH];
        if (u >= off) {
            qp = P * sp[u - off];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) qb[ch] = P * sb[ch][u - off] + b[ch];
        }
        __syncthreads();
        if (u >= off) {
            P     = qp;
            sp[u] = P;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                b[ch]     = qb[ch];
                sb[ch][u] = b[ch];
            }
        }
        __syncthreads();
    }
    double cv[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) cv[ch] = u == 0 ? seed[ch * sstride] : sp[u - 1] * seed[ch * sstride] + sb[ch][u - 1];
    if (u == 0) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) carry[ch] = cv[ch];
    }
    for (long i = i0; i < i1; ++i) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            cv[ch]                    = A * cv[ch] + z[i * zs + ch];
            carry[(i + 1) * NCH + ch] = cv[ch];
        }
    }
}

// pass 3: per segment, every lane's zero-state low-pass end (lz[ch * nl + lane]) and the segment's (lpz[s * 5 + ch])
template <typename T, int M>
__global__ __launch_bounds__(kIqdLanes) void iqd_mix_kernel(const T* __restrict__ r, const T* __restrict__ x, long n, bool vec, long seen, const double* __restrict__ st,
                                                            IqdCoef c, const double* __restrict__ hpz, const double* __restrict__ chp, double* __restrict__ lz, long nl,
                                                            double* __restrict__ lpz) {
    __shared__ double sh[5][kIqdLanes], tl[9][kIqdLanes];
    const int  t  = threadIdx.x;
    const long s  = blockIdx.x;
    const long p0 = s * kIqdS + (long)t * kIqdJ;
    const int  m  = iqd_lane_count(p0, n);
    double     hr[7], hx[4], vr, vx;
    iqd_hp_start(r, x, s, p0, m, n, vec, st, c, hpz, chp, sh, tl, hr, hx, vr, vx);
    double sl[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    iqd_true_run<T, M, false>(r, x, p0, m, n, vec, seen, c, hr, hx, vr, vx, sl, 1, nullptr, nullptr, nullptr);
#pragma unroll
    for (int ch = 0; ch < 5; ++ch) lz[ch * nl + s * kIqdLanes + t] = sl[ch];
    iqd_block_scan<5>(sh, sl, c.lpJ);
    if (t == kIqdLanes - 1) {
#pragma unroll
        for (int ch = 0; ch < 5; ++ch) lpz[s * 5 + ch] = sl[ch];
    }
}

// pass 5: per segment, the outputs of every chunk that ends in it; the lane with the call's last sample writes the handle's next state stn
template <typename T, int M>
__global__ __launch_bounds__(kIqdLanes) void iqd_out_kernel(const T* __restrict__ r, const T* __restrict__ x, long n, bool vec, long seen, const double* __restrict__ st,
                                                            IqdCoef c, const double* __restrict__ hpz, const double* __restrict__ chp, const double* __restrict__ lz, long nl,
                                                            const double* __restrict__ clp, long C, T* __restrict__ amp, T* __restrict__ ph, T* __restrict__ fr,
                                                            double* __restrict__ stn) {
    __shared__ double sh[5][kIqdLanes], tl[9][kIqdLanes];
    const int  t  = threadIdx.x;
    const long s  = blockIdx.x;
    const long p0 = s * kIqdS + (long)t * kIqdJ;
    const int  m  = iqd_lane_count(p0, n);
    double     hr[7], hx[4], vr, vx;
    iqd_hp_start(r, x, s, p0, m, n, vec, st, c, hpz, chp, sh, tl, hr, hx, vr, vx);
    double sl[5];
#pragma unroll
    for (int ch = 0; ch < 5; ++ch) sl[ch] = lz[ch * nl + s * kIqdLanes + t] + (t == 0 ? c.lpJ[0] * clp[s * 5 + ch] : 0.0);
    iqd_block_scan<5>(sh, sl, c.lpJ);
#pragma unroll
    for (int ch = 0; ch < 5; ++ch) sl[ch] = t ? sh[ch][t - 1] : clp[s * 5 + ch];
    iqd_true_run<T, M, true>(r, x, p0, m, n, vec, seen, c, hr, hx, vr, vx, sl, C, amp, ph, fr);
    if (m > 0 && p0 + m == n) {
#pragma unroll
        for (int j = 0; j < 6; ++j) stn[j] = hr[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) stn[6 + j] = hx[j];
        stn[9]  = vr;
        stn[10] = vx;
#pragma unroll
        for (int ch = 0; ch < 5; ++ch) stn[11 + ch] = sl[ch];
    }
}

__global__ void iqd_zero_state_kernel(double* st) {
    if (threadIdx.x < kIqdState) st[threadIdx.x] = 0.0;
}

// ------------------------------------------------------------------------------------------------ host side
static int iqd_check(int dtype, const gr4hip_iqdemod_params* p) {
    GR4_REQUIRE(p, "iqdemod: null params");
    GR4_REQUIRE(dtype == GR4HIP_F32 || dtype == GR4HIP_F64, "iqdemod: dtype %d (GR4HIP_F32 or GR4HIP_F64)", dtype);
    const float fs = p->sample_rate, fhp = p->f_high_pass, flp = p->f_low_pass;
    GR4_REQUIRE(std::isfinite(fs) && std::isfinite(fhp) && std::isfinite(flp) && std::isfinite(p->epsilon) && (dtype == GR4HIP_F64 || std::isfinite((float)p->epsilon)),
                "iqdemod: non-finite setting");
    GR4_REQUIRE(fs > 0.f, "iqdemod: sample_rate %g <= 0", (double)fs);
    // settingsChanged (:461-462), in float
    GR4_REQUIRE(!(fhp <= 0.f || flp <= 0.f || fhp >= flp || flp >= fs / 2.f), "invalid filter frequencies: 0 < f_hp(%g) < f_lp(%g) < fs/2(%g)", (double)fhp, (double)flp,
                (double)(fs / 2.f));
    GR4_REQUIRE(p->derivative_method >= 0 && p->derivative_method <= 2, "iqdemod: unknown derivative_method %d", p->derivative_method);
    GR4_REQUIRE(p->phase_unit == 0 || p->phase_unit == 1, "iqdemod: unknown phase_unit %d", p->phase_unit);
    GR4_REQUIRE(p->chunk >= 1, "iqdemod: chunk == 0");
    return GR4HIP_OK;
}

// initialiseFilters (:468-506) in T, widened; the rest of the extraction's constants as the reference writes them in T
template <typename T>
static IqdCoef iqd_coef(const gr4hip_iqdemod_params& p) {
    const T pi  = (T)3.14159265358979323846264338327950288; // std::numbers::pi_v<T>
    const T fs  = static_cast<T>(p.sample_rate);
    const T ahp = std::exp(T(-2) * pi * static_cast<T>(p.f_high_pass) / fs);
    const T alp = T(1) - std::exp(T(-2) * pi * static_cast<T>(p.f_low_pass) / fs);
    IqdCoef c{};
    c.ahp = (double)ahp;
    c.alp = (double)alp;
    const T   t0[3] = {T(1), T(0), T(-1)};
    const T   t1[5] = {T(0.2), T(0.1), T(0), T(-0.1), T(-0.2)};
    const T   t2[7] = {T(3) / T(28), T(2) / T(28), T(1) / T(28), T(0), T(-1) / T(28), T(-2) / T(28), T(-3) / T(28)};
    const T*  tp    = p.derivative_method == 0 ? t0 : p.derivative_method == 1 ? t1 : t2;
    const int K     = p.derivative_method == 0 ? 3 : p.derivative_method == 1 ? 5 : 7;
    for (int k = 0; k < 7; ++k) c.tap[k] = k < K ? (double)tp[k] : 0.0;
    const double mlp = 1.0 - c.alp;
    for (int k = 0; k < 8; ++k) {
        c.hpJ[k] = std::pow(c.ahp, (double)(kIqdJ << k));
        c.lpJ[k] = std::pow(mlp, (double)(kIqdJ << k));
    }
    for (int j = 0; j < 6; ++j) {
        c.hpTailJ[j] = std::pow(c.ahp, (double)(kIqdJ - j));
        c.hpTailS[j] = std::pow(c.ahp, (double)(kIqdS - j));
    }
    c.lpS     = std::pow(mlp, (double)kIqdS);
    c.eps     = (double)static_cast<T>(p.epsilon);
    c.fs      = (double)fs;
    c.g0      = p.derivative_method == 0 ? 2.0 : 1.0;
    c.g08     = (double)T(0.8);
    c.g02     = (double)T(0.2);
    c.pi      = (double)pi;
    c.degrees = p.phase_unit == 1;
    c.invert  = p.invert_phase != 0;
    return c;
}

} // namespace gr4

using namespace gr4;

struct gr4hip_iqdemod {
    int                   dtype = GR4HIP_F32;
    gr4hip_iqdemod_params p{};
    IqdCoef               c{};
    long long             seen         = 0;    // samples since the last re-initialisation (saturates): host-side, exact
    bool                  init_pending = true; // the state to be zeroed in front of the next launch, on its stream
    int                   cur          = 0;    // which state buffer holds the state
    DeviceBuffer          d_state[2], d_hpz, d_chp, d_lz, d_lpz, d_clp;
};

static void iqd_apply(gr4hip_iqdemod_t* h, const gr4hip_iqdemod_params& p, bool reinitialise) {
    h->p = p;
    h->c = h->dtype == GR4HIP_F32 ? iqd_coef<float>(p) : iqd_coef<double>(p);
    if (reinitialise) {
        h->seen         = 0;
        h->init_pending = true;
    }
}

template <typename T, int M>
static int iqd_launch(gr4hip_iqdemod_t* h, const T* r, const T* x, long n, T* amp, T* ph, T* fr, hipStream_t st) {
    const long     nseg = (long)ceil_div((size_t)n, (size_t)kIqdS), nl = nseg * kIqdLanes;
    const bool     vec  = ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
    const double*  s0   = (const double*)h->d_state[h->cur].ptr;
    double*        s1   = (double*)h->d_state[h->cur ^ 1].ptr;
    double*        hpz  = (double*)h->d_hpz.ptr;
    double*        chp  = (double*)h->d_chp.ptr;
    double*        lz   = (double*)h->d_lz.ptr;
    double*        lpz  = (double*)h->d_lpz.ptr;
    double*        clp  = (double*)h->d_clp.ptr;
    const IqdCoef& c    = h->c;
    const long     seen = (long)h->seen;
    if (nseg > 1) {
        hipLaunchKernelGGL(iqd_hp_reduce_kernel<T>, dim3((unsigned)(nseg - 1)), dim3(kIqdLanes), 0, st, r, x, n, vec, s0, c, hpz);
        GR4_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(iqd_carry_scan_kernel<2>, dim3(1), dim3(kIqdScan), 0, st, (const double*)hpz, 9, nseg - 1, c.hpTailS[0], s0, 6, chp);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL((iqd_mix_kernel<T, M>), dim3((unsigned)nseg), dim3(kIqdLanes), 0, st, r, x, n, vec, seen, s0, c, (const double*)hpz, (const double*)chp, lz, nl,
                       lpz);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL(iqd_carry_scan_kernel<5>, dim3(1), dim3(kIqdScan), 0, st, (const double*)lpz, 5, nseg - 1, c.lpS, s0 + 11, 1, clp);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL((iqd_out_kernel<T, M>), dim3((unsigned)nseg), dim3(kIqdLanes), 0, st, r, x, n, vec, seen, s0, c, (const double*)hpz, (const double*)chp,
                       (const double*)lz, nl, (const double*)clp, (long)h->p.chunk, amp, ph, fr, s1);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

template <typename T>
static int iqd_dispatch(gr4hip_iqdemod_t* h, const void* r, const void* x, long n, void* amp, void* ph, void* fr, hipStream_t st) {
    const T* rt = (const T*)r;
    const T* xt = (const T*)x;
    T*       at = (T*)amp;
    T*       pt = (T*)ph;
    T*       ft = (T*)fr;
    switch (h->p.derivative_method) {
    case 0: return iqd_launch<T, 0>(h, rt, xt, n, at, pt, ft, st);
    case 1: return iqd_launch<T, 1>(h, rt, xt, n, at, pt, ft, st);
    default: return iqd_launch<T, 2>(h, rt, xt, n, at, pt, ft, st);
    }
}

extern "C" {

int gr4hip_iqdemod_params_default(gr4hip_iqdemod_params* p) {
    GR4_REQUIRE(p, "iqdemod: null params");
    *p = gr4hip_iqdemod_params{62.5e6f, 100.f, 10000.f, 0, 0, 0, 1e-12, 1024}; // (:423-429), Resampling<1024U, 1U, false>
    return GR4HIP_OK;
}

int gr4hip_iqdemod_check(int dtype, const gr4hip_iqdemod_params* p) { return iqd_check(dtype, p); }

int gr4hip_iqdemod_create(gr4hip_iqdemod_t** out, int dtype, const gr4hip_iqdemod_params* p) {
    GR4_REQUIRE(out, "iqdemod: null output handle");
    int rc = iqd_check(dtype, p); // (validated before anything is allocated)
    if (rc) return rc;
    auto* h = new (std::nothrow) gr4hip_iqdemod();
    GR4_REQUIRE(h, "out of host memory");
    h->dtype = dtype;
    iqd_apply(h, *p, true);
    for (auto& b : h->d_state)
        if (!rc) rc = b.ensure(kIqdState * sizeof(double));
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return GR4HIP_OK;
}

int gr4hip_iqdemod_set_params(gr4hip_iqdemod_t* h, const gr4hip_iqdemod_params* p, int reinitialise) {
    GR4_REQUIRE(h, "iqdemod: null handle");
    const int rc = iqd_check(h->dtype, p);
    if (rc) return rc;
    if (!reinitialise) // the filters keep their coefficients and state: their settings must be the ones they were made from
        GR4_REQUIRE(p->sample_rate == h->p.sample_rate && p->f_high_pass == h->p.f_high_pass && p->f_low_pass == h->p.f_low_pass &&
                        p->derivative_method == h->p.derivative_method,
                    "iqdemod: a change of sample_rate, f_high_pass, f_low_pass or derivative_method re-initialises the filters (reinitialise = 1)");
    iqd_apply(h, *p, reinitialise != 0);
    return GR4HIP_OK;
}

int gr4hip_iqdemod_reset(gr4hip_iqdemod_t* h) {
    GR4_REQUIRE(h, "iqdemod: null handle");
    h->seen         = 0;
    h->init_pending = true;
    return GR4HIP_OK;
}

int gr4hip_iqdemod_destroy(gr4hip_iqdemod_t* h) {
    delete h;
    return GR4HIP_OK;
}

int gr4hip_iqdemod_process(gr4hip_iqdemod_t* h, const void* d_ref, const void* d_resp, size_t n_in, void* d_amp, void* d_phase, void* d_freq, size_t* n_out,
                           gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "iqdemod: null handle");
    const size_t C = h->p.chunk;
    GR4_REQUIRE(n_in % C == 0, "iqdemod: n_in %zu is not a multiple of the chunk %zu", n_in, C);
    GR4_REQUIRE(n_in < ((size_t)1 << 40), "iqdemod: n_in %zu too large", n_in);
    const size_t no = n_in / C;
    if (n_out) *n_out = no;
    if (n_in == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_ref && d_resp && d_amp && d_phase && d_freq, "iqdemod: null device pointer");
    hipStream_t  st   = as_stream(stream);
    const size_t nseg = ceil_div(n_in, (size_t)kIqdS);
    int          rc;
    // scratch sized for this call (a replaced buffer is fresh: hipFree waited for the device), then the pending re-initialisation, on this stream
    if ((rc = h->d_hpz.ensure(nseg * 9 * sizeof(double))) || (rc = h->d_chp.ensure(nseg * 2 * sizeof(double))) ||
        (rc = h->d_lz.ensure(nseg * kIqdLanes * 5 * sizeof(double))) || (rc = h->d_lpz.ensure(nseg * 5 * sizeof(double))) ||
        (rc = h->d_clp.ensure(nseg * 5 * sizeof(double))))
        return rc;
    if (h->init_pending) {
        hipLaunchKernelGGL(iqd_zero_state_kernel, dim3(1), dim3(64), 0, st, (double*)h->d_state[h->cur].ptr);
        GR4_LAUNCH_CHECK();
        h->init_pending = false;
    }
    rc = h->dtype == GR4HIP_F32 ? iqd_dispatch<float>(h, d_ref, d_resp, (long)n_in, d_amp, d_phase, d_freq, st)
                                : iqd_dispatch<double>(h, d_ref, d_resp, (long)n_in, d_amp, d_phase, d_freq, st);
    if (rc) return rc;
    h->cur ^= 1;
    h->seen = std::min<long long>(h->seen + (long long)n_in, 1ll << 40);
    return GR4HIP_OK;
}

} // extern "C"
