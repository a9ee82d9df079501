// power_metrics.hip -- gr::electrical::PowerMetrics<float, nPhases> (blocks/electrical/.../PowerEstimators.hpp:21-131): per phase, active, reactive and apparent
// power and the two RMS values of a voltage / current pair.
//
// Per sample and phase the block runs a Butterworth high-pass biquad on each input, forms u i, u u and i i, runs a Butterworth low-pass biquad on each product and,
// at the first sample of every chunk of `decimate` inputs, reads P, Q, S, U_rms and I_rms off the low-pass outputs (include/gr4hip.h "Power metrics",
// POWER_METRICS.md).  The coefficients are the library's float design (gr4hip_iir_design, pinned to the reference's), widened; every state, product and the final
// step are float64; the outputs are rounded to float once.  A biquad in direct form II, state c = (w[n-1], w[n-2]), is linear with constant coefficients:
// a lane's run of J samples maps c to M^J c + z (z: the run from zero state), a segment of S = 256 J samples to M^S c + z, with M = [[-a1, -a2], [1, 0]] and its
// powers from the host.  Carries are exact: no warm-up, no look-back window.  A call is up to five launches on its stream, phases in blockIdx.y:
//   pm_segment_kernel<.., 0>  per segment but the last: the zero-state high-pass end states of both inputs;
//   pm_carry_walk_kernel<2>   the two high-pass states in front of every segment, seeded from the handle: a workgroup per phase, every lane walking a run of
//                             32 segments in order, one lane per filter walking the runs' ends in order;
//   pm_segment_kernel<.., 1>  per segment but the last: lane carries by an in-block scan, the true high-pass, the products, the zero-state low-pass end states;
//   pm_carry_walk_kernel<3>   the three low-pass states in front of every segment;
//   pm_segment_kernel<.., 2>  per segment: the same again (the high-passed pairs kept in registers), the low-passes from their true lane carries, the outputs at
//                             every chunk start, the handle's next state.
// Every pass loads its segment with coalesced 16-byte loads into LDS, rows of J floats padded to J + 1 so that the lanes' runs read it free of bank conflicts.
// A non-finite input poisons the states it reaches, as in the reference: a lane or segment that starts behind a non-finite carry starts from NaN.
#include "common.hpp"

#include <cmath>

namespace gr4 {

constexpr int  kPmLanes = 256;
constexpr int  kPmJ     = 16;                      // samples per lane
constexpr int  kPmPad   = kPmJ + 1;                // floats per lane row in LDS
constexpr long kPmS     = (long)kPmLanes * kPmJ;   // samples per segment (one workgroup): GR4HIP_POWERMETRICS_SEGMENT
constexpr int  kPmRun   = 32;                      // segments per run of the carry walk
constexpr int  kPmState = 10;                      // doubles of a phase's state: (w1, w2) of hp(u), hp(i), lp(u i), lp(u u), lp(i i)
static_assert(kPmS == GR4HIP_POWERMETRICS_SEGMENT, "the exported segment length");

struct PmCoef {
    double hb[3], ha[2]; // high-pass b0..b2, a1, a2
    double lb[3], la[2]; // low-pass
    double hJ[8][4];     // M_hp^(J 2^k), row-major
    double lJ[8][4];     // M_lp^(J 2^k)
    double hS[4], lS[4]; // M^S
    double hR[4], lR[4]; // M^(S R), R = kPmRun segments (the carry walk's runs)
};

struct PmArgs {
    const float* u;
    const float* i;
    long         in_stride, n, nseg;
    int          vec;
    const double* st;  // [phase][kPmState]
    double*       stn; // the next state (pass 2)
    double*       hpz; // [phase][nseg][4]
    double*       chp;
    double*       lpz; // [phase][nseg][6]
    double*       clp;
    long          D;
    float*        out[5]; // P, Q, S, U_rms, I_rms (any may be null)
    long          out_stride;
    PmCoef        c;
};

__device__ __forceinline__ bool pm_bad(double a, double b) { return !(isfinite(a) && isfinite(b)); }

// one direct-form-II step (FilterTool.hpp:130-136): w = x - (a1 w1 + a2 w2), y = b0 w + b1 w1 + b2 w2
__device__ __forceinline__ double pm_step(double x, const double b[3], const double a[2], double& w1, double& w2) {
    const double w = x - (a[0] * w1 + a[1] * w2);
    const double y = b[0] * w + b[1] * w1 + b[2] * w2;
    w2 = w1;
    w1 = w;
    return y;
}

__device__ __forceinline__ void pm_step_state(double x, const double a[2], double& w1, double& w2) {
    const double w = x - (a[0] * w1 + a[1] * w2);
    w2 = w1;
    w1 = w;
}

// the segment's samples of both inputs into LDS: lane t loads 16 bytes at 4 t of every 1024-sample slab (one 1 KiB line run per wave-instruction)
__device__ __forceinline__ void pm_stage(const float* __restrict__ u, const float* __restrict__ i, long seg0, long n, bool vec, float* __restrict__ su,
                                         float* __restrict__ si) {
    float4 qu[kPmJ / 4], qi[kPmJ / 4];
#pragma unroll
    for (int it = 0; it < kPmJ / 4; ++it) {
        const long p = seg0 + it * (kPmLanes * 4) + threadIdx.x * 4;
        if (vec && p + 4 <= n) {
            qu[it] = *reinterpret_cast<const float4*>(u + p);
            qi[it] = *reinterpret_cast<const float4*>(i + p);
        } else {
            qu[it] = make_float4(p < n ? u[p] : 0.f, p + 1 < n ? u[p + 1] : 0.f, p + 2 < n ? u[p + 2] : 0.f, p + 3 < n ? u[p + 3] : 0.f);
            qi[it] = make_float4(p < n ? i[p] : 0.f, p + 1 < n ? i[p + 1] : 0.f, p + 2 < n ? i[p + 2] : 0.f, p + 3 < n ? i[p + 3] : 0.f);
        }
    }
#pragma unroll
    for (int it = 0; it < kPmJ / 4; ++it) {
        const int e = it * (kPmLanes * 4) + threadIdx.x * 4;
        float*    du = su + e + e / kPmJ;
        float*    di = si + e + e / kPmJ;
        du[0] = qu[it].x; du[1] = qu[it].y; du[2] = qu[it].z; du[3] = qu[it].w;
        di[0] = qi[it].x; di[1] = qi[it].y; di[2] = qi[it].z; di[3] = qi[it].w;
    }
}

// inclusive scan over the block's lanes of  v <- M^J v_prev + v  for NF filters of two state values each (pw[k] = M^(J 2^k)); sh is [2 NF][256]
template <int NF>
__device__ __forceinline__ void pm_block_scan(double (*sh)[kPmLanes], double v[2 * NF], const double (&pw)[8][4]) {
    const int t = threadIdx.x;
    __syncthreads(); // (sh may still be read by an earlier use)
#pragma unroll
    for (int ch = 0; ch < 2 * NF; ++ch) sh[ch][t] = v[ch];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int off = 1 << k;
        double    q[2 * NF];
        if (t >= off) {
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const double x0 = sh[2 * f][t - off], x1 = sh[2 * f + 1][t - off];
                q[2 * f]     = pw[k][0] * x0 + pw[k][1] * x1;
                q[2 * f + 1] = pw[k][2] * x0 + pw[k][3] * x1;
            }
        }
        __syncthreads();
        if (t >= off) {
#pragma unroll
            for (int ch = 0; ch < 2 * NF; ++ch) { v[ch] += q[ch]; sh[ch][t] = v[ch]; }
        }
        __syncthreads();
    }
}

// This lane's start states after pm_block_scan: the lane before's end (lane 0: the segment's carry).  A lane whose predecessor already started from a
// non-finite state lies at least J samples behind the non-finite input: the reference's states are all NaN there, whatever the scan's products give.
template <int NF>
__device__ __forceinline__ void pm_lane_start(double (*sh)[kPmLanes], const double* __restrict__ carry, double out[2 * NF]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        double a0 = t ? sh[2 * f][t - 1] : carry[2 * f], a1 = t ? sh[2 * f + 1][t - 1] : carry[2 * f + 1];
        if (t > 0) {
            const double b0 = t > 1 ? sh[2 * f][t - 2] : carry[2 * f], b1 = t > 1 ? sh[2 * f + 1][t - 2] : carry[2 * f + 1];
            if (pm_bad(b0, b1)) a0 = a1 = __builtin_nan("");
        }
        out[2 * f]     = a0;
        out[2 * f + 1] = a1;
    }
}

// lane 0 adds M^J carry to its zero-state end: the scan is then seeded with the segment's carry
template <int NF>
__device__ __forceinline__ void pm_seed(double v[2 * NF], const double* __restrict__ carry, const double (&pw)[8][4]) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const double c0 = carry[2 * f], c1 = carry[2 * f + 1];
            v[2 * f] += pw[0][0] * c0 + pw[0][1] * c1;
            v[2 * f + 1] += pw[0][2] * c0 + pw[0][3] * c1;
        }
    }
}

// MODE 0: zero-state high-pass ends -> hpz;  1: zero-state low-pass ends -> lpz;  2: outputs and the next state.  HPI: high_pass <= 0, the identity (:73).
template <bool HPI, int MODE>
__global__ __launch_bounds__(kPmLanes) void pm_segment_kernel(const PmArgs a) {
    __shared__ float  su[kPmLanes * kPmPad], si[kPmLanes * kPmPad];
    __shared__ double sh[6][kPmLanes];
    const int    t  = threadIdx.x;
    const long   s  = blockIdx.x;
    const long   ph = blockIdx.y;
    const PmCoef& c = a.c;
    pm_stage(a.u + ph * a.in_stride, a.i + ph * a.in_stride, s * kPmS, a.n, a.vec != 0, su, si);
    __syncthreads();
    const long   p0 = s * kPmS + (long)t * kPmJ;
    const int    m  = p0 >= a.n ? 0 : (int)min((long)kPmJ, a.n - p0);
    const float* lu = su + t * kPmPad;
    const float* li = si + t * kPmPad;

    double hs[4] = {0.0, 0.0, 0.0, 0.0}; // the true high-pass states at the lane's start
    if constexpr (!HPI) {
        double z[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kPmJ; ++k) {
            if (k < m) {
                pm_step_state((double)lu[k], c.ha, z[0], z[1]);
                pm_step_state((double)li[k], c.ha, z[2], z[3]);
            }
        }
        if constexpr (MODE == 0) {
            pm_block_scan<2>(sh, z, c.hJ);
            if (t == kPmLanes - 1) {
                double* o = a.hpz + (ph * a.nseg + s) * 4;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) o[ch] = z[ch];
            }
            return;
        } else {
            const double* carry = a.chp + (ph * a.nseg + s) * 4;
            pm_seed<2>(z, carry, c.hJ);
            pm_block_scan<2>(sh, z, c.hJ);
            pm_lane_start<2>(sh, carry, hs);
        }
    }
    if constexpr (MODE != 0) {
        // the true high-pass, the products, the zero-state low-passes
        double uh[MODE == 2 ? kPmJ : 1], ih[MODE == 2 ? kPmJ : 1];
        double lz[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kPmJ; ++k) {
            if (k < m) {
                double x = (double)lu[k], y = (double)li[k];
                if constexpr (!HPI) {
                    x = pm_step(x, c.hb, c.ha, hs[0], hs[1]);
                    y = pm_step(y, c.hb, c.ha, hs[2], hs[3]);
                }
                if constexpr (MODE == 2) {
                    uh[k] = x;
                    ih[k] = y;
                }
                pm_step_state(x * y, c.la, lz[0], lz[1]);
                pm_step_state(x * x, c.la, lz[2], lz[3]);
                pm_step_state(y * y, c.la, lz[4], lz[5]);
            }
        }
        if constexpr (MODE == 1) {
            pm_block_scan<3>(sh, lz, c.lJ);
            if (t == kPmLanes - 1) {
                double* o = a.lpz + (ph * a.nseg + s) * 6;
#pragma unroll
                for (int ch = 0; ch < 6; ++ch) o[ch] = lz[ch];
            }
        } else {
            const double* carry = a.clp + (ph * a.nseg + s) * 6;
            double        ls[6];
            pm_seed<3>(lz, carry, c.lJ);
            pm_block_scan<3>(sh, lz, c.lJ);
            pm_lane_start<3>(sh, carry, ls);
            long j = (p0 + a.D - 1) / a.D, e = j * a.D; // the next chunk start at or behind p0 (:111)
#pragma unroll
            for (int k = 0; k < kPmJ; ++k) {
                if (k < m) {
                    const double x = uh[k], y = ih[k];
                    const double ep = pm_step(x * y, c.lb, c.la, ls[0], ls[1]);
                    const double eu = pm_step(x * x, c.lb, c.la, ls[2], ls[3]);
                    const double ei = pm_step(y * y, c.lb, c.la, ls[4], ls[5]);
                    if (p0 + k == e) {
                        const double ur = sqrt(eu), ir = sqrt(ei), S = ur * ir; // (:113-116) sqrt of a negative average: NaN
                        const double d  = S * S - ep * ep;
                        const double Q  = sqrt(d < 0.0 ? 0.0 : d); // std::max(d, T(0)): NaN stays NaN (:117)
                        const long   o  = ph * a.out_stride + j;
                        if (a.out[0]) a.out[0][o] = (float)ep;
                        if (a.out[1]) a.out[1][o] = (float)Q;
                        if (a.out[2]) a.out[2][o] = (float)S;
                        if (a.out[3]) a.out[3][o] = (float)ur;
                        if (a.out[4]) a.out[4][o] = (float)ir;
                        ++j;
                        e += a.D;
                    }
                }
            }
            if (m > 0 && p0 + m == a.n) {
                double* o = a.stn + ph * kPmState;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) o[ch] = hs[ch];
#pragma unroll
                for (int ch = 0; ch < 6; ++ch) o[4 + ch] = ls[ch];
            }
        }
    }
}

// passes 2 / 4: carry[0] = the handle's state, carry[s + 1] = M^S carry[s] + z[s] for s < nseg - 1, on two levels.  One workgroup per phase takes kPmLanes
// runs of kPmRun segments at a time: every lane walks its run in order from zero state, one lane per filter walks the runs' ends in order with M^(S R) (which
// leaves every run's start state), and every lane walks its run again from that start and stores the carries.  Everything is composed in order and nothing is
// scanned with M^(S 2^k): where the float design puts a pole at z = 1 the state c grows with every sample of a DC offset while M^k tends to a projection
// with entries of 1 / (1 - second pole), 6e4 at 2 Hz / 1 MHz, so that a product M^k c is off by eps |M^k| |c|.  M^(S R) is applied once per run, where the
// R steps of a walk would each leave eps |M^S| |c|.  z is 32 or 48 bytes per segment and is read from the cache, four segments per round trip.
struct PmWalk {
    double s[4], r[4]; // M^S, M^(S R)
};

// cnt <= kPmRun steps c <- M^S c + z[q] for NF filters; STORE: c goes to out[q] after every step
template <int NF, bool STORE>
__device__ __forceinline__ void pm_walk_run(const double* __restrict__ zr, int cnt, const double (&m)[4], double c[2 * NF], double* __restrict__ out) {
    constexpr int CH = 2 * NF;
    for (int q0 = 0; q0 < cnt; q0 += 4) {
        double zq[4][CH];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q0 + q < cnt) {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) zq[q][ch] = zr[(q0 + q) * CH + ch];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q0 + q < cnt) {
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    const double c0 = c[2 * f], c1 = c[2 * f + 1];
                    double       n0 = m[0] * c0 + m[1] * c1 + zq[q][2 * f], n1 = m[2] * c0 + m[3] * c1 + zq[q][2 * f + 1];
                    if (pm_bad(c0, c1)) n0 = n1 = __builtin_nan(""); // a whole segment behind a non-finite state
                    c[2 * f]     = n0;
                    c[2 * f + 1] = n1;
                    if constexpr (STORE) {
                        out[(q0 + q) * CH + 2 * f]     = n0;
                        out[(q0 + q) * CH + 2 * f + 1] = n1;
                    }
                }
            }
        }
    }
}

template <int NF>
__global__ __launch_bounds__(kPmLanes) void pm_carry_walk_kernel(const double* __restrict__ z, long nseg, const double* __restrict__ st, int st_off, const PmWalk w,
                                                                  double* __restrict__ carry) {
    constexpr int CH = 2 * NF;
    __shared__ double sh[CH][kPmLanes]; // the runs' zero-state ends, then their start states
    __shared__ double sg[CH];           // the state in front of the group of runs
    const int     t  = threadIdx.x;
    const long    ph = blockIdx.x;
    const double* zp = z + ph * nseg * CH;
    double*       cp = carry + ph * nseg * CH;
    const long    nz = nseg - 1;
    if (t < CH) {
        const double c = st[ph * kPmState + st_off + t];
        sg[t] = c;
        cp[t] = c;
    }
    for (long base = 0; base < nz; base += (long)kPmLanes * kPmRun) {
        const long b0  = base + (long)t * kPmRun;
        const int  cnt = b0 >= nz ? 0 : (int)min((long)kPmRun, nz - b0);
        double     c[CH];
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) c[ch] = 0.0;
        pm_walk_run<NF, false>(zp + b0 * CH, cnt, w.s, c, nullptr);
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) sh[ch][t] = c[ch];
        __syncthreads();
        if (t < NF) { // (only the call's last run can be short, and nothing follows it)
            const int runs = (int)min((long)kPmLanes, (nz - base + kPmRun - 1) / kPmRun);
            double    c0 = sg[2 * t], c1 = sg[2 * t + 1];
            for (int r = 0; r < runs; ++r) {
                const double e0 = sh[2 * t][r], e1 = sh[2 * t + 1][r];
                sh[2 * t][r]     = c0;
                sh[2 * t + 1][r] = c1;
                double n0 = w.r[0] * c0 + w.r[1] * c1 + e0, n1 = w.r[2] * c0 + w.r[3] * c1 + e1;
                if (pm_bad(c0, c1)) n0 = n1 = __builtin_nan("");
                c0 = n0;
                c1 = n1;
            }
            sg[2 * t]     = c0;
            sg[2 * t + 1] = c1;
        }
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) c[ch] = sh[ch][t];
        pm_walk_run<NF, true>(zp + b0 * CH, cnt, w.s, c, cp + (b0 + 1) * CH);
        __syncthreads(); // (sh is written again)
    }
}

__global__ void pm_zero_state_kernel(double* st, int count) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) st[k] = 0.0;
}

// ------------------------------------------------------------------------------------------------ host side
// M^(J 2^k), k < 8, M^S and M^(S R) of M = [[-a1, -a2], [1, 0]].  M^k = [[h[k], -a2 h[k-1]], [h[k-1], -a2 h[k-2]]] with h the impulse response of 1 / A(z)
// (h[-1] = 0, h[0] = 1), run in long double: repeated squaring loses a factor 1 / sin(pole angle) (1e3 for 2 Hz at 10 kHz) of relative precision per
// squaring to cancellation, and an error of M^k times a direct-form-II state of 1e5 times the signal shows in the outputs where they ring through zero.
static void pm_powers(const double a[2], double pJ[8][4], double pS[4], double pR[4]) {
    const long double a1 = a[0], a2 = a[1];
    long double       h2 = 0.0L, h1 = 0.0L, h0 = 1.0L; // h[k-2], h[k-1], h[k] at k = 0
    int               next = 0;
    for (long k = 1; k <= kPmS * kPmRun; ++k) {
        const long double h = -a1 * h0 - a2 * h1;
        h2 = h1;
        h1 = h0;
        h0 = h;
        double* o = nullptr;
        if (next < 8 && k == ((long)kPmJ << next)) o = pJ[next++];
        if (k == kPmS) o = pS;
        if (k == kPmS * kPmRun) o = pR;
        if (o) {
            o[0] = (double)h0;
            o[1] = (double)(-a2 * h1);
            o[2] = (double)h1;
            o[3] = (double)(-a2 * h2);
        }
    }
}

// one second-order Butterworth section as iir::designFilter<float> gives it (:69-71, :85-87), widened
static int pm_biquad(int response, double f, double fs, double b[3], double a[2]) {
    gr4hip_filter_params fp;
    gr4hip_filter_params_default(&fp);
    fp.order = 2;
    fp.fs    = fs;
    (response == GR4HIP_HIGHPASS ? fp.f_high : fp.f_low) = f;
    float  hb[6], ha[6];
    size_t ns = 0;
    const int rc = gr4hip_iir_design(response, &fp, GR4HIP_BUTTERWORTH, hb, ha, 2, &ns);
    if (rc) return GR4HIP_INVALID_ARGUMENT;
    GR4_REQUIRE(ns == 1, "powermetrics: the %s design at %g Hz / %g Hz is not one biquad", response == GR4HIP_HIGHPASS ? "high-pass" : "low-pass", f, fs);
    for (int k = 0; k < 3; ++k) b[k] = (double)hb[k];
    a[0] = (double)ha[1];
    a[1] = (double)ha[2];
    GR4_REQUIRE(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2]),
                "powermetrics: non-finite %s coefficients", response == GR4HIP_HIGHPASS ? "high-pass" : "low-pass");
    // both roots of z^2 + a1 z + a2 inside or on the unit circle (Jury): a pole outside makes every state grow without bound
    GR4_REQUIRE(a[1] <= 1.0 && std::fabs(a[0]) <= 1.0 + a[1], "powermetrics: the %s design at %g Hz / %g Hz has a pole outside the unit circle (a1 %.9g, a2 %.9g)",
                response == GR4HIP_HIGHPASS ? "high-pass" : "low-pass", f, fs, a[0], a[1]);
    return GR4HIP_OK;
}

static int pm_check(const gr4hip_powermetrics_params* p, PmCoef* out) {
    GR4_REQUIRE(p, "powermetrics: null params");
    const float fs = p->sample_rate, fhp = p->high_pass, flp = p->low_pass;
    GR4_REQUIRE(std::isfinite(fs) && fs > 0.f, "powermetrics: sample_rate %g", (double)fs);
    GR4_REQUIRE(std::isfinite(flp) && flp > 0.f, "powermetrics: low_pass %g", (double)flp);
    GR4_REQUIRE(std::isfinite(fhp) && fhp < fs / 2.f, "powermetrics: high_pass %g (finite, below sample_rate / 2 = %g)", (double)fhp, (double)(fs / 2.f));
    GR4_REQUIRE(p->decimate >= 1, "powermetrics: decimate == 0");
    GR4_REQUIRE(p->n_phases >= 1 && p->n_phases <= 16, "powermetrics: n_phases %zu (1 ... 16)", p->n_phases);
    PmCoef c{};
    int    rc;
    if (fhp > 0.f) { // (:68)
        if ((rc = pm_biquad(GR4HIP_HIGHPASS, (double)fhp, (double)fs, c.hb, c.ha))) return rc;
        pm_powers(c.ha, c.hJ, c.hS, c.hR);
    }
    const double cutoff = std::min(0.5 * ((double)fs / (double)p->decimate), (double)flp); // (:83)
    if ((rc = pm_biquad(GR4HIP_LOWPASS, cutoff, (double)fs, c.lb, c.la))) return rc;
    pm_powers(c.la, c.lJ, c.lS, c.lR);
    if (out) *out = c;
    return GR4HIP_OK;
}

} // namespace gr4

using namespace gr4;

struct gr4hip_powermetrics {
    gr4hip_powermetrics_params p{};
    PmCoef                     c{};
    bool                       init_pending = true; // the state to be zeroed in front of the next launch, on its stream
    int                        cur          = 0;    // which state buffer holds the state
    DeviceBuffer               d_state[2], d_hpz, d_chp, d_lpz, d_clp;
};

static PmWalk pm_walk(const double s[4], const double r[4]) {
    PmWalk w;
    for (int k = 0; k < 4; ++k) {
        w.s[k] = s[k];
        w.r[k] = r[k];
    }
    return w;
}

template <bool HPI>
static int pm_launch(gr4hip_powermetrics_t* h, PmArgs& a, hipStream_t st) {
    const unsigned np = (unsigned)h->p.n_phases;
    const long     nseg = a.nseg;
    const PmCoef&  c    = h->c;
    if constexpr (!HPI) {
        if (nseg > 1) {
            hipLaunchKernelGGL((pm_segment_kernel<HPI, 0>), dim3((unsigned)(nseg - 1), np), dim3(kPmLanes), 0, st, a);
            GR4_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(pm_carry_walk_kernel<2>, dim3(np), dim3(kPmLanes), 0, st, (const double*)a.hpz, nseg, a.st, 0, pm_walk(c.hS, c.hR), a.chp);
        GR4_LAUNCH_CHECK();
    }
    if (nseg > 1) {
        hipLaunchKernelGGL((pm_segment_kernel<HPI, 1>), dim3((unsigned)(nseg - 1), np), dim3(kPmLanes), 0, st, a);
        GR4_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pm_carry_walk_kernel<3>, dim3(np), dim3(kPmLanes), 0, st, (const double*)a.lpz, nseg, a.st, 4, pm_walk(c.lS, c.lR), a.clp);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL((pm_segment_kernel<HPI, 2>), dim3((unsigned)nseg, np), dim3(kPmLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

extern "C" {

int gr4hip_powermetrics_params_default(gr4hip_powermetrics_params* p) {
    GR4_REQUIRE(p, "powermetrics: null params");
    *p = gr4hip_powermetrics_params{10000.f, 2.f, 90.f, 100, 1}; // (:46-49), one phase
    return GR4HIP_OK;
}

size_t gr4hip_powermetrics_segment(void) { return (size_t)kPmS; }

int gr4hip_powermetrics_check(const gr4hip_powermetrics_params* p) { return pm_check(p, nullptr); }

int gr4hip_powermetrics_create(gr4hip_powermetrics_t** out, const gr4hip_powermetrics_params* p) {
    GR4_REQUIRE(out, "powermetrics: null output handle");
    PmCoef c;
    int    rc = pm_check(p, &c); // (validated before anything is allocated)
    if (rc) return rc;
    auto* h = new (std::nothrow) gr4hip_powermetrics();
    GR4_REQUIRE(h, "out of host memory");
    h->p = *p;
    h->c = c;
    for (auto& b : h->d_state)
        if (!rc) rc = b.ensure(p->n_phases * kPmState * sizeof(double));
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return GR4HIP_OK;
}

int gr4hip_powermetrics_set_params(gr4hip_powermetrics_t* h, const gr4hip_powermetrics_params* p) {
    GR4_REQUIRE(h, "powermetrics: null handle");
    PmCoef    c;
    const int rc = pm_check(p, &c);
    if (rc) return rc;
    GR4_REQUIRE(p->n_phases == h->p.n_phases, "powermetrics: n_phases is fixed at create (%zu, not %zu)", h->p.n_phases, p->n_phases);
    h->p            = *p;
    h->c            = c;
    h->init_pending = true; // settingsChanged rebuilds every filter (:95)
    return GR4HIP_OK;
}

int gr4hip_powermetrics_reset(gr4hip_powermetrics_t* h) {
    GR4_REQUIRE(h, "powermetrics: null handle");
    h->init_pending = true;
    return GR4HIP_OK;
}

int gr4hip_powermetrics_destroy(gr4hip_powermetrics_t* h) {
    delete h;
    return GR4HIP_OK;
}

int gr4hip_powermetrics_process(gr4hip_powermetrics_t* h, const float* d_u, const float* d_i, size_t in_stride, size_t n_in, float* d_P, float* d_Q, float* d_S,
                                float* d_Urms, float* d_Irms, size_t out_stride, size_t* n_out, gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "powermetrics: null handle");
    const size_t D = h->p.decimate, np = h->p.n_phases;
    GR4_REQUIRE(n_in % D == 0, "powermetrics: n_in %zu is not a multiple of decimate %zu", n_in, D);
    GR4_REQUIRE(n_in < ((size_t)1 << 40), "powermetrics: n_in %zu too large", n_in);
    const size_t no = n_in / D;
    if (n_out) *n_out = no;
    if (n_in == 0) return GR4HIP_OK;
    GR4_REQUIRE(d_u && d_i, "powermetrics: null input pointer");
    GR4_REQUIRE(in_stride >= n_in && out_stride >= no, "powermetrics: a stride (%zu in, %zu out) smaller than the row (%zu in, %zu out)", in_stride, out_stride,
                n_in, no);
    GR4_REQUIRE(in_stride < ((size_t)1 << 40) && out_stride < ((size_t)1 << 40), "powermetrics: stride too large");
    float* outs[5] = {d_P, d_Q, d_S, d_Urms, d_Irms};
    {
        const size_t    in_span = ((np - 1) * in_stride + n_in) * sizeof(float), out_span = ((np - 1) * out_stride + no) * sizeof(float);
        const uintptr_t ins[2] = {reinterpret_cast<uintptr_t>(d_u), reinterpret_cast<uintptr_t>(d_i)};
        for (float* o : outs) {
            if (!o) continue;
            const uintptr_t ob = reinterpret_cast<uintptr_t>(o);
            for (uintptr_t ib : ins) GR4_REQUIRE(ob + out_span <= ib || ib + in_span <= ob, "powermetrics: an output overlaps an input");
        }
    }
    hipStream_t  st   = as_stream(stream);
    const size_t nseg = ceil_div(n_in, (size_t)kPmS);
    int          rc;
    // scratch sized for this call (a replaced buffer is fresh: hipFree waited for the device), then the pending re-initialisation, on this stream
    if ((rc = h->d_hpz.ensure(np * nseg * 4 * sizeof(double))) || (rc = h->d_chp.ensure(np * nseg * 4 * sizeof(double))) ||
        (rc = h->d_lpz.ensure(np * nseg * 6 * sizeof(double))) || (rc = h->d_clp.ensure(np * nseg * 6 * sizeof(double))))
        return rc;
    if (h->init_pending) {
        hipLaunchKernelGGL(pm_zero_state_kernel, dim3(1), dim3(256), 0, st, (double*)h->d_state[h->cur].ptr, (int)(np * kPmState));
        GR4_LAUNCH_CHECK();
        h->init_pending = false;
    }
    PmArgs a{};
    a.u         = d_u;
    a.i         = d_i;
    a.in_stride = (long)in_stride;
    a.n         = (long)n_in;
    a.nseg      = (long)nseg;
    a.vec       = ((reinterpret_cast<uintptr_t>(d_u) | reinterpret_cast<uintptr_t>(d_i)) & 15) == 0 && (np == 1 || in_stride % 4 == 0);
    a.st        = (const double*)h->d_state[h->cur].ptr;
    a.stn       = (double*)h->d_state[h->cur ^ 1].ptr;
    a.hpz       = (double*)h->d_hpz.ptr;
    a.chp       = (double*)h->d_chp.ptr;
    a.lpz       = (double*)h->d_lpz.ptr;
    a.clp       = (double*)h->d_clp.ptr;
    a.D         = (long)D;
    for (int k = 0; k < 5; ++k) a.out[k] = outs[k];
    a.out_stride = (long)out_stride;
    a.c          = h->c;
    rc = h->p.high_pass > 0.f ? pm_launch<false>(h, a, st) : pm_launch<true>(h, a, st);
    if (rc) return rc;
    h->cur ^= 1;
    return GR4HIP_OK;
}

} // extern "C"
