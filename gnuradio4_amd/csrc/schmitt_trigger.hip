// schmitt_trigger.hip -- gr::trigger::SchmittTrigger<T, Method, 32>::processOne (algorithm/.../SchmittTrigger.hpp:103-222) applied to every sample of a stream
// once, in order: the detector behind gr::blocks::basic::SchmittTrigger (blocks/basic/.../Trigger.hpp:45, N_HISTORY = 32), for NO_INTERPOLATION,
// BASIC_LINEAR_INTERPOLATION and LINEAR_INTERPOLATION and T in {int16, int32, float, double} (include/gr4hip.h "Schmitt trigger", SCHMITT_TRIGGER.md).
//
// What crosses lanes, segments and calls is a finite automaton, not a linear recurrence: one bit (_lastState) for NO / BASIC; (_lastState, in zone) plus the index
// at which the open zone was entered for LINEAR (accumulatedSamples = i - i_entry + 1).  A run of samples is a transfer map: for every entry state the exit state,
// the number of edges, and where a zone still open at the exit was entered if that happened inside the run (else it is the entry state's own).  Maps compose
// associatively and exactly (small integers), count(f o g)[s] = count_g[s] + count_f[g(s)], so every level is a parallel scan.  A call is three launches:
//   st_segment_kernel<.., false>  per segment of 4096 samples: the lanes' maps of their runs of 16, an in-block scan, the segment's map;
//   st_walk_kernel                one workgroup per tile of 512 segments: the maps in front of the tile composed (redundantly, no workgroup waits for another) and
//                                 applied to the handle's state, then the tile's maps scanned from there; leaves the true state, the open zone's entry index and
//                                 the edge rank in front of every segment, and the call's number of edges in *d_n_edges;
//   st_segment_kernel<.., true>   per segment: the same maps and scan, every lane's true entry state and rank from the segment's carry, the automaton once more,
//                                 one fit per edge read from the LDS copy (32 samples of halo in front: the handle's history or the previous segment's tail), the
//                                 edges stored at their ranks below `capacity`; the last segment's workgroup writes the handle's next state and last 32 samples
//                                 into the other of two state buffers.
// Every +, -, x and / of the fits is rounded on its own, in the reference's order (:133-142, :294-324): contraction is off for the whole file.
#include "common.hpp"

#include <climits>
#include <cmath>
#include <limits>
#include <type_traits>

#pragma clang fp contract(off)

namespace gr4 {

constexpr int  kStLanes   = 256;
constexpr int  kStJ       = 16;                     // samples per lane
constexpr int  kStS       = kStLanes * kStJ;        // samples per segment (one workgroup): GR4HIP_SCHMITT_SEGMENT
constexpr int  kStHist    = 32;                     // N_HISTORY (Trigger.hpp:45): the fit window and the halo
constexpr int  kStWalk    = 512;                    // lanes of a carry-walk workgroup = segments per tile (gr4hip_schmitt_walk_tile)
constexpr int  kStInh     = INT_MIN;                // "entered before this run": the entry state's own index
constexpr long long kStInh64 = LLONG_MIN;
constexpr size_t kStStateBytes = 16 + kStHist * 8;  // {int last, zone; long long entry (relative to the next call's sample 0)}, then 32 samples of T, oldest first
static_assert(kStS == GR4HIP_SCHMITT_SEGMENT, "the exported segment length");

struct StHead {
    int       last, zone;
    long long ent;
};

template <typename T>
struct StArgs {
    const T*       in;
    long long      n, nseg;
    int            vec;
    T              upper, lower, offset;
    const char*    st;  // the handle's state
    char*          stn; // the next one
    unsigned*      m_ex;  // [nseg]     the segments' maps: exit states, 2 bits per entry state
    int*           m_ent; // [nseg][4]  zone entry, relative to the segment (kStInh: the entry state's)
    unsigned*      m_cnt; // [nseg][4]  edges
    const int*                c_state; // [nseg]  the carries in front of every segment
    const long long*          c_ent;   //         (relative to the call)
    const unsigned long long* c_off;
    gr4hip_schmitt_edge*      edges;
    unsigned long long        capacity;
};

// LDS index of segment-relative sample i in [-32, 4096): rows of 16 padded to 17, so that the lanes' runs start on different banks
__device__ __forceinline__ int st_at(int i) { return (i + kStHist) + ((i + kStHist) >> 4); }
constexpr int kStLds = (kStS + kStHist) + ((kStS + kStHist) >> 4);

template <typename T>
__device__ __forceinline__ void st_stage(const StArgs<T>& a, long long seg0, T* __restrict__ sx) {
    constexpr int V = 16 / (int)sizeof(T); // samples per 16-byte load
    const int     t = threadIdx.x;
    union Q {
        uint4 q;
        T     v[V];
    };
    Q q[kStJ / V];
#pragma unroll
    for (int it = 0; it < kStJ / V; ++it) {
        const long long p = seg0 + (long long)it * (kStLanes * V) + t * V;
        if (a.vec && p + V <= a.n) {
            q[it].q = *reinterpret_cast<const uint4*>(a.in + p);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) q[it].v[e] = p + e < a.n ? a.in[p + e] : T(0);
        }
    }
#pragma unroll
    for (int it = 0; it < kStJ / V; ++it) {
        const int e0 = it * (kStLanes * V) + t * V;
#pragma unroll
        for (int e = 0; e < V; ++e) sx[st_at(e0 + e)] = q[it].v[e];
    }
    if (t < kStHist) // the halo: the previous segment's tail, or the handle's history in front of the call
        sx[st_at(t - kStHist)] = seg0 > 0 ? a.in[seg0 - kStHist + t] : reinterpret_cast<const T*>(a.st + 16)[t];
}

// what one sample means to the automaton; a NaN compares false everywhere and holds every state
struct StPred {
    bool ge_u, le_l, gt_l, lt_u, lt_l, gt_u, p_le_l, p_ge_u;
};
template <typename T>
__device__ __forceinline__ StPred st_pred(T prev, T x, T upper, T lower) {
    return {x >= upper, x <= lower, x > lower, x < upper, x < lower, x > upper, prev <= lower, prev >= upper};
}

// processOne's state update.  NO / BASIC (:107-121, :144-163): one bit.  LINEAR (:175-219): a zone is entered only while none is open, an edge needs an open
// zone, the zone is abandoned on the near side.  Returns whether the sample is an edge; `ent` is the index at which the open zone was entered.
template <bool LIN, typename E>
__device__ __forceinline__ bool st_step(const StPred& q, int& last, int& zone, E& ent, E pos) {
    if constexpr (!LIN) {
        if (!last && q.ge_u) { last = 1; return true; }
        if (last && q.le_l) { last = 0; return true; }
        return false;
    } else {
        if (!zone && (last ? (q.p_ge_u && q.lt_u) : (q.p_le_l && q.gt_l))) {
            zone = 1;
            ent  = pos;
        }
        if (zone) {
            if (last ? q.le_l : q.ge_u) {
                last ^= 1;
                zone = 0;
                return true;
            }
            if (last ? q.gt_u : q.lt_l) zone = 0;
        }
        return false;
    }
}

// a transfer map over NS entry states (state = last | zone << 1)
template <int NS, typename E, typename Cn>
struct StMap {
    unsigned ex;
    E        ent[NS];
    Cn       cnt[NS];
};
template <int NS, int LANES, typename E, typename Cn>
struct StScanLds {
    unsigned ex[LANES];
    E        ent[NS][LANES];
    Cn       cnt[NS][LANES];
};

// inclusive scan of the lanes' maps in lane order; the result is left in sh (and in m)
template <int NS, int LANES, typename E, typename Cn>
__device__ __forceinline__ void st_scan(StScanLds<NS, LANES, E, Cn>& sh, StMap<NS, E, Cn>& m, E inh) {
    const int t = threadIdx.x;
    __syncthreads(); // (sh may still be read by an earlier use)
    sh.ex[t] = m.ex;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        sh.ent[s][t] = m.ent[s];
        sh.cnt[s][t] = m.cnt[s];
    }
    __syncthreads();
    for (int off = 1; off < LANES; off <<= 1) {
        StMap<NS, E, Cn> r = m;
        if (t >= off) { // r = m o g: g (the lanes in front) first
            const unsigned gex = sh.ex[t - off];
            r.ex = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int mid = (gex >> (2 * s)) & 3;
                E         e   = m.ent[0];
                Cn        c   = m.cnt[0];
#pragma unroll
                for (int k = 1; k < NS; ++k) {
                    if (mid == k) {
                        e = m.ent[k];
                        c = m.cnt[k];
                    }
                }
                r.ex |= ((m.ex >> (2 * mid)) & 3u) << (2 * s);
                r.ent[s] = e != inh ? e : sh.ent[s][t - off];
                r.cnt[s] = sh.cnt[s][t - off] + c;
            }
        }
        __syncthreads();
        m = r;
        if (t >= off) {
            sh.ex[t] = m.ex;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                sh.ent[s][t] = m.ent[s];
                sh.cnt[s][t] = m.cnt[s];
            }
        }
        __syncthreads();
    }
}

template <typename T>
struct StComp {
    using type = float; // comp_t (:295): float for the integer types
};
template <>
struct StComp<double> {
    using type = double;
};

__device__ __forceinline__ float  st_round(float x) { return roundf(x); }
__device__ __forceinline__ double st_round(double x) { return round(x); }

// computeEdgePosition (:133-142) on float(yPrev), float(yCurr), float(offset)
__device__ __forceinline__ void st_fit_basic(float y1, float y2, float offset, int& idx, float& frac, unsigned& flags) {
    idx  = 0;
    frac = 0.f;
    if (y1 == y2) return;
    const float o  = (offset - y1) / (y2 - y1);
    const float cp = -1.0f + o;
    const float r  = roundf(cp);
    if (!(r >= -2147483648.0f && r < 2147483648.0f)) { // (NaN too) the reference's conversion is undefined
        flags |= GR4HIP_SCHMITT_DEGENERATE;
        return;
    }
    idx  = (int)r;
    frac = cp - (float)idx;
}

// findCrossingIndexLinearRegression (:294-324) over the n newest samples, newest first, and what :198-205 make of it.  sx: the LDS copy, p: the edge's sample.
template <typename T>
__device__ __forceinline__ void st_fit_linear(const T* __restrict__ sx, int p, int n, T offset, int& idx, float& frac, unsigned& flags) {
    using C = typename StComp<T>::type;
    const C nv    = (C)n;
    const C sumX2 = (nv * (nv - C(1)) * (C(2) * nv - C(1))) / C(6);
    const C meanX = C(0.5) * (nv - C(1));
    C       sumY = C(0), sumXY = C(0);
    for (int i = 0; i < n; ++i) {
        const C xi = (C)((n - 1) - i);
        const C yi = (C)sx[st_at(p - i)];
        sumY += yi;
        sumXY += xi * yi;
    }
    const C meanY       = sumY / nv;
    const C numerator   = sumXY - nv * meanX * meanY;
    const C denominator = sumX2 - nv * meanX * meanX; // (never 0 for 2 <= n <= 32)
    const C slope       = numerator / denominator;
    const C intercept   = meanY - slope * meanX;
    const C crossing    = ((C)offset - intercept) / slope;
    idx  = 0;
    frac = 0.f;
    if constexpr (std::is_floating_point_v<T>) {
        const T rel = crossing - (T)(n - 1); // (:198)
        const T r   = st_round(rel);
        if (!(r >= T(-2147483648.0) && r < T(2147483648.0))) {
            flags |= GR4HIP_SCHMITT_DEGENERATE;
            return;
        }
        idx  = (int)r;
        frac = (float)rel - (float)idx; // (:205)
    } else {
        // static_cast<value_t>(crossingIndex) truncates (:355); relativeIndex is value_t, so the offset is 0.  A value that leaves T's range is undefined there.
        constexpr float lo = (float)std::numeric_limits<T>::min(), hi = -(float)std::numeric_limits<T>::min();
        const float     tr = truncf(crossing);
        if (!(tr >= lo && tr < hi)) {
            flags |= GR4HIP_SCHMITT_DEGENERATE;
            return;
        }
        const long long rel = (long long)(T)tr - (long long)(n - 1);
        if (rel < (long long)std::numeric_limits<T>::min()) {
            flags |= GR4HIP_SCHMITT_DEGENERATE;
            return;
        }
        idx = (int)rel;
    }
}

// APPLY false: the segment's map.  APPLY true: the edges, and behind the call's last sample the handle's next state.  METHOD matters to APPLY only (BASIC's
// automaton is NO's).
template <typename T, int METHOD, bool APPLY>
__global__ __launch_bounds__(kStLanes) void st_segment_kernel(const StArgs<T> a) {
    constexpr bool LIN = METHOD == GR4HIP_SCHMITT_LINEAR_INTERPOLATION;
    constexpr int  NS  = LIN ? 4 : 2;
    using Map          = StMap<NS, int, unsigned>;
    __shared__ T                                       sx[kStLds];
    __shared__ StScanLds<NS, kStLanes, int, unsigned> sh;
    const int       t    = threadIdx.x;
    const long long s    = blockIdx.x;
    const long long seg0 = s * kStS;
    st_stage(a, seg0, sx);
    __syncthreads();
    const int       r0 = t * kStJ; // the lane's run, relative to the segment
    const long long p0 = seg0 + r0;
    const int       m  = p0 >= a.n ? 0 : (int)min((long long)kStJ, a.n - p0);

    T x[kStJ + 1]; // x[0]: the sample in front of the run
#pragma unroll
    for (int k = 0; k <= kStJ; ++k) x[k] = sx[st_at(r0 - 1 + k)];

    int last[NS], zone[NS];
    Map mp;
#pragma unroll
    for (int e = 0; e < NS; ++e) {
        last[e]   = e & 1;
        zone[e]   = e >> 1;
        mp.ent[e] = kStInh;
        mp.cnt[e] = 0;
    }
#pragma unroll
    for (int k = 0; k < kStJ; ++k) {
        if (k < m) {
            const StPred q = st_pred(x[k], x[k + 1], a.upper, a.lower);
#pragma unroll
            for (int e = 0; e < NS; ++e) mp.cnt[e] += st_step<LIN, int>(q, last[e], zone[e], mp.ent[e], r0 + k) ? 1u : 0u;
        }
    }
    mp.ex = 0;
#pragma unroll
    for (int e = 0; e < NS; ++e) mp.ex |= (unsigned)(last[e] | (zone[e] << 1)) << (2 * e);
    st_scan<NS, kStLanes, int, unsigned>(sh, mp, kStInh);

    if constexpr (!APPLY) {
        if (t == kStLanes - 1) {
            a.m_ex[s] = mp.ex;
#pragma unroll
            for (int e = 0; e < NS; ++e) {
                a.m_ent[s * 4 + e] = mp.ent[e];
                a.m_cnt[s * 4 + e] = mp.cnt[e];
            }
        }
    } else {
        // the lane's true entry state: the lanes in front applied to the segment's carry
        const int          cs   = a.c_state[s];
        const long long    cent = a.c_ent[s] - seg0; // < 0
        unsigned long long rank = a.c_off[s];
        int                st   = cs;
        int                ent  = (int)max(cent, (long long)-2 * kStHist); // (accumulatedSamples past 32 all fit alike)
        if (t > 0) {
            st = (sh.ex[t - 1] >> (2 * cs)) & 3;
            const int e = sh.ent[cs][t - 1];
            if (e != kStInh) ent = e;
            rank += sh.cnt[cs][t - 1];
        }
        int lst = st & 1, zn = st >> 1;
#pragma unroll
        for (int k = 0; k < kStJ; ++k) {
            if (k < m) {
                const StPred q      = st_pred(x[k], x[k + 1], a.upper, a.lower);
                const int    before = lst;
                if (st_step<LIN, int>(q, lst, zn, ent, r0 + k)) {
                    if (rank < a.capacity) {
                        const int p     = r0 + k;
                        unsigned  flags = before ? GR4HIP_SCHMITT_FALLING : GR4HIP_SCHMITT_RISING;
                        int       idx = 0, nfit = 0;
                        float     frac = 0.f;
                        if constexpr (METHOD == GR4HIP_SCHMITT_BASIC_LINEAR_INTERPOLATION) {
                            nfit = 2;
                            st_fit_basic((float)x[k], (float)x[k + 1], (float)a.offset, idx, frac, flags);
                        } else if constexpr (LIN) {
                            const int acc = p - ent + 1;
                            nfit          = min(max(acc, 2), kStHist); // (:194)
                            st_fit_linear<T>(sx, p, nfit, a.offset, idx, frac, flags);
                        }
                        gr4hip_schmitt_edge e;
                        e.sample      = p0 + k;
                        e.edge_idx    = idx;
                        e.edge_offset = frac;
                        e.kind_flags  = flags;
                        e.n_fit       = (unsigned)nfit;
                        a.edges[rank] = e;
                    }
                    ++rank;
                }
            }
        }
        if (s == a.nseg - 1) {
            if (m > 0 && p0 + m == a.n) {
                StHead h;
                h.last = lst;
                h.zone = zn;
                h.ent  = zn ? max((long long)ent - (a.n - seg0), (long long)-2 * kStHist) : 0;
                *reinterpret_cast<StHead*>(a.stn) = h;
            }
            if (t < kStHist) reinterpret_cast<T*>(a.stn + 16)[t] = sx[st_at((int)(a.n - seg0) - kStHist + t)];
        }
    }
}

// g first, f second: exit(f o g)[s] = exit_f[exit_g[s]], count(f o g)[s] = count_g[s] + count_f[exit_g[s]], the zone entry is f's if f knows one, else g's
template <int NS, typename E, typename Cn>
__device__ __forceinline__ StMap<NS, E, Cn> st_compose(const StMap<NS, E, Cn>& g, const StMap<NS, E, Cn>& f, E inh) {
    StMap<NS, E, Cn> r;
    r.ex = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int mid = (g.ex >> (2 * s)) & 3;
        E         e   = f.ent[0];
        Cn        c   = f.cnt[0];
#pragma unroll
        for (int k = 1; k < NS; ++k) {
            if (mid == k) {
                e = f.ent[k];
                c = f.cnt[k];
            }
        }
        r.ex |= ((f.ex >> (2 * mid)) & 3u) << (2 * s);
        r.ent[s] = e != inh ? e : g.ent[s];
        r.cnt[s] = g.cnt[s] + c;
    }
    return r;
}

// segment q's map with its zone entries relative to the call; the identity behind the call's last segment
template <int NS>
__device__ __forceinline__ StMap<NS, long long, unsigned long long> st_walk_load(const unsigned* __restrict__ m_ex, const int* __restrict__ m_ent,
                                                                                  const unsigned* __restrict__ m_cnt, long long q, long long nseg) {
    StMap<NS, long long, unsigned long long> mp;
    mp.ex = 0;
#pragma unroll
    for (int e = 0; e < NS; ++e) {
        mp.ex |= (unsigned)e << (2 * e);
        mp.ent[e] = kStInh64;
        mp.cnt[e] = 0;
    }
    if (q < nseg) {
        mp.ex = m_ex[q];
#pragma unroll
        for (int e = 0; e < NS; ++e) {
            const int r = m_ent[q * 4 + e];
            mp.ent[e]   = r == kStInh ? kStInh64 : q * kStS + r;
            mp.cnt[e]   = m_cnt[q * 4 + e];
        }
    }
    return mp;
}

// a scanned tile's last map applied to the state (cs, ent, off) in front of it
template <int NS>
__device__ __forceinline__ void st_walk_advance(const StScanLds<NS, kStWalk, long long, unsigned long long>& sh, int at, int& cs, long long& ent, unsigned long long& off) {
    const long long e = sh.ent[cs][at];
    if (e != kStInh64) ent = e;
    off += sh.cnt[cs][at];
    cs = (sh.ex[at] >> (2 * cs)) & 3;
}

// The carries: what stands in front of every segment.  Workgroup b owns the tile of kStWalk segments from b * kStWalk, one per lane.  No workgroup waits for
// another: b first composes the b * kStWalk maps in front of its tile itself, b consecutive ones per lane in order and one scan over the lanes, and applies the
// result to the handle's state; then it scans its own tile from there.  The maps are small integers and compose exactly, so the association does not matter.
// The work in front of the tiles grows with the square of their number (b maps per lane, 63 at most for 2^27 samples): SCHMITT_TRIGGER.md "Rates and limits".
template <int NS>
__global__ __launch_bounds__(kStWalk) void st_walk_kernel(const unsigned* __restrict__ m_ex, const int* __restrict__ m_ent, const unsigned* __restrict__ m_cnt, long long nseg,
                                                           const char* __restrict__ st, int* __restrict__ c_state, long long* __restrict__ c_ent,
                                                           unsigned long long* __restrict__ c_off, unsigned long long* __restrict__ d_n_edges) {
    using Map = StMap<NS, long long, unsigned long long>;
    __shared__ StScanLds<NS, kStWalk, long long, unsigned long long> sh;
    const int          t    = threadIdx.x;
    const long long    per  = blockIdx.x; // maps per lane in front of the tile
    const long long    base = per * kStWalk;
    const StHead       h    = *reinterpret_cast<const StHead*>(st);
    int                cs   = NS == 4 ? (h.last | (h.zone << 1)) : h.last;
    long long          ent  = h.ent;
    unsigned long long off  = 0;
    if (per > 0) {
        Map mp = st_walk_load<NS>(m_ex, m_ent, m_cnt, t * per, nseg);
#pragma unroll 4
        for (long long j = 1; j < per; ++j) mp = st_compose<NS>(mp, st_walk_load<NS>(m_ex, m_ent, m_cnt, t * per + j, nseg), kStInh64);
        st_scan<NS, kStWalk, long long, unsigned long long>(sh, mp, kStInh64);
        st_walk_advance<NS>(sh, kStWalk - 1, cs, ent, off);
    }
    const long long q  = base + t;
    Map             mp = st_walk_load<NS>(m_ex, m_ent, m_cnt, q, nseg);
    st_scan<NS, kStWalk, long long, unsigned long long>(sh, mp, kStInh64); // (its first barrier: every lane has read the scan above)
    if (base + kStWalk >= nseg && t == 0) { // the last tile (padded with identities): the call's number of edges
        int                c2 = cs;
        long long          e2 = ent;
        unsigned long long n2 = off;
        st_walk_advance<NS>(sh, kStWalk - 1, c2, e2, n2);
        *d_n_edges = n2;
    }
    if (q < nseg) {
        if (t > 0) st_walk_advance<NS>(sh, t - 1, cs, ent, off);
        c_state[q] = cs;
        c_ent[q]   = ent;
        c_off[q]   = off;
    }
}

template <typename T>
static bool st_in_range(double v) {
    if constexpr (std::is_integral_v<T>) return v >= (double)std::numeric_limits<T>::min() && v <= (double)std::numeric_limits<T>::max();
    return std::isfinite((double)(T)v);
}

template <typename T>
static int st_check_t(const gr4hip_schmitt_params* p, const char* name) {
    if constexpr (std::is_integral_v<T>) {
        GR4_REQUIRE(p->offset == std::floor(p->offset) && p->threshold == std::floor(p->threshold), "schmitt: offset %g / threshold %g are no %s values", p->offset,
                    p->threshold, name);
    }
    GR4_REQUIRE(st_in_range<T>(p->offset) && st_in_range<T>(p->threshold), "schmitt: offset %g / threshold %g outside %s", p->offset, p->threshold, name);
    // upper = offset + threshold, lower = offset - threshold in the value type (:67): a sum that leaves an integer type's range is undefined there
    GR4_REQUIRE(st_in_range<T>((double)(T)p->offset + (double)(T)p->threshold) && st_in_range<T>((double)(T)p->offset - (double)(T)p->threshold),
                "schmitt: offset %g +- threshold %g leaves the range of %s", p->offset, p->threshold, name);
    return GR4HIP_OK;
}

static int st_check(const gr4hip_schmitt_params* p) {
    GR4_REQUIRE(p, "schmitt: null params");
    if (p->method == GR4HIP_SCHMITT_POLYNOMIAL_INTERPOLATION) {
        set_error("schmitt: POLYNOMIAL_INTERPOLATION needs the Savitzky-Golay coefficient design, which this library does not have");
        return GR4HIP_UNSUPPORTED;
    }
    GR4_REQUIRE(p->method >= GR4HIP_SCHMITT_NO_INTERPOLATION && p->method <= GR4HIP_SCHMITT_LINEAR_INTERPOLATION, "schmitt: unknown method %d", p->method);
    GR4_REQUIRE(std::isfinite(p->offset), "schmitt: offset %g", p->offset);
    GR4_REQUIRE(std::isfinite(p->threshold) && p->threshold >= 0.0, "schmitt: threshold %g (finite, not negative)", p->threshold);
    switch (p->dtype) {
    case GR4HIP_I16: return st_check_t<int16_t>(p, "int16");
    case GR4HIP_I32: return st_check_t<int32_t>(p, "int32");
    case GR4HIP_F32: return st_check_t<float>(p, "float");
    case GR4HIP_F64: return st_check_t<double>(p, "double");
    default: GR4_REQUIRE(false, "schmitt: dtype %d (int16, int32, float, double)", p->dtype);
    }
    return GR4HIP_OK;
}

} // namespace gr4

using namespace gr4;

struct gr4hip_schmitt {
    gr4hip_schmitt_params p{};
    bool                  init_pending = true; // the state to be reset in front of the next launch, on its stream
    int                   cur          = 0;    // which state buffer holds the state
    DeviceBuffer          d_state[2], d_maps, d_carry;
};

template <typename T, int METHOD>
static int st_launch_m(StArgs<T>& a, unsigned long long* d_n_edges, hipStream_t st) {
    constexpr int NS = METHOD == GR4HIP_SCHMITT_LINEAR_INTERPOLATION ? 4 : 2;
    hipLaunchKernelGGL((st_segment_kernel<T, METHOD == GR4HIP_SCHMITT_LINEAR_INTERPOLATION ? METHOD : GR4HIP_SCHMITT_NO_INTERPOLATION, false>), dim3((unsigned)a.nseg),
                       dim3(kStLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL(st_walk_kernel<NS>, dim3((unsigned)ceil_div((size_t)a.nseg, (size_t)kStWalk)), dim3(kStWalk), 0, st, (const unsigned*)a.m_ex, (const int*)a.m_ent, (const unsigned*)a.m_cnt, a.nseg, a.st,
                       const_cast<int*>(a.c_state), const_cast<long long*>(a.c_ent), const_cast<unsigned long long*>(a.c_off), d_n_edges);
    GR4_LAUNCH_CHECK();
    hipLaunchKernelGGL((st_segment_kernel<T, METHOD, true>), dim3((unsigned)a.nseg), dim3(kStLanes), 0, st, a);
    GR4_LAUNCH_CHECK();
    return GR4HIP_OK;
}

template <typename T>
static int st_launch(gr4hip_schmitt_t* h, const void* d_in, size_t n_in, gr4hip_schmitt_edge* d_edges, size_t capacity, unsigned long long* d_n_edges, hipStream_t st) {
    const size_t nseg = ceil_div(n_in, (size_t)kStS);
    StArgs<T>    a{};
    a.in     = static_cast<const T*>(d_in);
    a.n      = (long long)n_in;
    a.nseg   = (long long)nseg;
    a.vec    = (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
    a.offset = (T)h->p.offset;
    a.upper  = (T)((T)h->p.offset + (T)h->p.threshold);
    a.lower  = (T)((T)h->p.offset - (T)h->p.threshold);
    a.st     = (const char*)h->d_state[h->cur].ptr;
    a.stn    = (char*)h->d_state[h->cur ^ 1].ptr;
    char* mp = (char*)h->d_maps.ptr;
    a.m_ex   = (unsigned*)mp;
    a.m_ent  = (int*)(mp + nseg * 4);
    a.m_cnt  = (unsigned*)(mp + nseg * 20);
    char* cp = (char*)h->d_carry.ptr;
    a.c_ent  = (const long long*)cp;
    a.c_off  = (const unsigned long long*)(cp + nseg * 8);
    a.c_state = (const int*)(cp + nseg * 16);
    a.edges    = d_edges;
    a.capacity = capacity;
    switch (h->p.method) {
    case GR4HIP_SCHMITT_NO_INTERPOLATION: return st_launch_m<T, GR4HIP_SCHMITT_NO_INTERPOLATION>(a, d_n_edges, st);
    case GR4HIP_SCHMITT_BASIC_LINEAR_INTERPOLATION: return st_launch_m<T, GR4HIP_SCHMITT_BASIC_LINEAR_INTERPOLATION>(a, d_n_edges, st);
    default: return st_launch_m<T, GR4HIP_SCHMITT_LINEAR_INTERPOLATION>(a, d_n_edges, st);
    }
}

extern "C" {

int gr4hip_schmitt_params_default(gr4hip_schmitt_params* p) {
    GR4_REQUIRE(p, "schmitt: null params");
    *p = gr4hip_schmitt_params{0.0, 1.0, GR4HIP_SCHMITT_NO_INTERPOLATION, GR4HIP_F32}; // (:45-46, Trigger.hpp:52-53)
    return GR4HIP_OK;
}

size_t gr4hip_schmitt_segment(void) { return (size_t)kStS; }

size_t gr4hip_schmitt_walk_tile(void) { return (size_t)kStWalk; }

int gr4hip_schmitt_check(const gr4hip_schmitt_params* p) { return st_check(p); }

int gr4hip_schmitt_create(gr4hip_schmitt_t** out, const gr4hip_schmitt_params* p) {
    GR4_REQUIRE(out, "schmitt: null output handle");
    int rc = st_check(p); // (validated before anything is allocated)
    if (rc) return rc;
    auto* h = new (std::nothrow) gr4hip_schmitt();
    GR4_REQUIRE(h, "out of host memory");
    h->p = *p;
    for (auto& b : h->d_state)
        if (!rc) rc = b.ensure(kStStateBytes);
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return GR4HIP_OK;
}

int gr4hip_schmitt_set_params(gr4hip_schmitt_t* h, const gr4hip_schmitt_params* p) {
    GR4_REQUIRE(h, "schmitt: null handle");
    const int rc = st_check(p);
    if (rc) return rc;
    GR4_REQUIRE(p->dtype == h->p.dtype, "schmitt: the sample type is fixed at create (%d, not %d)", h->p.dtype, p->dtype);
    h->p            = *p;
    h->init_pending = true; // settingsChanged resets the detector (Trigger.hpp:76-80)
    return GR4HIP_OK;
}

int gr4hip_schmitt_reset(gr4hip_schmitt_t* h) {
    GR4_REQUIRE(h, "schmitt: null handle");
    h->init_pending = true;
    return GR4HIP_OK;
}

int gr4hip_schmitt_destroy(gr4hip_schmitt_t* h) {
    delete h;
    return GR4HIP_OK;
}

int gr4hip_schmitt_process(gr4hip_schmitt_t* h, const void* d_in, size_t n_in, gr4hip_schmitt_edge* d_edges, size_t capacity, unsigned long long* d_n_edges,
                           gr4hip_stream_t stream) {
    GR4_REQUIRE(h, "schmitt: null handle");
    GR4_REQUIRE(d_n_edges, "schmitt: null edge counter");
    // the carry walk composes the tiles in front of every tile once more: beyond this length that work would no longer be small against the two streaming passes
    GR4_REQUIRE(n_in <= (size_t)GR4HIP_SCHMITT_MAX_SAMPLES, "schmitt: n_in %zu exceeds GR4HIP_SCHMITT_MAX_SAMPLES (a longer stream goes in several calls)", n_in);
    GR4_REQUIRE(capacity == 0 || d_edges, "schmitt: null edge buffer with capacity %zu", capacity);
    hipStream_t st = as_stream(stream);
    if (n_in == 0) {
        GR4_HIP_TRY(hipMemsetAsync(d_n_edges, 0, sizeof(unsigned long long), st));
        return GR4HIP_OK;
    }
    GR4_REQUIRE(d_in, "schmitt: null input pointer");
    const size_t esz = dtype_size(h->p.dtype);
    GR4_REQUIRE((reinterpret_cast<uintptr_t>(d_in) & (esz - 1)) == 0, "schmitt: the input is not aligned to its sample type");
    const size_t nseg = ceil_div(n_in, (size_t)kStS);
    int          rc;
    // scratch sized for this call (a replaced buffer is fresh: hipFree waited for the device), then the pending reset, on this stream
    if ((rc = h->d_maps.ensure(nseg * 36)) || (rc = h->d_carry.ensure(nseg * 20))) return rc;
    if (h->init_pending) { // reset() (:90-101): _lastState false, nothing accumulated, a history of 32 zeros
        GR4_HIP_TRY(hipMemsetAsync(h->d_state[h->cur].ptr, 0, kStStateBytes, st));
        h->init_pending = false;
    }
    switch (h->p.dtype) {
    case GR4HIP_I16: rc = st_launch<int16_t>(h, d_in, n_in, d_edges, capacity, d_n_edges, st); break;
    case GR4HIP_I32: rc = st_launch<int32_t>(h, d_in, n_in, d_edges, capacity, d_n_edges, st); break;
    case GR4HIP_F32: rc = st_launch<float>(h, d_in, n_in, d_edges, capacity, d_n_edges, st); break;
    default: rc = st_launch<double>(h, d_in, n_in, d_edges, capacity, d_n_edges, st); break;
    }
    if (rc) return rc;
    h->cur ^= 1;
    return GR4HIP_OK;
}

} // extern "C"
