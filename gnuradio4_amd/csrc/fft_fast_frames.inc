// fft_fast_frames.inc -- the body of fft_fast_kernel<LOG2N, REAL> (fft_kernels.hpp), included textually by every kernel that runs its frame loop, so that all of
// them compile the same statements.  Expects in scope: LOG2N, REAL, FRONT / front (the first-pass load; FRONT::kSink: it takes |X|^2 instead of the store; FRONT::kBinSink: it takes the bins instead of every store), in,
// window, tw, out (FftOutputs), n_frames.
    constexpr int N = 1 << LOG2N, T = N / 16, FPB = 512 / T, NP = N + N / 32, HALF = N / 2;
    constexpr int TWS = REAL ? 2 : 1; // stride of W_N^j in the table
    static_assert(!REAL || LOG2N <= 12, "the real-input split is implemented for the 16 x 16 x R3 plans");
    constexpr int R3  = N >= 4096 ? 16 : N / 256; // 256 -> 1 (no third pass)
    constexpr int R4  = N / (256 * R3);           // 8192 -> 2
    constexpr int B3  = R3 > 1 ? 16 / R3 : 1;     // third-pass butterflies per lane
    constexpr int NB3 = N / R3;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    auto P = [](int i) { return i + (i >> 5); };
    const int t0 = threadIdx.x % T;

    // per-lane twiddle bases, exact table values (tw[j] = W_N^j)
    const float2 w2a_ = tw[TWS * (t0 & 15) * (N / 256)], w2b_ = tw[TWS * 2 * (t0 & 15) * (N / 256)]; // W_256^k, W_256^2k
    // third pass, butterfly b of the lane: k = t + b T (< 256), W_{256 R3}^k = W_{256 R3}^t W_16^b  (256 R3 = N below 8192)
    float2 w3_ = make_float2(1.f, 0.f), w3sq_ = make_float2(1.f, 0.f);
    // (8192: the lane's third-pass butterfly is i = (t >> 1) + 256 (t & 1), k = t >> 1, see below)
    constexpr int kShift3 = R4 == 2 ? 1 : 0;
    if constexpr (R3 > 1) w3_ = tw[TWS * ((t0 >> kShift3) & 255) * (N / (256 * R3))];
    if constexpr (R3 == 16) w3sq_ = tw[TWS * 2 * ((t0 >> kShift3) & 255) * (N / 4096)];
    float2 w4_ = make_float2(1.f, 0.f);
    if constexpr (R4 == 2) w4_ = tw[t0 >> 1]; // W_8192^{t >> 1}
    const float2 wr_  = REAL ? tw[t0] : make_float2(1.f, 0.f); // REAL: W_2N^t, the split twiddle of bin t + j T is this times W_32^j
    const rsrc_t rwin = make_rsrc(window, window ? (REAL ? 2 : 1) * N * 4u : 0u);

    const long ngroups = (n_frames + FPB - 1) / FPB;
    for (long g = front.first_group(); g < front.end_group(ngroups); g += front.group_stride()) { // (the FFT block: blockIdx.x, ngroups, gridDim.x)
        // all global accesses of this iteration go through buffer descriptors over the group's FPB frames: one 32-bit lane offset +
        // compile-time bin offsets, frames past n_frames fall out of range (loads return 0, stores are dropped)
        // (the lane id is laundered every iteration: lane-dependent LDS / buffer offsets are recomputed instead of being hoisted out of
        // the loop as dozens of loop-invariant VGPRs)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        // same for the twiddle bases: their power chains are loop-invariant and hipcc would keep all ~35 products in registers
        float2 w2a = w2a_, w2b = w2b_, w3sq = w3sq_, w4 = w4_;
        asm volatile("" : "+v"(w2a.x), "+v"(w2a.y), "+v"(w2b.x), "+v"(w2b.y), "+v"(w3sq.x), "+v"(w3sq.y), "+v"(w4.x), "+v"(w4.y));
        float2 w3 = w3_;
        asm volatile("" : "+v"(w3.x), "+v"(w3.y));
        const int      fl    = tid / T, t = tid % T;
        float2*        buf   = lds + fl * NP;
        const long     f0    = front.template group<FPB>(g, ngroups) * FPB; // (the FFT block: group g itself)
        const unsigned nlive = (unsigned)(n_frames - f0 < FPB ? n_frames - f0 : FPB);
        const int      vN    = fl * N + t; // element offset of (frame slot, bin t) in an [FPB][N] group (input side)
        float2         v[16];
        // ---- pass 1 (p = 1, radix 16) from global memory; window (fft.hpp:148-162); real input becomes (x*w, 0)
        if constexpr (FRONT::kFrontEnd) {
            front.template load<N>(v, f0, nlive, fl, t);
        } else if constexpr (REAL) {
            const rsrc_t rx = make_rsrc(in + f0 * N * 2, nlive * N * 8u); // 2N floats per frame = N float2
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = buf_load_f2(rx, vN * 8, r * T * 8);
            if (window) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float2 w = buf_load_f2(rwin, t * 8, r * T * 8); v[r].x *= w.x; v[r].y *= w.y; }
            }
        } else if (out.real_input) {
            const rsrc_t rx = make_rsrc(in + f0 * N, nlive * N * 4u);
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = make_float2(buf_load_f(rx, vN * 4, r * T * 4), 0.f);
        } else {
            const rsrc_t rx = make_rsrc(in + f0 * N * 2, nlive * N * 8u);
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = buf_load_f2(rx, vN * 8, r * T * 8);
        }
        if (!REAL && window) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float w = buf_load_f(rwin, t * 4, r * T * 4); v[r].x *= w; v[r].y *= w; }
        }
        fft16<1>(v);
#pragma unroll
        for (int r = 0; r < 16; ++r) buf[P(16 * t + r)] = v[perm16(r)];
        __syncthreads();
        // ---- pass 2 (p = 16, radix 16): butterfly i = t, k = t & 15
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = buf[P(t + r * T)];
        __syncthreads();
        apply_powers(v, w2a, w2b);
        fft16<1>(v);
        float2 X[16]; // X[j] = bin t + j T
        if constexpr (R3 == 1) { // N = 256: bins t + 16 q
#pragma unroll
            for (int q = 0; q < 16; ++q) X[q] = v[perm16(q)];
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) buf[P((t & ~15) * 16 + (t & 15) + 16 * q)] = v[perm16(q)];
            __syncthreads();
            // ---- pass 3 (p = 256, radix R3): butterflies i_b = t + b T, k = i_b & 255
            // 8192: the two butterflies whose outputs meet in the final radix-2 step (i and i + 256) go to NEIGHBOURING lanes
            const int i3 = R4 == 2 ? (t >> 1) + 256 * (t & 1) : t;
#pragma unroll
            for (int b = 0; b < B3; ++b)
#pragma unroll
                for (int r = 0; r < R3; ++r) v[b * R3 + r] = buf[P(i3 + b * T + r * NB3)];
            __syncthreads();
            if constexpr (R3 == 16) {
                apply_powers(v, w3, w3sq);
                fft16<1>(v);
            } else {
#pragma unroll
                for (int b = 0; b < B3; ++b) {
                    const float2 wb = b == 0 ? w3 : cmul(w3, w32(2 * b));
                    float2       pw = wb;
#pragma unroll
                    for (int r = 1; r < R3; ++r) {
                        v[b * R3 + r] = cmul(v[b * R3 + r], pw);
                        if (r + 1 < R3) pw = cmul(pw, wb);
                    }
                    dft_small<R3>(v + b * R3);
                }
            }
            if constexpr (R4 == 1) { // last pass: k = i_b, bins i_b + 256 q = t + (b + q B3) T
#pragma unroll
                for (int b = 0; b < B3; ++b)
#pragma unroll
                    for (int q = 0; q < R3; ++q) X[b + q * B3] = v[b * R3 + (R3 == 16 ? perm16(q) : q)];
            } else { // N = 8192, pass 4 (p = 4096, radix 2) across the lane pair through DPP, no fourth LDS round trip:
                // even lane a = X3[i][q], odd lane b = X3[i + 256][q];  bin k3 + 256 q = a + W b (even lane), + 4096: a - W b (odd lane),
                // W = W_8192^{k3 + 256 q} = W_8192^{k3} W_32^q
                const int   par = t & 1;
                const float sgn = par ? -1.f : 1.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    float2       u  = v[perm16(q)];
                    const float2 uw = cmul(u, q == 0 ? w4 : cmul(w4, w32(q)));
                    u.x = par ? uw.x : u.x;
                    u.y = par ? uw.y : u.y;
                    const float2 o = make_float2(lane_xor1(u.x), lane_xor1(u.y));
                    X[q] = make_float2(fmaf(sgn, u.x, o.x), fmaf(sgn, u.y, o.y));
                }
            }
        }
        // per-frame {min, max} of the four DataSet signals, accumulated while the values are in registers (no second pass over HBM)
        float rmin[4], rmax[4];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) { rmin[g4] = FLT_MAX; rmax[g4] = -FLT_MAX; }
        auto track = [&](int sig, float v) { rmin[sig] = fminf(rmin[sig], v); rmax[sig] = fmaxf(rmax[sig], v); };
        if constexpr (REAL) {
            // ---- split: X[j] holds Z[k], k = t + j T; the partner Z[(N - k) mod N] lives in another lane -> one more LDS round trip
            float2 wr = wr_;
            asm volatile("" : "+v"(wr.x), "+v"(wr.y));
#pragma unroll
            for (int j = 0; j < 16; ++j) buf[P(t + j * T)] = X[j];
            __syncthreads();
            float2 Zp[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) Zp[j] = buf[P((N - (t + j * T)) & (N - 1))];
            __syncthreads(); // buf is rewritten by the next iteration
            const float nyq = X[0].x - X[0].y; // bin N (lane t = 0 only): Re Z[0] - Im Z[0]
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float2 e  = make_float2(0.5f * (X[j].x + Zp[j].x), 0.5f * (X[j].y - Zp[j].y));
                const float2 o  = make_float2(0.5f * (X[j].y + Zp[j].y), -0.5f * (X[j].x - Zp[j].x)); // -i (Z - conj Zp) / 2
                const float2 wk = j == 0 ? wr : cmul(wr, w32(j));
                X[j]            = cadd(e, cmul(wk, o));
            }
            const int vH = fl * N + t; // outputs are [frames][N]
            if (out.mag) {
                const rsrc_t r = make_rsrc(out.mag + f0 * N, nlive * N * 4u);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float m = hypotf(X[j].x, X[j].y) * 2.f / (float)(2 * N);
                    if (out.in_db) m = (m > 0.f) ? 20.f * log10f(m) : -FLT_MAX;
                    buf_store_f(r, m, vH * 4, j * T * 4);
                    track(0, m);
                }
            }
            if (out.phase || out.phase_raw) {
                const rsrc_t r = make_rsrc((out.phase_raw ? out.phase_raw : out.phase) + f0 * N, nlive * N * 4u);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float ph = atan2f(X[j].y, X[j].x);
                    if (!out.phase_raw && out.in_deg) ph = ph * 180.f * 0.318309886183790671538f;
                    buf_store_f(r, ph, vH * 4, j * T * 4);
                    if (!out.phase_raw) track(1, ph);
                }
            }
            // Re / Im: output index m <-> bin N + m = conj(bin N - m); the lane holding bin k = t + j T (k >= 1) owns m = N - k, bin N itself is nyq
            if (out.re) {
                const rsrc_t r = make_rsrc(out.re + f0 * N, nlive * N * 4u);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const bool  dc = j == 0 && t == 0;
                    const float v_ = dc ? nyq : X[j].x;
                    buf_store_f(r, v_, (fl * N + (dc ? 0 : N - t - j * T)) * 4, 0); // (no negative scalar offset: the range check sees the lane offset only)
                    track(2, v_);
                }
            }
            if (out.im) {
                const rsrc_t r = make_rsrc(out.im + f0 * N, nlive * N * 4u);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const bool  dc = j == 0 && t == 0;
                    const float v_ = dc ? 0.f : -X[j].y;
                    buf_store_f(r, v_, (fl * N + (dc ? 0 : N - t - j * T)) * 4, 0);
                    track(3, v_);
                }
            }
        } else {
        // ---- every requested output, straight from registers (fft.hpp:164-166, fft_common.hpp:20-56, 91-123)
        // X[j] is bin eN + j ST of the lane's frame; eS + soff(j) is the same bin after fftshift
        constexpr int ST = R4 == 2 ? 256 : T;
        const int     eN = R4 == 2 ? (t >> 1) + 4096 * (t & 1) : fl * N + t;
        const int     eS = R4 == 2 ? (t >> 1) + 4096 * (1 - (t & 1)) : eN;
        auto          soff = [](int j) { return R4 == 2 ? j * ST : (j * ST + HALF) % N; };
        if constexpr (front_bin_sink<FRONT>::value) { // the inverse transform's store (ifft_kernels.hpp): X[j] is then sample eN + j ST, sample (eN - fl N) + j ST of its frame
            front_store_bins<N, ST>(front, X, f0, nlive, eN, R4 == 2 ? eN : t);
        } else {
        if (out.spectrum) {
            const rsrc_t r = make_rsrc(out.spectrum + f0 * N * 2, nlive * N * 8u);
#pragma unroll
            for (int j = 0; j < 16; ++j) buf_store_f2(r, X[j], eN * 8, j * ST * 8);
        }
        if (out.mag2) {
            const rsrc_t r = make_rsrc(out.mag2 + f0 * N, nlive * N * 4u);
            float m[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) m[j] = fmaf(X[j].x, X[j].x, X[j].y * X[j].y);
            if (out.mag2_post.n_ops > 0) ewise_apply<float, 16>(m, out.mag2_post.ops, out.mag2_post.n_ops, out.mag2_post.has_div, [](int) { return 0L; }); // (float programs have no index-dependent op)
            if constexpr (FRONT::kSink) { // the spectrum integrator's sink (specint_kernels.hpp): the values join the lane's leaf sums, nothing is stored
                front.sink(m);
            } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) buf_store_f(r, m[j], eN * 4, j * ST * 4);
            }
        }
        if (!out.real_input) { // N bins; magnitude and phase are fftshift-ed (bin k -> (k + N/2) mod N), Re/Im natural
            if (out.re) {
                const rsrc_t r = make_rsrc(out.re + f0 * N, nlive * N * 4u);
#pragma unroll
                for (int j = 0; j < 16; ++j) { buf_store_f(r, X[j].x, eN * 4, j * ST * 4); track(2, X[j].x); }
            }
            if (out.im) {
                const rsrc_t r = make_rsrc(out.im + f0 * N, nlive * N * 4u);
#pragma unroll
                for (int j = 0; j < 16; ++j) { buf_store_f(r, X[j].y, eN * 4, j * ST * 4); track(3, X[j].y); }
            }
            if (out.mag) {
                const rsrc_t r = make_rsrc(out.mag + f0 * N, nlive * N * 4u);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float m = hypotf(X[j].x, X[j].y) * 2.f / (float)N;
                    if (out.in_db) m = (m > 0.f) ? 20.f * log10f(m) : -FLT_MAX;
                    buf_store_f(r, m, eS * 4, soff(j) * 4);
                    track(0, m);
                }
            }
            if (out.phase || out.phase_raw) {
                const rsrc_t r = make_rsrc((out.phase_raw ? out.phase_raw : out.phase) + f0 * N, nlive * N * 4u);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float ph = atan2f(X[j].y, X[j].x);
                    if (out.phase_raw) {
                        buf_store_f(r, ph, eN * 4, j * ST * 4); // natural order, finished by unwrap_kernel
                    } else {
                        if (out.in_deg) ph = ph * 180.f * 0.318309886183790671538f;
                        buf_store_f(r, ph, eS * 4, soff(j) * 4);
                        track(1, ph);
                    }
                }
            }
        } else { // real input: Re/Im = bins N/2..N-1 (fft.hpp:221-227), magnitude / phase = bins 0..N/2-1, never rotated
            // below 8192 the lane holds bins t + j T: upper half = j >= 8; at 8192 the odd lanes hold the upper half
            const int  eH  = R4 == 2 ? (t >> 1) : fl * HALF + t;
            const bool hi  = R4 == 2 ? (t & 1) != 0 : true, lo = R4 == 2 ? (t & 1) == 0 : true;
            constexpr int J0 = R4 == 2 ? 0 : 8, J1 = R4 == 2 ? 16 : 8; // [J0, 16) upper-half slots, [0, J1) lower-half slots
            if (out.re && hi) {
                const rsrc_t r = make_rsrc(out.re + f0 * HALF, nlive * HALF * 4u);
#pragma unroll
                for (int j = J0; j < 16; ++j) { buf_store_f(r, X[j].x, eH * 4, (j - J0) * ST * 4); track(2, X[j].x); }
            }
            if (out.im && hi) {
                const rsrc_t r = make_rsrc(out.im + f0 * HALF, nlive * HALF * 4u);
#pragma unroll
                for (int j = J0; j < 16; ++j) { buf_store_f(r, X[j].y, eH * 4, (j - J0) * ST * 4); track(3, X[j].y); }
            }
            if (out.mag && lo) {
                const rsrc_t r = make_rsrc(out.mag + f0 * HALF, nlive * HALF * 4u);
#pragma unroll
                for (int j = 0; j < J1; ++j) {
                    float m = hypotf(X[j].x, X[j].y) * 2.f / (float)N;
                    if (out.in_db) m = (m > 0.f) ? 20.f * log10f(m) : -FLT_MAX;
                    buf_store_f(r, m, eH * 4, j * ST * 4);
                    track(0, m);
                }
            }
            if ((out.phase || out.phase_raw) && lo) {
                const rsrc_t r = make_rsrc((out.phase_raw ? out.phase_raw : out.phase) + f0 * HALF, nlive * HALF * 4u);
#pragma unroll
                for (int j = 0; j < J1; ++j) {
                    float ph = atan2f(X[j].y, X[j].x);
                    if (!out.phase_raw && out.in_deg) ph = ph * 180.f * 0.318309886183790671538f;
                    buf_store_f(r, ph, eH * 4, j * ST * 4);
                    if (!out.phase_raw) track(1, ph);
                }
            }
        }
        } // !front_bin_sink
        } // !REAL
        if (out.ranges) { // reduce over the T lanes of the frame: butterflies inside the wave, then (T > 64) through LDS
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
#pragma unroll
                for (int off = (T < 64 ? T : 64) / 2; off > 0; off >>= 1) {
                    rmin[g4] = fminf(rmin[g4], __shfl_xor(rmin[g4], off));
                    rmax[g4] = fmaxf(rmax[g4], __shfl_xor(rmax[g4], off));
                }
            }
            if constexpr (T > 64) {
                __syncthreads(); // everybody is done with buf (the last LDS reads were before the previous barrier, but waves may lag)
                float* red = reinterpret_cast<float*>(buf);
                if ((tid & 63) == 0) {
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) { red[(t >> 6) * 8 + g4] = rmin[g4]; red[(t >> 6) * 8 + 4 + g4] = rmax[g4]; }
                }
                __syncthreads();
                if (t == 0) {
                    for (int w = 1; w < T / 64; ++w)
#pragma unroll
                        for (int g4 = 0; g4 < 4; ++g4) { rmin[g4] = fminf(rmin[g4], red[w * 8 + g4]); rmax[g4] = fmaxf(rmax[g4], red[w * 8 + 4 + g4]); }
                }
                __syncthreads(); // red lives in buf: the next iteration writes there
            }
            if (t == 0 && f0 + fl < n_frames) {
                const bool have[4] = {out.mag != nullptr, out.phase != nullptr, out.re != nullptr, out.im != nullptr};
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    out.ranges[((f0 + fl) * 4 + g4) * 2 + 0] = have[g4] ? rmin[g4] : 0.f;
                    out.ranges[((f0 + fl) * 4 + g4) * 2 + 1] = have[g4] ? rmax[g4] : 0.f;
                }
            }
        }
    }
