/*
 * gr4hip.h -- C-ABI of the MI355X (gfx950) kernel library behind GNU Radio 4's block API.
 *
 * This is the drop-in boundary: plain pointers, sizes and opaque handles; no C++ or torch
 * types; nothing throws across it.  Each entry point replaces the per-block processOne/processBulk arithmetic
 * that gr::Block<>::dispatchProcessing (core/include/gnuradio-4.0/Block.hpp:1848-1917, device seam :1855-1862)
 * would run on the CPU.  The reference has no FFI of its own for this path -- the seam is the inert
 * `compute_domain == "gpu:hip"` hook -- so this header IS the binding a maintainer adds there
 * (INTEGRATION.md shows the stub).  All citations are relative to /root/reference.
 *
 * Conventions
 *   - every function returns gr4hip_status; values -100..0 are gr::work::Status
 *     (core/include/gnuradio-4.0/WorkStatus.hpp:12-41), library errors are < -100.
 *   - `d_*` pointers are device (HBM) pointers on the current device; `stream` is a hipStream_t passed as void*
 *     (NULL = default stream).  Calls are asynchronous on that stream: spans are borrowed until the stream
 *     reaches the end of the enqueued work (Block.hpp:1838-1846 publish/consume ordering is the caller's).
 *   - complex samples are interleaved {re, im}; dtype ids are gr4hip_dtype.
 *   - state that the reference keeps in block members (HistoryBuffer, _accumulated_phase, twiddles, windows)
 *     lives in opaque handles created/destroyed by *_create / *_destroy.
 *   - LIFECYCLE CALLS ARE STREAM-ORDERED WITH THE DATA.  *_reset, *_set_taps, gr4hip_fir_set_prologue / _epilogue, *_set_algo and *_set_guard_mode return at once
 *     and never touch device memory: they note what the handle's device state has to become, and the NEXT *_process call on the handle applies it on the stream
 *     IT is given (hipMemsetAsync / hipMemcpyAsync / a small kernel), in front of its own launches -- hence behind every launch that stream still has in flight
 *     for the handle.  This is the reference's contract: reset() and settingsChanged() run on the block's own worker between two work() calls
 *     (Block.hpp:606, 916-917, 1296; one worker per job list, Scheduler.hpp:1938-1951), so they are ordered with the block's samples by construction.  It holds
 *     on hipStreamNonBlocking streams (gr4hip_stream_create makes those), which the NULL stream does not order against, and needs no device-wide wait.  A caller
 *     that moves a handle from one stream to another orders the two streams itself (gr4hip_event_record + gr4hip_stream_wait_event), as it must for the carried
 *     history anyway.  After a settings change the first process call may hold the HOST until that stream has drained: the new tables go up from pageable memory,
 *     stream-ordered.  Calls that hand a device value back to the host (gr4hip_rotator_phase under the recurrence, gr4hip_iir_status; gr4hip_iir_set_algo and
 *     gr4hip_rotator_set_algo when they have to measure or read something) wait for what they need and say so.  *_create uploads block and are complete on return.
 *   - one handle is driven by one thread at a time (Scheduler.hpp:1938-1951: job lists are disjoint).
 *   - PARITY CONTRACT (stated here once; tests/test_gpu_parity.py::_rel is this formula and every float test uses it): integer, byte and copy results are
 *     bit-exact.  A float32 result y against the float64 evaluation t of the same blocks on the same input satisfies
 *         max_k |y_k - t_k| / max(|t_k|, rms(t)) <= 1e-5
 *     -- the relative error of every value above the rms level of the OUTPUT, the rms-normalised absolute error of every value below it (point-wise relative
 *     error is meaningless at spectral zeros; an all-rms normalisation would ask for better than float32 epsilon on the dominant bin of a quadratic output).
 *     Where the reference's own float32 arithmetic cannot meet that bound (a rejected signal far above the output, an ill-conditioned IIR cascade), the bound is
 *     the reference's float32 error on the same input -- the error of its sums evaluated in float32 in ITS order (time_domain_filter.hpp:44-47, iir section by
 *     section) against float64 -- with a factor of ONE, at every shape (tests and fuzzers compare with the oracle's restatement of exactly that arithmetic, never
 *     with another device kernel).  What keeps the device there: every FIR / decimator kernel answers to one guard -- a segment whose output power is more than
 *     21 dB below what white noise of its input power would pass is evaluated again with float64 products and sums (fir_exact.hip; error ~6e-8 of the output
 *     whatever the signal) --, the fused chain marks such frames and evaluates them again in the time domain behind its launch, and an ill-conditioned IIR
 *     cascade runs on GR4HIP_IIR_SEQUENTIAL_F32.
 */
#ifndef GR4HIP_H
#define GR4HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR4HIP_ABI_VERSION 1 /* cf. gr_plugin_base::abiVersion() == 1, core/include/gnuradio-4.0/Plugin.hpp:20-33 */

typedef enum {
    GR4HIP_OK                  = 0,    /* work::Status::OK */
    GR4HIP_DONE                = -1,   /* work::Status::DONE */
    GR4HIP_INSUFFICIENT_INPUT  = -2,   /* work::Status::INSUFFICIENT_INPUT_ITEMS */
    GR4HIP_INSUFFICIENT_OUTPUT = -3,   /* work::Status::INSUFFICIENT_OUTPUT_ITEMS */
    GR4HIP_ERROR               = -100, /* work::Status::ERROR */
    GR4HIP_INVALID_ARGUMENT    = -101,
    GR4HIP_RUNTIME_ERROR       = -102, /* a HIP runtime call failed; see gr4hip_last_error() */
    GR4HIP_UNSUPPORTED         = -103, /* valid request the device path does not implement (caller keeps the CPU path) */
    GR4HIP_NO_DEVICE           = -104
} gr4hip_status;

typedef enum { /* element types of the reference's block registrations (Math.hpp:25-28, time_domain_filter.hpp:20,213) */
    GR4HIP_U8 = 0, GR4HIP_U16, GR4HIP_U32, GR4HIP_U64, GR4HIP_I8, GR4HIP_I16, GR4HIP_I32, GR4HIP_I64,
    GR4HIP_F32, GR4HIP_F64, GR4HIP_C32, GR4HIP_C64,
    /* gr::UncertainValue<float | double> (meta/.../UncertainValue.hpp:34): an element is the pair {value, uncertainty}, 8 / 16 bytes, laid out like the struct.
     * Taken by the math blocks (gr4hip_math_const / gr4hip_math_nary: both operands carry an uncertainty, uncorrelated propagation as the reference's operators
     * write it, UncertainValue.hpp:121-250: a +- b -> hypot(ua, ub); a * b -> hypot(a ub, b ua); a / b -> hypot(ua / b, ub a / b^2)), by gr4hip_decimate and the
     * ring buffers (any element size).  Not a filter / transform sample type here. */
    GR4HIP_UF32, GR4HIP_UF64
} gr4hip_dtype;

typedef enum { GR4HIP_ADD = 0, GR4HIP_SUB, GR4HIP_MUL, GR4HIP_DIV } gr4hip_op; /* std::plus/minus/multiplies/divides */

typedef enum { GR4HIP_GUARD_STRICT = 0, GR4HIP_GUARD_DEFERRED = 1, GR4HIP_GUARD_OFF = 2 } gr4hip_guard_mode; /* dynamic-range guard: gr4hip_chain_set_guard_mode */

typedef enum { /* gr::filter::IIRForm (time_domain_filter.hpp:50-55) == gr::filter::Form (FilterTool.hpp:107-112) */
    GR4HIP_DF_I = 0, GR4HIP_DF_II, GR4HIP_DF_I_TRANSPOSED, GR4HIP_DF_II_TRANSPOSED
} gr4hip_iir_form;

typedef enum { /* gr::algorithm::window::Type (algorithm/.../fourier/window.hpp:35) */
    GR4HIP_WIN_NONE = 0, GR4HIP_WIN_RECTANGULAR, GR4HIP_WIN_HAMMING, GR4HIP_WIN_HANN, GR4HIP_WIN_HANNEXP,
    GR4HIP_WIN_BLACKMAN, GR4HIP_WIN_NUTTALL, GR4HIP_WIN_BLACKMANHARRIS, GR4HIP_WIN_BLACKMANNUTTALL,
    GR4HIP_WIN_FLATTOP, GR4HIP_WIN_EXPONENTIAL, GR4HIP_WIN_KAISER
} gr4hip_window;

enum { /* FFT block output options (blocks/fourier/.../fft.hpp:103-105) */
    GR4HIP_FFT_OUTPUT_IN_DB  = 1,
    GR4HIP_FFT_OUTPUT_IN_DEG = 2,
    GR4HIP_FFT_UNWRAP_PHASE  = 4
};

typedef enum { /* how the FIR->FFT->mag2 chain is executed */
    GR4HIP_CHAIN_AUTO = 0,
    GR4HIP_CHAIN_UNFUSED,  /* fir kernel -> HBM -> fft+mag2 kernel (any window, any size the FFT block supports: what AUTO takes beyond 8192 points, at sizes that are no power of two
                              and past 256 taps).  Since round 6 the filter runs on float32 products here too (= GR4HIP_CHAIN_TIME_DOMAIN): the 22-bit products of the f16 direct form err
                              COHERENTLY on a tone, and the transform behind the filter gathers that into one bin -- up to 4e-5 of |Y|^2 where a tone 15 dB above the noise is removed by
                              60 dB (tools/dbg/pair_coherent.py), which no power statistic of the filter can see.  44 Gsamples/s at 256 taps x 16384 points (130 on the f16 form) */
    GR4HIP_CHAIN_FUSED_TD, /* one launch: direct-form FIR on the matrix pipe -> window -> FFT -> mag2 (fft_size 256 .. 4096, <= 256 taps); AUTO takes it for <= 64 taps */
    GR4HIP_CHAIN_FUSED_FD, /* one launch, frequency-domain FIR (circular convolution + exact tail correction) + FFT + mag2;
                              fft_size 256 ... 8192 (power of two), <= 256 taps, any window */
    GR4HIP_CHAIN_TIME_DOMAIN /* direct-form FIR kernel with float32 products (GR4HIP_FIR_TIME_DOMAIN_F32) -> HBM -> fft+mag2 kernel: the reference's arithmetic; for
                              inputs whose out-of-band content dwarfs the filtered output (see gr4hip_fir_set_algo), and where the dynamic-range guard sends a stream */
} gr4hip_chain_algo_t;

typedef struct gr4hip_ewise gr4hip_ewise_t; /* a run of per-sample blocks (gr4hip_ewise_* below) */
typedef void* gr4hip_stream_t; /* hipStream_t */
typedef void* gr4hip_event_t;  /* hipEvent_t  */

/* ------------------------------------------------------------------------------------------------ runtime */
int         gr4hip_abi_version(void);
const char* gr4hip_last_error(void); /* thread-local text of the last failure */
/* Developer switches: which of two kernels that compute the same thing serves a call (the tests compare them; tools/ time them).  Each is read from the
 * environment variable of the same name ONCE, when the library is first used, and can be changed afterwards with this call (atomic; process-wide).
 * Nothing here changes the meaning of a call -- choices that do (exact float32 FIR arithmetic, the rotator's phase recurrence, the chain's algorithm and
 * guard) are per-handle settings: gr4hip_fir_set_algo, gr4hip_rotator_set_algo, gr4hip_chain_create / gr4hip_chain_set_guard_mode.
 * Names: GR4HIP_FIR_NO_BF16X3, GR4HIP_FIR_NO_DECIM_FD, GR4HIP_IIR_THREE_PASS, GR4HIP_IIR_LOOKBACK, GR4HIP_IIR_NO_SPLIT, GR4HIP_IIR_SEQ_SLOTS (an integer), GR4HIP_FFT_BLUESTEIN_PIPELINE,
 * GR4HIP_FFT_NO_PIPELINE, GR4HIP_ROTATOR_LEAP, GR4HIP_ROTATOR_WALK, GR4HIP_CHAIN16, GR4HIP_FFT_SMOOTH_RUNTIME, GR4HIP_EWISE_NO_DIV_RCP, GR4HIP_SIGGEN_GAUSS_PERMILLE (an integer:
 * the attempts the Gaussian signal generator launches per 1000 needed pairs, 0 = its own formula; whatever it launches, the values are the same), GR4HIP_INTERP_NO_MFMA (the
 * interpolating FIR stays off the matrix pipe), GR4HIP_INTERP_SPW (an integer: 1 .. 4 segments per workgroup of the interpolating FIR's matrix-pipe kernel, 0 = its own formula),
 * GR4HIP_STFT_GATHER (an integer: 1 = overlapped FFT frames take the gather path also where the hop kernels read them in place, 2 = the hop kernels also for the short
 * calls with a seam that the default sends to the gather path). */
int gr4hip_developer_switch(const char* name, int value);
const char* gr4hip_status_string(int status);
int         gr4hip_device_count(int* count);
int         gr4hip_set_device(int index); /* ComputeDomain "gpu:hip:<index>" (ComputeDomain.hpp:47-100) */
int         gr4hip_get_device(int* index);
int         gr4hip_device_name(int index, char* buf, size_t buflen);

/* "hip" memory provider (the ComputeRegistry::register_provider("hip", fn) resources, ComputeDomain.hpp:105-173) */
int gr4hip_malloc(void** d_ptr, size_t bytes);
int gr4hip_free(void* d_ptr);
int gr4hip_malloc_host(void** h_ptr, size_t bytes); /* pinned host staging */
int gr4hip_free_host(void* h_ptr);
/* A page-locked host RING (round 5): `bytes` of storage (a multiple of the page size) mapped TWICE back to back -- the double mapping of the reference's CircularBuffer
 * (core/include/gnuradio-4.0/CircularBuffer.hpp:75-172: memfd + two mmaps) on the host side of the link, registered with the runtime: base[0 .. 2 bytes) is addressable,
 * base[i] and base[i + bytes] are the same byte, so a span that wraps the physical end is contiguous in virtual memory and the copy engines read / write it in place at the
 * link's rate (measured: 56.2 GB/s inside the mapping, across its end, and from hipHostMalloc memory alike).  What a CPU-domain edge that feeds the device is made of:
 * nothing is ever moved to the front of such an edge. */
int gr4hip_host_ring_create(void** base, size_t bytes);
int gr4hip_host_ring_destroy(void* base, size_t bytes);
int gr4hip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, gr4hip_stream_t stream);
int gr4hip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, gr4hip_stream_t stream);
int gr4hip_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, gr4hip_stream_t stream);
int gr4hip_memset(void* d_dst, int value, size_t bytes, gr4hip_stream_t stream);
int gr4hip_stream_create(gr4hip_stream_t* stream);
int gr4hip_stream_destroy(gr4hip_stream_t stream);
int gr4hip_stream_synchronize(gr4hip_stream_t stream);
int gr4hip_stream_query(gr4hip_stream_t stream, int* idle); /* *idle = 1: everything queued on the stream has finished (hipStreamQuery; never waits) -- one call instead of an event record + query per copy for a caller that keeps one copy in flight per stream (gr::hip::DeviceRun's pieces) */
int gr4hip_event_create(gr4hip_event_t* ev);
int gr4hip_event_destroy(gr4hip_event_t ev);
int gr4hip_event_record(gr4hip_event_t ev, gr4hip_stream_t stream);
int gr4hip_stream_wait_event(gr4hip_stream_t stream, gr4hip_event_t ev); /* work queued on `stream` after this call starts once `ev` has fired */
int gr4hip_event_synchronize(gr4hip_event_t ev);
int gr4hip_event_query(gr4hip_event_t ev, int* done);
int gr4hip_event_elapsed_ms(gr4hip_event_t start, gr4hip_event_t stop, float* ms);

/* GPU-resident double-mapped ring: the device analogue of CircularBuffer's memfd_create + 2x mmap
 * (core/include/gnuradio-4.0/CircularBuffer.hpp:75-172, 191-236): [base, base+size) and [base+size, base+2*size)
 * alias the same HBM, so a reader/writer span never has to be split at the wrap point. */
typedef struct gr4hip_ring gr4hip_ring_t;
int gr4hip_ring_create(gr4hip_ring_t** ring, size_t min_bytes); /* size rounded up to the VMM granularity */
int gr4hip_ring_destroy(gr4hip_ring_t* ring);
int gr4hip_ring_base(const gr4hip_ring_t* ring, void** d_base);
int gr4hip_ring_size(const gr4hip_ring_t* ring, size_t* bytes);

/* ------------------------------------------------------------------------------------------------ a1/a2/a5/a6
 * gr::filter::fir_filter<T>::processOne (blocks/filter/.../time_domain_filter.hpp:44-47):
 *   y[n] = sum_k b[k] x[n-k], zero initial history, history carried across calls (HistoryBuffer.hpp:130-139).
 * dtype F32 (registered) or C32 (complex data x real taps; SURVEY.md Appendix A -- complex taps: gr4hip_cfir_* below).  decim > 1 gives the
 * BasicFilterProto decimating processBulk (:190-204): output m == y[m*decim]; n_in must be a multiple of decim
 * (the reference guarantees it through input_chunk_size = decimate, :166-168). */
/* Decimate by 8 with 97 .. 1025 taps (float, long 16-byte-aligned spans: BASELINE configs[2]'s filter), by 16 with 33 .. 897 and by 32 with 33 .. 641 taps (complex data: by 8 with 64 .. 513, by 16 with 33 .. 449, by 32 with 33 .. 321 taps) run since late round 4 on the f16 matrix pipe with the arithmetic and
 * the safeguards described below for the non-decimating filters (csrc/fir_decim_f16.hip: block exponent per segment of 1024 outputs, per-segment verdict, second evaluation with
 * three-term f16 products, float32 sums for segments with a non-finite sample or a spread beyond 2^28): error relative to the OUTPUT, the call asynchronous.  The
 * frequency-domain kernel of rounds 1-3 (error floor relative to the input, strict host-side guard) is what GR4HIP_FIR_IIR_ONE_LAUNCH fuses the cascade into. */
/* Non-finite and near-FLT_MAX samples (pinned by tests/test_gpu_parity.py::test_fir_non_finite_samples / test_fir_f16_kernel_outliers_and_non_finite_samples /
 * test_chain_non_finite_samples).  The reference's transform_reduce gives +-Inf / NaN on exactly the ntaps outputs whose window contains such a sample.  With the
 * default algorithm:
 *  - 33 .. 256 taps (float and complex; as slices of 256 taps that add into y: float up to 3840, complex up to 1792 taps) on long 16-byte-aligned spans evaluate the products on the f16 matrix pipe, samples and taps split
 *    into two f16 terms under a block exponent per segment of 4096 (complex: 2048) outputs (csrc/fir_f16.hip; same 1e-5 parity bar).  A segment that holds a
 *    non-finite sample is evaluated as plain float32 sums instead: the reference's classes (+Inf, -Inf, NaN) on exactly its outputs; a finite outlier more than
 *    2^28 above the segment's ordinary level (1e30 or 3.4e38 beside unit-power samples, a burst that ends inside the segment) sends its segment to float32 products on the f32 matrix pipe, so the
 *    samples beside it keep their accuracy.  (GR4HIP_FIR_TIME_DOMAIN_BF16X3, the three-term bf16 kernels of rounds 2-3: every output the reference makes
 *    non-finite is non-finite, as NaN, the reach is the kernel's 32-sample-granular window -- at most 15 outputs earlier and 46 later than the reference's --,
 *    and a finite sample above bf16's largest value, 3.39e38, counts as infinite.)
 *  - complex data, 97 .. 256 taps, spans of >= 64 x 8192 samples take a fast-convolution kernel: a non-finite sample reaches every output of its 8192-sample
 *    block (and of the next block when it lies within the block's last 255 samples) instead of the next ntaps outputs.
 * gr4hip_fir_set_algo(GR4HIP_FIR_EXACT_F32) selects, per handle, kernels whose classes (+Inf, -Inf, NaN) and reach are the reference's exactly. */
typedef struct gr4hip_fir gr4hip_fir_t;
int gr4hip_fir_create(gr4hip_fir_t** fir, int dtype, const float* h_taps, size_t ntaps, size_t decim);
int gr4hip_fir_set_taps(gr4hip_fir_t* fir, const float* h_taps, size_t ntaps); /* settingsChanged (:38-42): history is kept */
int gr4hip_fir_reset(gr4hip_fir_t* fir);
/* GR4HIP_FIR_AUTO (default): since round 4 complex data with 33 .. 256 taps takes the f16 direct form on 16-byte-aligned spans (error relative to the output, see
 * below); long complex spans that are only 8-byte aligned (97 .. 256 taps) take the fast-convolution kernel.  Its float32 error floor is ~2e-6 of the INPUT rms per output sample
 * (three transforms' worth of rounding), the direct form's ~2e-7: when out-of-band signals that the filter removes are much stronger than what it
 * passes, GR4HIP_FIR_TIME_DOMAIN keeps the error relative to the OUTPUT inside the 1e-5 parity bar (the reference's own arithmetic, 1024 flop/sample). */
/* FIR_AUTO carries the same dynamic-range guard as GR4HIP_CHAIN_AUTO (gr4hip_chain_last_power_ratio below): the first fast convolution of a stream is probed
 * on eight frames, later ones are watched through the powers every launch measures (every frame judged by itself), and below an output / input power ratio of
 * 0.04 the direct form takes over. */
/* Accuracy of the direct form on the matrix pipes (the default for 33 .. 3840 taps -- complex: .. 1792 -- and the decimators; GR4HIP_FIR_TIME_DOMAIN for complex data).  Two-term f16
 * splits under a per-segment block exponent, three products per tap (everything above 2^-22 of a product; a correctly rounded float32 product carries 2^-25): on
 * ordinary input the error against float64 is that of a float32 sum (3e-7 .. 6e-7).  The error is relative to the PRODUCTS, so it shows against the OUTPUT when the
 * filter removes nearly all it is given -- like the reference's own float32 sum, whatever its order.  ONE guard for every kernel gr4hip_fir_process can take (round 5):
 * each segment's output power P_y is compared with its input power P_x, and a segment with D P_y < (sum b^2 / 128) P_x (21 dB more rejected than white noise would lose;
 * the split products are then at <= 6e-6 of the output; the f16 decimators mark at sum b^2 / 64 since round 6: a tone in a long filter's transition band left 9e-6) is marked and evaluated again with float64 products and sums, rounded once -- by fir_exact_kernel on the FP64
 * matrix pipe behind the launch (same stream, no host), inside the workgroup for the register-window kernel, with the filter's load / store programs applied where it
 * carries any.  Result: within 1e-5 of float64 on every stream tools/tone_ratio.py, tools/fuzz_fir_f16.py and the tests could construct (rejected tones up to 70 dB
 * above what passes: 6e-8), where the reference's float32 sum itself is at 1e-5 .. 1e-3.  A stream in which EVERY segment is marked runs at the FP64 matrix pipe's
 * rate (measured, profiles/r05_rejected_stream_rates.txt: float 256 taps 264 Gsamples/s against 518 unmarked, complex 143 against 178, decimate-by-8 with 1024 taps 417 against 749).  gr4hip_fir_set_guard_mode(GR4HIP_GUARD_OFF) switches the verdict off (the kernels' own products).
 * Non-finite samples: a segment whose window holds one keeps the main kernel's float32 sums (the reference's classes and reach). */
/* GR4HIP_FIR_TIME_DOMAIN_BF16X3: the three-term bf16 products of rounds 2-3 (six products per tap, everything above 2^-23 of a product, float32's exponent range
 * without a block exponent; judged like every kernel) where the default takes the f16 kernels; for complex data also "direct form" like GR4HIP_FIR_TIME_DOMAIN. */
/* GR4HIP_FIR_EXACT_F32: every product and sum in IEEE float32 (no frequency-domain kernels, no bf16 splits): the kernels whose arithmetic is the reference's
 * transform_reduce (time_domain_filter.hpp:44-47) term for term up to the order of the additions -- an infinite or NaN input sample reaches exactly the
 * ntaps outputs whose window contains it, as +-Inf / NaN (tests/test_gpu_parity.py::test_fir_non_finite_samples pins this and what the default algorithm
 * does instead).  Slower for 33 .. 1024 taps (the f32 MFMA / register-window kernels: DESIGN.md 3.2, 3.6). */
/* GR4HIP_FIR_TIME_DOMAIN_F32: the direct form with float32 products on the f32 matrix pipe (block-wise float32 sums: at least as close to float64 as the
 * reference's sequential float32 sum -- 7e-6 of the output where a rejected signal 50 dB above it leaves the float32 CPU form at 3e-5 and the three-term bf16
 * products at 1e-4), 33 .. 256 taps at about a third of the bf16 kernels' rate; Inf / NaN reach as described above.  Judged like every kernel (above). */
typedef enum { GR4HIP_FIR_AUTO = 0, GR4HIP_FIR_TIME_DOMAIN = 1, GR4HIP_FIR_EXACT_F32 = 2, GR4HIP_FIR_TIME_DOMAIN_F32 = 3, GR4HIP_FIR_TIME_DOMAIN_BF16X3 = 4 } gr4hip_fir_algo;
int gr4hip_fir_set_algo(gr4hip_fir_t* fir, int algo);
int gr4hip_fir_set_guard_mode(gr4hip_fir_t* fir, int mode); /* gr4hip_guard_mode (below), for FIR_AUTO's fast convolution of long complex spans and (GUARD_OFF) the f16 direct form's per-segment verdict; default GR4HIP_GUARD_STRICT */
int gr4hip_fir_process(gr4hip_fir_t* fir, const void* d_in, size_t n_in, void* d_out, size_t* n_out, gr4hip_stream_t stream);
int gr4hip_fir_destroy(gr4hip_fir_t* fir);

/* Interpolating FIR (BASELINE.json north_star "decimating / interpolating FIR").  The reference has no such block, only the rate declaration
 * it would carry, Resampling<1, L> (core/include/gnuradio-4.0/annotated.hpp:121-128; chunk bookkeeping Block.hpp:1576-1636), so the definition is
 * SURVEY.md Appendix A's: zero-stuff by `interp`, then fir_filter's sum at the output rate, gain `interp`:
 *   u[n] = x[n / L] if n % L == 0 else 0,   y[n] = L sum_k b[k] u[n - k]   ==   y[m L + p] = sum_q (L b[q L + p]) x[m - q]   (polyphase, evaluated)
 * n_out = n_in * interp; zero initial history, ceil(ntaps / interp) - 1 input samples carried across calls; dtype F32 or C32 (real taps).
 * Parity is pinned by the project's own float64 oracle (gr4o_fir_interp_*: literal zero-stuffing + the a1 sum), not by the reference. */
typedef struct gr4hip_fir_interp gr4hip_fir_interp_t;
int gr4hip_fir_interp_create(gr4hip_fir_interp_t** fir, int dtype, const float* h_taps, size_t ntaps, size_t interp);
int gr4hip_fir_interp_set_taps(gr4hip_fir_interp_t* fir, const float* h_taps, size_t ntaps); /* history kept unless it must grow (like fir_filter) */
int gr4hip_fir_interp_reset(gr4hip_fir_interp_t* fir);
int gr4hip_fir_interp_process(gr4hip_fir_interp_t* fir, const void* d_in, size_t n_in, void* d_out, size_t* n_out, gr4hip_stream_t stream);
int gr4hip_fir_interp_destroy(gr4hip_fir_interp_t* fir);

/* Rational resampler: polyphase FIR at rate interp / decim = L / M (RATIONAL_RESAMPLER.md).  The reference has no such block, only the rate machinery one would
 * declare (Resampling<inputChunk, outputChunk>), so the definition is the project's, pinned by its own float64 oracle (tests/rational_resampler_oracle.py).  Real taps
 * b[0 .. K), data F32 or C32, zero initial history; L and M need not be coprime, the definition is literal:
 *   u[n] = x[n / L] if n % L == 0 else 0,   v[n] = L sum_k b[k] u[n - k]   (the interpolator's definition above),   y[j] = v[j M]
 * evaluated, with Kp = ceil(K / L) and j = c L + p (cycle c, slot p < L), o_p = floor(p M / L), phi_p = (p M) mod L, as
 *   y[c L + p] = sum_{q = 0}^{Kp - 1} w_p[q] x[c M + o_p - q],   w_p[q] = float(L) b[q L + phi_p]   (one float32 rounding; 0 where q L + phi_p >= K)
 * in float32 from 0 with q ascending, one fmaf per term and component, every slot summing all Kp terms (the zero-padded ones included).  There are no split products
 * and no guard: this is the GR4HIP_FIR_EXACT_F32 class of arithmetic.
 *  - n_in must be a multiple of M, n_out = n_in / M * L.  A call consumes whole cycles and always restarts at slot 0: no phase is carried, only the last Kp - 1 inputs
 *    (capacity max(32, bit_ceil(Kp)), like the interpolator).
 *  - Output values do not depend on how a stream is cut into calls, bit for bit: every output's sum has one fixed order.
 *  - M == 1 computes the interpolator's definition, L == 1 the decimating fir_filter's y[m M].
 *  - A non-finite input at position pos reaches exactly the outputs with c M + o_p - Kp < pos <= c M + o_p, as IEEE arithmetic gives them.
 * Supported: F32 and C32, 1 <= interp, decim <= 1024, 1 <= ntaps <= 65536 (beyond: GR4HIP_UNSUPPORTED).  NULL handle, taps or buffers, ntaps, interp or decim == 0, a
 * non-finite tap, n_in % decim != 0, overlapping buffers, buffers not aligned to the element size: GR4HIP_INVALID_ARGUMENT before any device work.  n_in == 0 is a
 * no-op.  set_taps keeps the history unless it must grow; another L or M needs a new handle.  gr4hip_resamp_tile(): output cycles per workgroup.
 * gr4hip_resamp_design (host code, no device; h_out == NULL: *ntaps only): the windowed-sinc low-pass in front of the rate change, float64 rounded once:
 *   K = 2 half_len max(L, M) + 1,  fc = 0.4 / max(L, M) cycles per sample of the L-times rate,  h[k] = w_K[k] 2 fc sinc(2 fc (k - (K - 1) / 2)),  h /= sum h
 * with w = gr4hip_window_create_f64(window, ., K, beta). */
typedef struct gr4hip_resamp gr4hip_resamp_t;
int    gr4hip_resamp_create(gr4hip_resamp_t** rs, int dtype, const float* h_taps, size_t ntaps, size_t interp, size_t decim);
int    gr4hip_resamp_set_taps(gr4hip_resamp_t* rs, const float* h_taps, size_t ntaps);
int    gr4hip_resamp_reset(gr4hip_resamp_t* rs);
int    gr4hip_resamp_process(gr4hip_resamp_t* rs, const void* d_in, size_t n_in, void* d_out, size_t* n_out /* may be NULL */, gr4hip_stream_t stream);
int    gr4hip_resamp_destroy(gr4hip_resamp_t* rs);
size_t gr4hip_resamp_tile(void);
int    gr4hip_resamp_design(float* h_out, size_t cap, size_t* ntaps, size_t interp, size_t decim, size_t half_len, int window, double beta);

/* Complex-tap FIR for complex streams, direct and decimating (SURVEY.md Appendix A lists the "complex-tap variant as an option"; COMPLEX_FIR.md).  The reference has
 * no such block -- its fir_filter is `requires std::floating_point<T>` -- so it does not pin parity here: the definition below is the project's, and the project's own
 * float64 oracle (tests/complex_fir_oracle.py) pins it:
 *   y[n] = sum_{k < ntaps} b[k] x[n - k],   b and x complex<float> (h_taps: ntaps interleaved {re, im}), every complex product as four real products;
 *   decim D: output m = y[m D], n_in a multiple of D, n_out = n_in / D.  Zero initial history, the last ntaps - 1 inputs carried across calls.
 * 1 <= ntaps <= 2048, 1 <= decim <= 64 (beyond: GR4HIP_UNSUPPORTED).  NULL taps, ntaps == 0, decim == 0, a non-finite tap, n_in % decim != 0, overlapping or not
 * 8-byte-aligned buffers: GR4HIP_INVALID_ARGUMENT before any device work.  17 .. 1024 taps at decim <= 16 run on the f32 matrix pipe in tile groups of
 * gr4hip_cfir_tile() outputs (exact float32 products; the tap operand of that form is what gr4hip_cfir_band_table returns: [n_steps][16][16] floats, step r_min first;
 * h_out == NULL: sizes only; host code, no device), everything else and the ragged tail as IEEE float32 multiply-adds.  The guard is the FIR family's one rule
 * (above): per segment of gr4hip_cfir_segment() outputs, D P_y < (sum |b|^2 / 128) P_x or a non-finite sample in the segment's window marks it, and marked segments are
 * evaluated again as float64 sums in ascending k, rounded once, behind the launch on the same stream.  Guard modes: GR4HIP_GUARD_STRICT (default) or GR4HIP_GUARD_OFF
 * (no marking, no second evaluation); GR4HIP_GUARD_DEFERRED: GR4HIP_UNSUPPORTED. */
typedef struct gr4hip_cfir gr4hip_cfir_t;
int    gr4hip_cfir_create(gr4hip_cfir_t** fir, const float* h_taps, size_t ntaps, size_t decim);
int    gr4hip_cfir_set_taps(gr4hip_cfir_t* fir, const float* h_taps, size_t ntaps); /* history kept unless it must grow (like fir_filter) */
int    gr4hip_cfir_reset(gr4hip_cfir_t* fir);
int    gr4hip_cfir_set_guard_mode(gr4hip_cfir_t* fir, int mode);
int    gr4hip_cfir_process(gr4hip_cfir_t* fir, const void* d_in, size_t n_in, void* d_out, size_t* n_out /* may be NULL */, gr4hip_stream_t stream);
int    gr4hip_cfir_destroy(gr4hip_cfir_t* fir);
size_t gr4hip_cfir_tile(void);    /* complex outputs per MFMA tile group of one workgroup */
size_t gr4hip_cfir_segment(void); /* complex outputs per guard segment */
int    gr4hip_cfir_band_table(const float* h_taps, size_t ntaps, size_t decim, float* h_out, size_t cap, size_t* n_steps, long* r_min);

/* gr::filter::Decimator<T>::processBulk (time_domain_filter.hpp:234-244): keep samples with i % decim == 0. */
int gr4hip_decimate(int dtype, const void* d_in, size_t n_in, size_t decim, void* d_out, size_t* n_out, gr4hip_stream_t stream);

/* ------------------------------------------------------------------------------------------------ a3/a4
 * gr::filter::Filter<float>::processOne == cascade of sections through detail::computeFilter
 * (algorithm/.../filter/FilterTool.hpp:116-158, 244-246), and gr::filter::iir_filter<float, form>::processOne
 * (time_domain_filter.hpp:89-121) for nsections == 1.  b: [nsections][nb], a: [nsections][na]; a[.][0] is taken as 1 whatever it holds (computeFilter never
 * reads it: nothing is divided by it).  d_in[0 .. n) and d_out[0 .. n) must not overlap: the cascade does not run in place (GR4HIP_INVALID_ARGUMENT, nothing enqueued).
 * All four forms compute the same transfer function from zero state and are EVALUATED as direct form II (the parallel-in-time scan works on the DF-II
 * state); `form` is recorded for introspection only, so rounding can differ from the reference's DF_I / transposed forms in the last bits (the four forms
 * agree to 1e-5 upstream too, qa_filter.cpp:53-128).
 * Evaluation: when the cascade's memory fades within 1, 2 or 4 tiles of 8192 samples (||Phi^tiles||_inf <= 1e-8, checked in float64 at create), a span is cut
 * into contiguous runs of tiles that start from a warm-up over the preceding tiles instead of the exact state: the state a run starts from is within 1e-8
 * (relative to the state that far back) of the exact one -- three orders below the float32 parity tolerance; the first run of every call starts from the
 * handle's carried state exactly.  Filters that fade more slowly (poles within ~5e-4 of the unit circle) take the exact look-back scan.
 * gr4hip_iir_status: synchronises `stream` and reports a look-back time-out of an earlier launch of this handle (a bounded wait gave up: never observed,
 * but then that call's output is invalid) as GR4HIP_RUNTIME_ERROR; the next process / reset call reports it too. */
typedef struct gr4hip_iir gr4hip_iir_t;
int gr4hip_iir_create(gr4hip_iir_t** iir, int form, size_t nsections, const float* h_b, size_t nb, const float* h_a, size_t na);
int gr4hip_iir_reset(gr4hip_iir_t* iir);
int gr4hip_iir_process(gr4hip_iir_t* iir, const float* d_in, size_t n, float* d_out, gr4hip_stream_t stream);
int gr4hip_iir_status(gr4hip_iir_t* iir, gr4hip_stream_t stream);
/* How the cascade is evaluated (per handle; changing it restarts the filter from zero state):
 *   GR4HIP_IIR_PARALLEL        the parallel-in-time kernels described above (direct form II whatever `form` says).
 *   GR4HIP_IIR_SEQUENTIAL_F32  the reference's own arithmetic: one lane walks the cascade sample by sample in the REQUESTED form (detail::computeFilter,
 *                              FilterTool.hpp:116-158: DF_I / DF_II / DF_I_TRANSPOSED / DF_II_TRANSPOSED with their own input / output histories), float32
 *                              operations in source order.  ~10 Msamples/s; as close to float64 as the block on the host, form for form.
 *   GR4HIP_IIR_AUTO (default)  PARALLEL unless float32 cannot carry this cascade's state through the scan: gr4hip_iir_create measures it -- a three-tile noise vector
 *                              through the kernels the handle would use, against float64 and against the sequential float32 form on the host -- and selects
 *                              SEQUENTIAL_F32 when the parallel result is off by more than 1e-5 of the output rms AND by more than ten times the sequential float32
 *                              error (ill-conditioned narrow-band cascades of high order: an order-16, fc = 0.016 Butterworth measured 7.8e-2 against 7.0e-3).
 * gr4hip_iir_get_algo reports the evaluation in use and the two create-time errors (max |error| / output rms; < 0: not measured). */
typedef enum { GR4HIP_IIR_AUTO = 0, GR4HIP_IIR_PARALLEL = 1, GR4HIP_IIR_SEQUENTIAL_F32 = 2 } gr4hip_iir_algo;
int gr4hip_iir_set_algo(gr4hip_iir_t* iir, int algo);
int gr4hip_iir_get_algo(const gr4hip_iir_t* iir, int* algo_in_use, float* selftest_parallel, float* selftest_sequential_f32);
int gr4hip_iir_destroy(gr4hip_iir_t* iir);

/* BasicDecimatingFilter (FIR design) -> BasicFilter (IIR design), BASELINE.json configs[2]: the decimating processBulk loop (time_domain_filter.hpp:190-204) feeding
 * Filter<float>::processOne over the sections (FilterTool.hpp:244-246).  One call for both handles; each keeps its own state (history, delay lines) exactly as if
 * gr4hip_fir_process and gr4hip_iir_process were called one after the other, and the two may be mixed freely with those calls.
 * mode GR4HIP_FIR_IIR_ONE_LAUNCH: when the filter takes the frequency-domain decimator (float, decimate by 8, <= 1024 taps, a span of >= 64 blocks of 7168 samples) and
 * the cascade is up to four biquads on the parallel path whose memory fades within four blocks, the cascade runs as the decimator's STORE EPILOGUE: one launch, the
 * decimated stream never reaches HBM (4.5 instead of 5.5 bytes per input sample) -- contiguous block runs per workgroup, the cascade's state carried in one wave,
 * every run but the first warmed up over the blocks in front of it (state error <= 1e-8); anything else runs as the two launches.
 * mode GR4HIP_FIR_IIR_TWO_LAUNCHES: the decimated stream through a scratch buffer of the filter handle.
 * mode GR4HIP_FIR_IIR_AUTO: the faster of the two as measured on MI355X -- the two launches (the decimator is bound by vector-instruction issue, not by HBM: the
 * cascade's instructions cost the same inside its launch as in their own, and the contiguous runs cost the decimator another 10 %; DESIGN.md 7 has the numbers).
 * ONE_LAUNCH is for a caller that shares HBM bandwidth with other streams and prefers the smaller traffic.
 * The decimator's dynamic-range guard works as in gr4hip_fir_process (a rejected span is redone on the polyphase kernels + the cascade's own, from untouched states). */
typedef enum { GR4HIP_FIR_IIR_AUTO = 0, GR4HIP_FIR_IIR_ONE_LAUNCH = 1, GR4HIP_FIR_IIR_TWO_LAUNCHES = 2 } gr4hip_fir_iir_mode;
int gr4hip_fir_iir_process(gr4hip_fir_t* fir, gr4hip_iir_t* iir, const float* d_in, size_t n_in, float* d_out, size_t* n_out, int mode, gr4hip_stream_t stream);

/* ------------------------------------------------------------------------------------------------ a5 (host-side design)
 * BasicFilterProto<float>::designFilter (time_domain_filter.hpp:163-182): FIR by window method
 * (fir::designFilter<float>, FilterTool.hpp:964-1071; tap count from Kaiser's estimate :985-1004) or IIR biquad
 * sections (iir::designFilter<float>, :476-917).  Pure host code; results feed gr4hip_fir_create / gr4hip_iir_create. */
typedef struct { /* gr::filter::FilterParameters (FilterTool.hpp:66-75) */
    size_t order;
    double f_low, f_high, gain, ripple_db, attenuation_db, beta, fs;
} gr4hip_filter_params;
typedef enum { GR4HIP_LOWPASS = 0, GR4HIP_HIGHPASS, GR4HIP_BANDPASS, GR4HIP_BANDSTOP } gr4hip_filter_response; /* filter::Type :64 */
typedef enum { GR4HIP_BUTTERWORTH = 0, GR4HIP_BESSEL, GR4HIP_CHEBYSHEV1, GR4HIP_CHEBYSHEV2 } gr4hip_iir_design_t; /* iir::Design :425-430 */
int gr4hip_filter_params_default(gr4hip_filter_params* p);
/* h_taps == NULL: only *ntaps is returned (size query) */
int gr4hip_fir_design(int response, const gr4hip_filter_params* p, int window, float* h_taps, size_t cap, size_t* ntaps);
/* biquads: h_b, h_a are [cap_sections][3] (first-order sections are zero padded) */
int gr4hip_iir_design(int response, const gr4hip_filter_params* p, int design, float* h_b, float* h_a, size_t cap_sections, size_t* nsections);

/* ------------------------------------------------------------------------------------------------ a7-a10
 * gr::blocks::fft::FFT<T>::processBulk (blocks/fourier/.../fft.hpp:147-171) per frame of fft_size samples:
 * window (window.hpp:69-183, default Hann) -> forward DFT (algorithm/.../fourier/fft.hpp:113-153) ->
 * magnitude hypot*2/N [dB] fft-shifted + phase atan2 [unwrap][deg] fft-shifted (fft_common.hpp:20-123) + Re + Im
 * (natural order, fft.hpp:217-220).  in_dtype C32: fft_size values per output; F32: fft_size/2 (fft.hpp:140-143, 221-227).
 * Any output pointer may be NULL.  d_ranges (optional): per frame {min,max} of mag, phase, re, im (fft.hpp:229-232).
 * fft_size: any power of two up to 2^20 (one kernel up to 8192, a four-step pipeline above) and every other size up to 2^19 -- the
 * sizes SimdFFT takes with radix-3/5 passes (SimdFFT.hpp:348-375) and the ones the reference sends to Bluestein
 * (algorithm/.../fourier/fft.hpp:353-381) alike run as a chirp convolution over the power-of-two transforms; larger sizes return
 * GR4HIP_UNSUPPORTED from create (the caller keeps its CPU path). */
typedef struct gr4hip_fft gr4hip_fft_t;
int gr4hip_fft_create(gr4hip_fft_t** fft, int in_dtype, size_t fft_size, int window, int flags);
int gr4hip_fft_process(gr4hip_fft_t* fft, const void* d_in, size_t n_frames, float* d_mag, float* d_phase, float* d_re, float* d_im,
                       float* d_ranges, gr4hip_stream_t stream);
/* raw spectrum of algorithm::FFT::compute (interleaved complex, natural order, window applied if configured) */
int gr4hip_fft_spectrum(gr4hip_fft_t* fft, const void* d_in, size_t n_frames, float* d_spectrum, gr4hip_stream_t stream);
/* |X[k]|^2 in natural bin order: mag2[(k + N/2) % N] == (magnitude_block[k] * N/2)^2 */
int gr4hip_fft_mag2(gr4hip_fft_t* fft, const void* d_in, size_t n_frames, float* d_mag2, gr4hip_stream_t stream);
/* Per-sample float blocks BEHIND a power spectrum (MultiplyConst / DivideConst / AddConst / SubtractConst<float> on the |X|^2 stream: normalisation, an offset) in the
 * transform's launch: the program (gr4hip_ewise_t of dtype F32, copied; NULL or empty removes it) is applied to every |X|^2 value of gr4hip_fft_mag2 before its store --
 * natively in every transform kernel of the FFT block (one launch); the 8192-point frame pipeline runs it as one element-wise launch over its output inside the call. */
int gr4hip_fft_set_epilogue(gr4hip_fft_t* fft, const gr4hip_ewise_t* f32_prog);
int gr4hip_fft_destroy(gr4hip_fft_t* fft);
/* Which device path a size takes (host-only, no device needed): kind 0 = power of two <= 8192 (one kernel), 3 = {2,3,5}-smooth <= 8192 (mixed-radix passes in one
 * launch: the sizes SimdFFT::canProcessSize takes with radix-3 / radix-5 passes, SimdFFT.hpp:348-375; radices[0 .. n_passes) is the run-time plan, <= 15 passes of
 * radix 2 .. 16), 1 = power of two up to 2^20 (four-step), 2 = any other size up to 2^19 (chirp convolution); GR4HIP_UNSUPPORTED beyond. */
int gr4hip_fft_plan(size_t fft_size, int* kind, int* radices16, int* n_passes);
/* window::create on the host (float), for callers that need the block's _window member */
int gr4hip_window_create(int window, float* h_out, size_t n, float beta);
int gr4hip_window_create_f64(int window, double* h_out, size_t n, double beta); /* create<double> */

/* Polyphase filter bank in front of the FFT block's transform: PFB spectrometer and channelizer (critically sampled analysis bank, PFB.md).  The reference has no
 * polyphase form, so it does not pin parity here: the definition below is the project's, and the project's own float64 oracle
 * (tests/pfb_oracle.py) pins it.  N channels, P taps per channel, prototype h[0 .. P N) (real), input x complex<float>, zero initial history:
 *   u_m[i] = sum_{k < P} h[k N + i] x[(m - P + 1 + k) N + i]   (float32, k ascending, one fma per term and component; x[n] = 0 for n < 0)
 *   X_m[c] = sum_{i < N} u_m[i] e^{-2 pi i i c / N}            (the FFT block's unnormalised forward transform)
 *   d_spectrum[m][c] = X_m[c] (interleaved complex, natural bin order), d_mag2[m][c] = |X_m[c]|^2; either may be NULL, not both.
 * Frame m leaves when input frame m has arrived (latency (P - 1) N samples); the last (P - 1) N samples are carried across calls in the handle, so the values do
 * not depend on how a stream is cut into calls.  With P = 1 and h = a window the outputs are those of gr4hip_fft_spectrum / gr4hip_fft_mag2.  Non-finite samples
 * propagate as float arithmetic does (the P frames whose window holds one); there is no guard, the sums have no cancelling tier.
 * gr4hip_pfb_design (host code, no device): h[j] = w_{PN}[j] sinc((j - (P N - 1) / 2) / N), w = gr4hip_window_create_f64(window, ., P N, beta), evaluated in
 * float64 and rounded once; no other normalisation.  gr4hip_pfb_create: h_taps = P N values, NULL = that design with the Hamming window; flags must be 0.
 * gr4hip_pfb_set_taps keeps the history; it and gr4hip_pfb_reset (history back to zeros) are stream-ordered (LIFECYCLE CALLS above).
 * Supported: in_dtype C32; n_channels a size of gr4hip_fft_plan kind 0 (a power of two <= 8192); 1 <= taps_per_channel <= 32.  GR4HIP_UNSUPPORTED (the caller
 * keeps its own path): F32 input, other sizes, more than 32 taps per channel.  GR4HIP_INVALID_ARGUMENT before any device work: a NULL handle or input, fewer than 2
 * channels, 0 taps per channel, a non-finite tap, count != P N, both outputs NULL, d_in / d_spectrum not aligned to 8 bytes or d_mag2 not to 4, an output that
 * overlaps the input, more than 2^40 samples in one call (below 256 channels: more than 2^31 - 1 workgroups of 64 / max(1, N / 8) frames).  n_frames == 0 is a no-op. */
typedef struct gr4hip_pfb gr4hip_pfb_t;
int gr4hip_pfb_design(float* h_out, size_t n_channels, size_t taps_per_channel, int window, float beta);
int gr4hip_pfb_create(gr4hip_pfb_t** pfb, int in_dtype, size_t n_channels, size_t taps_per_channel, const float* h_taps /* P N values, or NULL */, int flags);
int gr4hip_pfb_set_taps(gr4hip_pfb_t* pfb, const float* h_taps, size_t count);
int gr4hip_pfb_reset(gr4hip_pfb_t* pfb);
int gr4hip_pfb_process(gr4hip_pfb_t* pfb, const void* d_in, size_t n_frames, float* d_spectrum, float* d_mag2, gr4hip_stream_t stream);
int gr4hip_pfb_destroy(gr4hip_pfb_t* pfb);

/* Inverse transform and polyphase synthesis bank (INVERSE_FFT.md): from frames of N complex bins in natural order (what gr4hip_fft_spectrum and
 * gr4hip_pfb_process(d_spectrum) write) back to samples.  N a size of gr4hip_fft_plan kind 0 (a power of two, 2 <= N <= 8192).
 *   C2C (out_dtype C32):  x[n] = sum_{k < N} X[k] e^{+2 pi i k n / N}                                                            [frames][N] complex out
 *   C2R (out_dtype F32):  x[n] = Re X[0] + (-1)^n Re X[N/2] + 2 sum_{k = 1}^{N/2 - 1} Re( X[k] e^{+2 pi i k n / N} )             [frames][N] float out
 * Unnormalised, like the reference's Direction::Backward (algorithm/.../fourier/fft.hpp:260-314); GR4HIP_IFFT_SCALE multiplies every output by 1 / N, once, as
 * the last operation of the transform (exact for these N, barring underflow).  C2R reads full N-bin frames and uses bins 0 .. N/2 only: the imaginary parts of
 * bins 0 and N/2 and every bin above N/2 are ignored, as trySimdFFT_C2R packs them (fft.hpp:277-283).  window (ids as in gr4hip_fft_create; NONE: no multiply):
 * x[n] times gr4hip_window_create(window, ., N, 1.6)[n] after the scale, one float multiply per component.  Non-finite values propagate as float arithmetic
 * gives them; there is no guard.  The values are conj(forward transform(conj X)) of the FFT block's kernels, bit for bit.  Oracles (tests/synthesis_oracle.py):
 * N numpy.fft.ifft, and N numpy.fft.irfft of bins 0 .. N/2 with the two imaginary parts zeroed.
 *
 * Synthesis bank (the project's own definition, as the analysis bank's is): N channels, P taps per channel, prototype g[0 .. P N) (real), frames of spectra Y_m,
 *   v_m[i]    = sum_{c < N} Y_m[c] e^{+2 pi i i c / N}          (the C2C transform above; v_m = 0 for m < 0, or the carried history)
 *   y[m N + i] = sum_{k < P} g[k N + i] v_{m - k}[i]            (float32, from y = 0, k ascending, one fma per term and component)
 * N values in, N samples out per frame; the last P - 1 frames of v (float32, after the transform and its optional 1 / N) are carried in the handle, so the
 * values do not depend on how the frame stream is cut into calls.  With P = 1 and g = a window the outputs are those of gr4hip_ifft_process with that window.
 * With g = h the bank is the adjoint of gr4hip_pfb_process with prototype h, delayed by P - 1 frames; it is NOT a reconstruction of the analysis bank's input
 * (INVERSE_FFT.md).  h_taps NULL: gr4hip_pfb_design(N, P, Hamming).  gr4hip_pfb_synth_set_taps keeps the history; it and gr4hip_pfb_synth_reset (history back to
 * zeros) are stream-ordered (LIFECYCLE CALLS above).  A non-finite value in Y_m reaches every sample of output frames m .. m + P - 1 and nothing else.
 * GR4HIP_INVALID_ARGUMENT before any device work, outputs untouched: a NULL handle, input or output, fft_size / n_channels < 2, 0 taps per channel, a non-finite
 * tap, count != P N, unknown flags, window or out_dtype, a complex buffer not aligned to 8 bytes (a real output: 4), an output overlapping the input, more than
 * 2^40 values in one call (below 256 points: more than 2^31 - 1 workgroups of 64 / max(1, N / 8) frames).  GR4HIP_UNSUPPORTED: sizes of gr4hip_fft_plan kinds
 * 1, 2 and 3, more than 32 taps per channel.  n_frames == 0 is a no-op. */
#define GR4HIP_IFFT_SCALE 1
typedef struct gr4hip_ifft      gr4hip_ifft_t;
typedef struct gr4hip_pfb_synth gr4hip_pfb_synth_t;
int gr4hip_ifft_create(gr4hip_ifft_t** ifft, int out_dtype /* GR4HIP_C32 | GR4HIP_F32 */, size_t fft_size, int window, int flags);
int gr4hip_ifft_process(gr4hip_ifft_t* ifft, const void* d_spectra, size_t n_frames, void* d_out, gr4hip_stream_t stream);
int gr4hip_ifft_destroy(gr4hip_ifft_t* ifft);
int gr4hip_pfb_synth_create(gr4hip_pfb_synth_t** bank, size_t n_channels, size_t taps_per_channel, const float* h_taps /* P N values, or NULL */, int flags /* 0 | GR4HIP_IFFT_SCALE */);
int gr4hip_pfb_synth_set_taps(gr4hip_pfb_synth_t* bank, const float* h_taps, size_t count);
int gr4hip_pfb_synth_reset(gr4hip_pfb_synth_t* bank);
int gr4hip_pfb_synth_process(gr4hip_pfb_synth_t* bank, const void* d_spectra, size_t n_frames, void* d_out, gr4hip_stream_t stream);
int gr4hip_pfb_synth_destroy(gr4hip_pfb_synth_t* bank);

/* Spectrum integrator behind the |X|^2 outputs above: the sum (or mean) of A consecutive power spectra, one spectrum out per A frames in
 * (SPECTRUM_INTEGRATOR.md).  The reference has no such block: the definition is the project's, tests/spectrum_integrator_oracle.py pins it.  Frames m[f][c],
 * c < n_bins, float; output q covers frames [q A, (q + 1) A); leaf l of it covers frames q A + [l B, min((l + 1) B, A)), B = gr4hip_specint_leaf() = 32:
 *   leaf_l[c] = (((0 + m[f0][c]) + m[f0 + 1][c]) + ...)                 float32, frames ascending, one IEEE add per frame
 *   acc[c]    = ((0 + (double)leaf_0[c]) + (double)leaf_1[c]) + ...     float64, leaves ascending
 *   y_q[c]    = (float)acc[c]  (flags 0: sum)   or   (float)(acc[c] / (double)A)  (GR4HIP_SPECINT_MEAN)
 * Every sum has one fixed order, so the values do not depend on how a stream is cut into calls, bit for bit: the handle carries acc, the running leaf and the
 * frame position inside the integration.  A call that completes no integration writes nothing (d_out may then be NULL); a trailing incomplete integration is
 * never emitted.  *n_out = spectra written, known on the host without a device sync; gr4hip_specint_pending (host only) says it beforehand.  A = 1 reproduces
 * the input; non-finite values propagate as IEEE arithmetic gives them and reach exactly the integration that holds their frame.
 * gr4hip_specint_reset and gr4hip_specint_set_length (which clears the carried state) are stream-ordered (LIFECYCLE CALLS above).
 * gr4hip_fft_mag2_integrate / gr4hip_pfb_power_integrate: the values of gr4hip_fft_mag2 / gr4hip_pfb_process(d_mag2) followed by gr4hip_specint_process, bit for
 * bit, without the per-frame spectra in HBM where that measured faster (complex frames, the FFT block at 256 .. 4096 points and the bank with one tap per channel at
 * 256 .. 8192; SPECTRUM_INTEGRATOR.md); elsewhere the two calls run in pieces through a bounded scratch of 64 MiB in the integrator handle.  At 8192 points they always have the arithmetic gr4hip_fft_mag2 has below 256 frames per call, so that the values
 * do not depend on the cut.  A gr4hip_fft_set_epilogue program is applied per frame, before the sum.  si's n_bins must be what the transform's |X|^2 call
 * writes per frame.
 * GR4HIP_INVALID_ARGUMENT before any device work, outputs untouched: a NULL handle, input or n_out, d_out NULL in a call that completes an integration,
 * n_bins < 2, n_integrate == 0, unknown flags, buffers not aligned to 4 bytes (complex input: 8), input overlapping output, mismatched n_bins, more than 2^40
 * values in one call.  GR4HIP_UNSUPPORTED: n_bins > 2^20.  n_frames == 0 is a no-op (*n_out = 0). */
#define GR4HIP_SPECINT_MEAN 1
typedef struct gr4hip_specint gr4hip_specint_t;
int    gr4hip_specint_create(gr4hip_specint_t** si, size_t n_bins, size_t n_integrate, int flags);
int    gr4hip_specint_reset(gr4hip_specint_t* si);
int    gr4hip_specint_set_length(gr4hip_specint_t* si, size_t n_integrate);
int    gr4hip_specint_pending(const gr4hip_specint_t* si, size_t n_frames, size_t* n_out);
int    gr4hip_specint_process(gr4hip_specint_t* si, const float* d_frames, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream);
int    gr4hip_specint_destroy(gr4hip_specint_t* si);
size_t gr4hip_specint_leaf(void);
int    gr4hip_fft_mag2_integrate(gr4hip_fft_t* fft, gr4hip_specint_t* si, const void* d_in, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream);
int    gr4hip_pfb_power_integrate(gr4hip_pfb_t* pfb, gr4hip_specint_t* si, const void* d_in, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream);

/* Overlapped and skipped FFT frames: STFT and Welch (OVERLAPPED_FFT.md) -- the reference's `stride` setting (Block.hpp:711, 1546-1574, 1611-1616) on the FFT block,
 * stated for a stream.  N = fft_size, S = stride (0 means N).  Frame m of a stream covers the samples [m S, m S + N) and is emitted once its last sample has arrived;
 * nothing synthetic is transformed (no zeros in front of the stream, no trailing partial frame).  Each frame's outputs are exactly those of the FFT block above for
 * that frame, under the same window and flags; S < N overlaps frames, S > N skips samples.  The handle keeps `off`, the start of the next frame relative to the next
 * call's first sample (0 after create / reset, never below -(N - 1)), and carries the last N - 1 samples.  A call of n_in samples emits k = 0 frames if
 * n_in - off < N, else k = (n_in - N - off) / S + 1; afterwards off += k S - n_in.  The values do not depend on how a stream is cut into calls, nor on a call's frame
 * count: the 8192-point frame pipeline of gr4hip_fft_spectrum / _mag2 is never used.  Non-finite samples reach exactly the frames that hold them.
 * *n_frames = k, known on the host without a device sync; gr4hip_stft_pending (host only) says it beforehand: output capacity is the caller's duty.  Output layouts per
 * frame are the FFT block's.  gr4hip_stft_mag2_integrate is gr4hip_stft_mag2 followed by gr4hip_specint_process, bit for bit, in pieces through the integrator's
 * bounded scratch.  gr4hip_stft_reset (off = 0, history dropped) is stream-ordered (LIFECYCLE CALLS above).
 * Supported: every fft_size gr4hip_fft_create takes; strides 1 .. 2^20 -- GR4HIP_UNSUPPORTED from create beyond (the caller keeps its CPU path).
 * GR4HIP_INVALID_ARGUMENT before any device work: a NULL handle or n_frames, a NULL input with n_in > 0, every output NULL, an input not aligned to its element (8 bytes
 * C32, 4 bytes F32), d_spectrum not aligned to 8 bytes or a float output not to 4, an output that overlaps the input, more than 2^40 samples in or values per output
 * in one call.  n_in == 0 is a no-op with *n_frames = 0. */
typedef struct gr4hip_stft gr4hip_stft_t;
int gr4hip_stft_create(gr4hip_stft_t** stft, int in_dtype, size_t fft_size, size_t stride, int window, int flags);
int gr4hip_stft_reset(gr4hip_stft_t* stft);
int gr4hip_stft_pending(const gr4hip_stft_t* stft, size_t n_in, size_t* n_frames);
int gr4hip_stft_process(gr4hip_stft_t* stft, const void* d_in, size_t n_in, float* d_mag, float* d_phase, float* d_re, float* d_im, float* d_ranges, size_t* n_frames,
                        gr4hip_stream_t stream);
int gr4hip_stft_spectrum(gr4hip_stft_t* stft, const void* d_in, size_t n_in, float* d_spectrum, size_t* n_frames, gr4hip_stream_t stream);
int gr4hip_stft_mag2(gr4hip_stft_t* stft, const void* d_in, size_t n_in, float* d_mag2, size_t* n_frames, gr4hip_stream_t stream);
int gr4hip_stft_mag2_integrate(gr4hip_stft_t* stft, gr4hip_specint_t* si, const void* d_in, size_t n_in, float* d_out, size_t* n_out, gr4hip_stream_t stream);
int gr4hip_stft_destroy(gr4hip_stft_t* stft);

/* Cross-spectrum correlator (X-engine) behind the spectra above: the averaged cross-spectral matrix of S streams, 1 < S <= 32 (CROSS_SPECTRUM.md).  The reference
 * has no such block: the definition is the project's, tests/cross_spectrum_oracle.py pins it.  Each stream is a sequence of frames X_s[f][c], c < n_bins,
 * complex<float> -- what gr4hip_fft_spectrum / gr4hip_pfb_process(d_spectrum) write.  Output q covers frames [q A, (q + 1) A); leaf l of it covers frames
 * q A + [l B, min((l + 1) B, A)), B = gr4hip_xcorr_leaf() = 64; baselines are the lower triangle j <= i, packed p = i (i + 1) / 2 + j, P = S (S + 1) / 2:
 *   per leaf, per (i, j), per bin, float32, frames ascending, re = im = +0 at the leaf's start:
 *       re = fmaf(xr_i, xr_j, re);   re = fmaf(xi_i, xi_j, re);
 *       im = fmaf(xi_i, xr_j, im);   im = fmaf(-xr_i, xi_j, im);
 *   acc_re, acc_im: float64, leaves ascending, ((0 + (double)leaf_0) + (double)leaf_1) + ...
 *   V_q[p][c] = ((float)acc_re, (float)acc_im)  (flags 0: sum)   or   ((float)(acc_re / A), (float)(acc_im / A))  (GR4HIP_XCORR_MEAN)
 *   the imaginary part of the diagonal (i == j) is written as exactly +0.0f
 * d_out[q][p][c], interleaved complex, bin fastest.  Every sum has one order, so the values do not depend on how the stream is cut into calls or on which kernel
 * ran, bit for bit: the handle carries acc, the running leaf and the frame position.  A call that completes no integration writes nothing (d_out may then be
 * NULL); a trailing incomplete integration is never emitted.  *n_out = matrices written, known on the host without a device sync; gr4hip_xcorr_pending (host
 * only) says it beforehand.  Non-finite values propagate as IEEE arithmetic gives them and reach only the baselines that contain their stream, in the
 * integration and bin that hold them.  d_spectra is a HOST array of S device pointers, each [n_frames][n_bins] complex; the same pointer may appear twice.
 * gr4hip_xcorr_reset and gr4hip_xcorr_set_length (which clears the carried state) are stream-ordered (LIFECYCLE CALLS above).
 * gr4hip_xcorr_coherence: stateless, from n_spectra emitted matrices d_vis[n_spectra][P][n_bins] for one pair (i, j), any i, j < S (i < j: V_ji with the
 * imaginary part negated); either output may be NULL, not both:
 *   d_msc[n_spectra][n_bins]         = (float)(((double)re re + (double)im im) / ((double)V_ii (double)V_jj))     magnitude-squared coherence
 *   d_h1[n_spectra][n_bins] complex  = ((float)((double)re / (double)V_jj), (float)((double)im / (double)V_jj))   H1 = V_ij / V_jj
 * GR4HIP_INVALID_ARGUMENT before any device work, outputs untouched: a NULL handle, pointer array, entry of it or n_out, d_out NULL in a call that completes an
 * integration, n_streams < 2, n_bins < 2, n_integrate == 0, unknown flags, inputs or output not aligned to 8 bytes (d_msc: 4), the output overlapping an input,
 * i or j >= S, more than 2^40 input values per stream in one call.  GR4HIP_UNSUPPORTED: n_streams > 32, n_bins > 2^20, P n_bins > 2^24.  n_frames == 0 is a
 * no-op (*n_out = 0). */
#define GR4HIP_XCORR_MEAN 1
typedef struct gr4hip_xcorr gr4hip_xcorr_t;
int    gr4hip_xcorr_create(gr4hip_xcorr_t** xc, size_t n_streams, size_t n_bins, size_t n_integrate, int flags);
int    gr4hip_xcorr_reset(gr4hip_xcorr_t* xc);
int    gr4hip_xcorr_set_length(gr4hip_xcorr_t* xc, size_t n_integrate);
int    gr4hip_xcorr_pending(const gr4hip_xcorr_t* xc, size_t n_frames, size_t* n_out);
int    gr4hip_xcorr_process(gr4hip_xcorr_t* xc, const float* const* d_spectra, size_t n_frames, float* d_out, size_t* n_out, gr4hip_stream_t stream);
int    gr4hip_xcorr_destroy(gr4hip_xcorr_t* xc);
size_t gr4hip_xcorr_leaf(void);
int    gr4hip_xcorr_coherence(const float* d_vis, size_t n_streams, size_t n_bins, size_t n_spectra, size_t i, size_t j, float* d_msc, float* d_h1, gr4hip_stream_t stream);

/* Beamformer (B-engine) behind the spectra above: the per-bin weighted sum of S streams into B beams, 1 <= S <= 32, 1 <= B <= 32 (BEAMFORMER.md).  The reference
 * has no such block: the definition is the project's, tests/beamformer_oracle.py pins it.  Each stream is a sequence of frames X_s[f][c], c < n_bins,
 * complex<float> -- what gr4hip_fft_spectrum / gr4hip_pfb_process(d_spectrum) write.  Weights W[b][s][c], complex<float>, bin fastest, one per beam, stream and
 * bin.  Voltage beams, per beam, frame and bin, float32, streams ascending, re = im = +0 at the start:
 *       re = fmaf( wr_s, xr_s, re);   re = fmaf(-wi_s, xi_s, re);
 *       im = fmaf( wi_s, xr_s, im);   im = fmaf( wr_s, xi_s, im);
 *   Y_b[f][c] = (re, im)
 * Detected and integrated power: p_b[f][c] = fmaf(yr, yr, yi * yi) (the operation of gr4hip_fft_mag2), then the spectrum integrator's definition above, unchanged,
 * on frames of B n_bins floats laid out [b][c]: d_out[q][b][c] of gr4hip_beamform_power_integrate equals gr4hip_specint_process applied to the per-frame power,
 * bit for bit, with that block's emission rules (nothing is written until an integration completes, d_out may be NULL in a call that completes none, a trailing
 * incomplete integration is never emitted; *n_out = spectra written); the integration's state lives in si, whose n_bins must be B n_bins.  A = 1 gives the
 * per-frame power itself.  Every chain has one order, so the values do not depend on how the stream is cut into calls or on which kernel ran, bit for bit.  A
 * non-finite input value reaches every beam, one whose weight is 0 included (0 NaN = NaN), in exactly its own frame and bin, and in the integrated output
 * exactly the integration that holds its frame.  Per component |Y - exact| <= (2 S + 1) 2^-24 sum_s |W[b][s][c]| |X_s[f][c]|.
 * d_spectra is a HOST array of S device pointers, each [n_frames][n_bins] complex; the same pointer may appear twice.  d_beams is a HOST array of B device
 * pointers: d_beams[b] points at beam b's first frame, frame f lies f out_frame_stride complex values further (stride n_bins: one dense stream per beam, what
 * gr4hip_ifft_process, the synthesis bank and the X-engine take; stride B n_bins with d_beams[b] = base + b n_bins: frames [f][b][c] in one buffer).
 * gr4hip_beamform_set_weights copies d_weights ([B][S][n_bins] complex, device memory) on the stream: stream-ordered, it holds for every call enqueued after it.
 * The handle has no other state.  gr4hip_beamform_create is host code; the device buffers come with the first use.
 * GR4HIP_INVALID_ARGUMENT before any device work, outputs and *n_out untouched: a NULL handle, array, entry of one or n_out, a process call before any
 * set_weights, n_streams or n_beams == 0, n_bins < 2, buffers not aligned to 8 bytes (the float output: 4), out_frame_stride < n_bins, an output overlapping an
 * input or another beam's rows, si with n_bins != B n_bins, d_out NULL in a call that completes an integration, more than 2^40 values per stream in one call.
 * GR4HIP_UNSUPPORTED: n_streams or n_beams > 32, n_bins > 2^20, B S n_bins > 2^24.  n_frames == 0 is a no-op. */
typedef struct gr4hip_beamform gr4hip_beamform_t;
int gr4hip_beamform_create(gr4hip_beamform_t** bf, size_t n_streams, size_t n_beams, size_t n_bins);
int gr4hip_beamform_set_weights(gr4hip_beamform_t* bf, const float* d_weights /* [B][S][N] complex */, gr4hip_stream_t stream);
int gr4hip_beamform_process(gr4hip_beamform_t* bf, const float* const* d_spectra /* host array, S device pointers */, size_t n_frames,
                            float* const* d_beams /* host array, B device pointers */, size_t out_frame_stride /* complex values, >= n_bins */,
                            gr4hip_stream_t stream);
int gr4hip_beamform_power_integrate(gr4hip_beamform_t* bf, gr4hip_specint_t* si, const float* const* d_spectra, size_t n_frames,
                                    float* d_out /* [q][B][N] */, size_t* n_out, gr4hip_stream_t stream);
int gr4hip_beamform_destroy(gr4hip_beamform_t* bf);

/* Adaptive (MVDR / Capon) beamformer weights from the X-engine's matrices: per emitted matrix and bin one S x S Hermitian positive-definite solve in float64,
 * 2 <= S <= 32, for 1 <= B <= 32 steering vectors (ADAPTIVE_WEIGHTS.md).  The reference has no such block: the definition is the project's,
 * tests/adaptive_weights_oracle.py pins it.  Inputs: V[q][p][c], complex<float>, exactly what gr4hip_xcorr_process writes (packed lower triangle
 * p = i (i + 1) / 2 + j, j <= i, bin fastest); steering vectors a[b][s][c], complex<float>, in the layout of the beamformer's weights (a_s: the array's response
 * in stream s to the wanted direction; for delays tau, a = exp(+2 pi j f tau)); loading >= 0, a double held by the handle (default 0).  All arithmetic is
 * float64 (a float input is exact there); every step reads the step before it:
 *       R_ij = V_ij (j < i),  R_ji = conj(V_ij),  R_ii = Re V_ii (the imaginary part is ignored)
 *       lambda = loading * (sum_i R_ii) / S ;   R'_ii = R_ii + lambda
 *       R' = L L^H   Cholesky, columns j ascending, every inner sum with k ascending:
 *           s_j  = R'_jj - sum_{k<j} |L_jk|^2 ;   L_jj = sqrt(s_j)
 *           L_ij = (R'_ij - sum_{k<j} L_ik conj(L_jk)) / L_jj            (i > j)
 *       per beam b:   L y = a_b  (forward, k ascending) ;   d = sum_k |y_k|^2
 *                     L^H u = y  (backward) ;   w = u / d
 *       W[q][b][s][c] = conj(w_s)  rounded once to complex<float>
 *       P[q][b][c]    = (float)(1 / d)
 * The beamformer's Y = sum_s W_s X_s is then w^H X and sum_s W_s a_s = 1; P is the Capon power estimate in the units of V.  d_weights + q B S n_bins complex
 * values is directly what gr4hip_beamform_set_weights takes.  If any pivot s_j is not > 0 (NaN included) the bin of that matrix has failed: every W and P of
 * that (q, c), for all beams, is a quiet NaN and the bin is counted; neighbouring bins and matrices are untouched.  Every entry of R' feeds some pivot, so a NaN
 * anywhere in the matrix fails exactly its own bin.  A non-finite steering value goes through IEEE arithmetic, reaches only its own beam in its own bin and is
 * not counted.  The result of (q, c) is the same bits whatever n_spectra and whichever other matrices share the call.  Per component
 * |W - exact| <= 2^-24 |W_exact| + (8 + S) cond2(R') 2^-53 ||w||_2 and |P - exact| <= 2^-24 P + 2 (8 + S) cond2(R') 2^-53 P.
 * gr4hip_mvdr_create is host code; the device buffers come with the first use.  gr4hip_mvdr_set_steering copies d_steer (device memory) on the stream: it holds
 * for the calls enqueued after it.  gr4hip_mvdr_set_loading is stream-ordered like every lifecycle call (LIFECYCLE CALLS above).  gr4hip_mvdr_stats waits for
 * the handle's last call: bins_failed = failed (matrix, bin) pairs since create, bins_solved = all other pairs processed since create.
 * GR4HIP_INVALID_ARGUMENT before any device work, outputs untouched: a NULL handle, d_vis, d_weights or d_steer, a process call before any set_steering,
 * n_streams < 2, n_beams == 0, n_bins < 2, a negative or non-finite loading, complex buffers not aligned to 8 bytes (d_power: 4), an output overlapping an
 * input or the other output, more than 2^40 weights in one call.  GR4HIP_UNSUPPORTED: n_streams or n_beams > 32, n_bins > 2^20, B S n_bins > 2^24.
 * n_spectra == 0 is a no-op. */
typedef struct gr4hip_mvdr gr4hip_mvdr_t;
int gr4hip_mvdr_create(gr4hip_mvdr_t** h, size_t n_streams, size_t n_beams, size_t n_bins);
int gr4hip_mvdr_set_steering(gr4hip_mvdr_t* h, const float* d_steer /* [B][S][N] complex */, gr4hip_stream_t stream);
int gr4hip_mvdr_set_loading(gr4hip_mvdr_t* h, double loading);
int gr4hip_mvdr_process(gr4hip_mvdr_t* h, const float* d_vis /* [n_spectra][P][N] complex */, size_t n_spectra, float* d_weights /* [n_spectra][B][S][N] complex */,
                        float* d_power /* [n_spectra][B][N], may be NULL */, gr4hip_stream_t stream);
int gr4hip_mvdr_stats(gr4hip_mvdr_t* h, unsigned long long* bins_solved, unsigned long long* bins_failed);
int gr4hip_mvdr_destroy(gr4hip_mvdr_t* h);

/* ------------------------------------------------------------------------------------------------ headline chain
 * complex<float> fir_filter -> FFT block frames -> |X|^2 (BASELINE.json configs[1]).  One call consumes
 * floor(n_samples / fft_size) frames; FIR history (ntaps-1 samples) is carried across calls.
 * The runtime analogue of Merge<fir,"out",fft,"in"> (core/include/gnuradio-4.0/BlockMerging.hpp:136-320). */
typedef struct gr4hip_chain gr4hip_chain_t;
int gr4hip_chain_create(gr4hip_chain_t** chain, const float* h_taps, size_t ntaps, size_t fft_size, int window, int algo);
int gr4hip_chain_reset(gr4hip_chain_t* chain);
int gr4hip_chain_process(gr4hip_chain_t* chain, const void* d_in_c32, size_t n_samples, float* d_mag2, size_t* n_frames,
                         gr4hip_stream_t stream);
int gr4hip_chain_get_algo(const gr4hip_chain_t* chain, int* algo_in_use);
/* Dynamic-range guard of GR4HIP_CHAIN_AUTO.  The fused kernels filter in the frequency domain and carry the float32 rounding of their transforms, which is sized by the
 * frame's INPUT, while the parity bar (1e-5 of max(|Y_k|^2, rms_k |Y_k|^2)) is sized by its OUTPUT.  Every fused launch of an AUTO chain therefore judges EVERY frame (all of its
 * samples and bins) on two statistics (round 6; chain_fused.hip kGuardR4Max / kGuardPeakMax have the measurements):
 *   R4 = w2 nf mean|x|^2 / rms_k |Y_k|^2          the spread error, K sqrt(R4) with K <= 1.1e-6 on noise-like input: wide-band input the filter removes most of (a 1 %-pass-band
 *                                                filter over white noise has R4 = 6 .. 13, a 4 % one 3 .. 5, a wide-band neighbour 20 dB up ~50);
 *   T' = 2 wg^2 peak(X)^2 / rms_k |Y_k|^2         the images a float32 transform leaves of a strong line (1.2 eps of it, half a transform away): a line the filter takes down by
 *                                                10 dB or more that still dominates the output, error <= 1.4e-7 sqrt(T');
 * a frame is marked when R4 / 20 + T' / 2000 > 1 (the errors add in power: <= 6.3e-6 on the boundary; fftSize < 8192, judged per 8192-sample block: R4 / 8 + T' / 600).
 * (Until round 6 the test was output / input power < 0.08, which marked every frame of every narrow filter where nothing needed fixing, and missed the second case.)
 * What happens with the verdicts is the handle's guard mode (gr4hip_chain_set_guard_mode below; default STRICT: the frames a launch marks are evaluated again in the time domain
 * by launches enqueued behind it -- on the f16 matrix pipe where that agrees with the fused result, in float64 where it does not -- and a stream in which more than a tenth of
 * all frames end in float64 moves to the direct-form kernels, history handed over, where it stays until gr4hip_chain_reset).  Explicit GR4HIP_CHAIN_FUSED_FD never measures nor
 * switches.  gr4hip_chain_last_power_ratio waits for the last measured launch and returns its output / input power (window gain taken out; < 0: nothing measured yet --
 * informative since round 6) and whether the chain now runs in the time domain; gr4hip_chain_last_guard_fractions the fraction of that launch's frames the kernel marked
 * (< 0: nothing measured yet) and the fraction of all frames since create / reset that went on to float64. */
int gr4hip_chain_last_power_ratio(gr4hip_chain_t* chain, float* ratio, int* time_domain, gr4hip_stream_t stream);
int gr4hip_chain_last_guard_fractions(gr4hip_chain_t* chain, float* marked, float* float64, gr4hip_stream_t stream);
/* What the guard does with its measurement (per handle; GR4HIP_CHAIN_AUTO chains on the fused frequency-domain kernel only, a no-op elsewhere):
 *   GR4HIP_GUARD_STRICT (default): nothing out of tolerance is ever handed out, and nobody waits.  The fused kernel writes one verdict byte per frame; chain_td16_kernel
 *     (8192-point frames: the filter with 22-bit products on the f16 matrix pipe, window, frame transform; stored where it agrees with the fused result in every bin)
 *     and chain_redo_kernel (what that leaves: y = sum b[k] x[n - k] on the FP64 matrix pipe, window, frame transform, |.|^2 over the fused result), enqueued behind it
 *     on the same stream, evaluate exactly the marked frames again (an ordinary stream costs two near-empty launches, ~5 us each).  gr4hip_chain_process returns when
 *     the launches are queued ("user code must not block in work()", docs/USER_API_advanced_work.md).  The counts of EARLIER launches, once they have arrived, move a
 *     stream in which more than a tenth of all frames ended in float64 to the direct-form kernels for good -- read without waiting.  Several chains in one call
 *     (gr4hip_chain_process_multi) work the same way: per-channel verdict bytes and one chain_redo_kernel per channel, or -- the fold -- a frame marked when ANY
 *     channel's share of it is and chain_redo_fold_kernel, which evaluates every channel of a marked frame again and keeps the sum in registers.
 *   GR4HIP_GUARD_DEFERRED: calls stay asynchronous.  The first call after create / reset probes its first 8 blocks synchronously; later calls read the finished
 *     measurements of EARLIER launches, so the call in which a strong out-of-band signal first appears is published from the fused kernel (error floor
 *     ~2e-6 of the input rms) and the switch happens from the next call on.
 *   GR4HIP_GUARD_OFF: no measurement, never switches (what an explicit GR4HIP_CHAIN_FUSED_FD chain does). */
int gr4hip_chain_set_guard_mode(gr4hip_chain_t* chain, int mode);
/* n_chains (<= 16) chains of the same fft size fed n_samples each in ONE call -- the branches of a flowgraph with parallel SDR channels that share a device
 * (BASELINE.json configs[4] at fewer GPUs than channels).  d_in_c32 / d_mag2 are HOST arrays of device pointers.
 *   d_mag2 != NULL: chain i's spectra go to d_mag2[i];  d_sum != NULL: sum_i |FFT(fir(x_i))|^2, the combiner MathOpMultiPortImpl<float, std::plus>
 *   (blocks/math/.../Math.hpp:73-108, left fold over the inputs) -- both may be given.
 * When every chain runs the fused frequency-domain kernel at 8192 points with the rectangular window, the call is ONE persistent launch (one workgroup per
 * CU) instead of n kernels contending for every CU; with d_mag2 == NULL and identical taps on all chains the fold is kept in registers and only d_sum is
 * written (8 + 4 / n bytes of HBM traffic per sample).  Any other combination is served chain by chain followed by gr4hip_math_nary, with the same results.
 * History, guard state and measurements stay per chain (with the in-register fold the guard measures all channels together: the ratio that matters for
 * the delivered sum).  Do not mix this call with calls on the same handles from other streams. */
int gr4hip_chain_process_multi(gr4hip_chain_t* const* chains, size_t n_chains, const void* const* d_in_c32, size_t n_samples, float* const* d_mag2,
                               float* d_sum, size_t* n_frames, gr4hip_stream_t stream);
/* The fused kernels are persistent: one workgroup per CU that takes ALL of the CU's registers and LDS, so nothing else (e.g. the RCCL
 * kernels of a fan-in collective on another stream) runs beside them.  n > 0 caps the grid at n workgroups and leaves the other CUs free;
 * 0 = all CUs (default).  No effect on the unfused path. */
int gr4hip_chain_set_max_workgroups(gr4hip_chain_t* chain, unsigned n);
int gr4hip_chain_destroy(gr4hip_chain_t* chain);

/* ------------------------------------------------------------------------------------------------ e: the cross-device combiner edge
 * A flowgraph shards across the GPUs of a node only along independent branches (one SDR channel per GPU); the one exchange step is the
 * combiner MathOpMultiPortImpl<float, std::plus> (blocks/math/.../Math.hpp:73-108) whose inputs sit on different "gpu:hip:i" compute domains
 * (ComputeDomain.hpp:47-100; EdgeParameters.domain, BlockModel.hpp:64-72).  Every rank folds its own channels (gr4hip_chain_process_multi /
 * gr4hip_math_nary) and these calls add the partial sums over RCCL (xGMI): one process per GPU, one communicator rank per process, the collective
 * queued on a caller stream like every other call here.  librccl is opened at run time (an RCCL the process already carries is reused; GR4HIP_RCCL_LIBRARY
 * names one explicitly) -- GR4HIP_UNSUPPORTED with the reason in gr4hip_last_error() when there is none.
 *   gr4hip_fanin_unique_id   rank 0 draws the 128-byte id; the caller ships it to the other ranks (file, socket, MPI, a torch.distributed store ...)
 *   gr4hip_fanin_create      collective over all ranks; binds the communicator to the calling thread's current device (gr4hip_set_device)
 *   ..._reduce_scatter_sum   d_partial: n_ranks shards of shard_count floats (this rank's partial sum of every shard); d_shard: the all-rank sum of shard `rank`
 *   ..._all_to_all_sum       the same result as point-to-point sends (one xGMI link per peer, all busy at once) + a left fold in RANK order: the reduction
 *                            order does not depend on RCCL's ring; d_scratch: n_ranks * shard_count floats
 *   ..._all_reduce_sum       every rank gets the whole sum (a sink that lives on every rank, or on one)
 * In-place operation (d_shard inside d_partial etc.) follows RCCL's rules. */
typedef struct gr4hip_fanin gr4hip_fanin_t;
#define GR4HIP_FANIN_ID_BYTES 128
int gr4hip_fanin_unique_id(void* id128);
int gr4hip_fanin_create(gr4hip_fanin_t** fanin, const void* id128, int rank, int n_ranks);
int gr4hip_fanin_rank(const gr4hip_fanin_t* fanin, int* rank, int* n_ranks);
int gr4hip_fanin_reduce_scatter_sum_f32(gr4hip_fanin_t* fanin, const float* d_partial, float* d_shard, size_t shard_count, gr4hip_stream_t stream);
int gr4hip_fanin_all_to_all_sum_f32(gr4hip_fanin_t* fanin, const float* d_partial, float* d_scratch, float* d_shard, size_t shard_count, gr4hip_stream_t stream);
int gr4hip_fanin_all_reduce_sum_f32(gr4hip_fanin_t* fanin, const float* d_partial, float* d_sum, size_t count, gr4hip_stream_t stream);
int gr4hip_fanin_destroy(gr4hip_fanin_t* fanin);

/* ------------------------------------------------------------------------------------------------ a11/a12/a13
 * MathOpImpl<T,op>::processOne (blocks/math/.../Math.hpp:38-56): out = in (op) value, C++ semantics for T
 * (integer promotion then narrowing, wrap-around).  h_value points to one host element of `dtype`.
 * Spans need only their element's natural alignment (a ring span starts at any element); 16-byte aligned spans are fastest. */
int gr4hip_math_const(int op, int dtype, const void* d_in, void* d_out, size_t n, const void* h_value, gr4hip_stream_t stream);
/* MathOpMultiPortImpl<T,op>::processBulk (Math.hpp:100-107): left fold ((in0 op in1) op in2) ... over 1..32 inputs.
 * h_d_ins is a HOST array of n_inputs device pointers. */
int gr4hip_math_nary(int op, int dtype, const void* const* h_d_ins, size_t n_inputs, void* d_out, size_t n, gr4hip_stream_t stream);

/* ------------------------------------------------------------------------------------------------ fused runs of per-sample blocks
 * The reference fuses adjacent blocks at compile time: Merge<A, "out", B, "in"> (core/include/gnuradio-4.0/BlockMerging.hpp:126-240) is ONE processOne() that
 * carries the value through both parts in registers -- its published table (docs/USER_API_Connecting_Blocks.md:207-222) measures mult -> div -> add and that
 * chain ten times over.  gr4hip_ewise is the same thing for chains known at run time: a PROGRAM of per-sample ops of one sample type --
 *   gr4hip_ewise_append_const    MathOpImpl<T, op>::processOne (Math.hpp:38-56): value (op) constant, the semantics of gr4hip_math_const (integers promote, wrap and
 *                                narrow like C++: bit-exact; float ops are single IEEE operations in program order, never contracted into fused multiply-adds)
 *   gr4hip_ewise_append_rotator  Rotator<complex<float>>::processOne (Rotator.hpp:51-61) with the closed-form phase of GR4HIP_ROTATOR_CLOSED_FORM: sample k of the
 *                                stream (counted from create / reset) is multiplied by exp(j (initial_phase + (k + 1) phase_increment)); C32 programs only
 * -- that gr4hip_ewise_process runs as ONE launch with the values in registers: 2 sizeof(T) bytes of HBM traffic per sample whatever the number of ops.
 * The same program can ride in the launch of a neighbouring filter as its load hook (prologue) or store hook (epilogue): gr4hip_fir_set_prologue / _epilogue below.
 * A program holds no device state besides its op list; the stream position (what a rotator op's phase is a function of) is advanced by gr4hip_ewise_process. */
int gr4hip_ewise_create(gr4hip_ewise_t** prog, int dtype);
int gr4hip_ewise_append_const(gr4hip_ewise_t* prog, int op, const void* h_value); /* h_value: one host element of the program's dtype */
int gr4hip_ewise_append_rotator(gr4hip_ewise_t* prog, float phase_increment, float initial_phase);
int gr4hip_ewise_length(const gr4hip_ewise_t* prog, size_t* n_ops);
int gr4hip_ewise_reset(gr4hip_ewise_t* prog); /* stream position back to 0: rotator ops restart from their initial phase */
int gr4hip_ewise_position(const gr4hip_ewise_t* prog, uint64_t* samples);
int gr4hip_ewise_process(gr4hip_ewise_t* prog, const void* d_in, void* d_out, size_t n, gr4hip_stream_t stream); /* in place (d_in == d_out) is allowed */
/* gr::filter::Decimator<T> (time_domain_filter.hpp:234-244) with the program's blocks BEHIND it in one launch: d_out[m] = program(d_in[m * decim]), m < ceil(n_in / decim);
 * only the kept samples are read.  The stream position (rotator phase) counts OUTPUT samples.  Memoryless blocks in front of a Decimator commute with it, so a planner
 * that finds const blocks on either side of one hands them all to this call. */
int gr4hip_ewise_decimate(gr4hip_ewise_t* prog, const void* d_in, size_t n_in, size_t decim, void* d_out, size_t* n_out, gr4hip_stream_t stream);
int gr4hip_ewise_destroy(gr4hip_ewise_t* prog);
/* Neighbours of a FIR filter in ITS launch.  prologue: applied to every input sample before the filter sees it (the history the filter carries is the history of
 * the prologue's OUTPUT, zero before the first sample, exactly as if the blocks ran one after the other); epilogue: applied to every output sample before it is
 * stored.  The program is copied (later changes to `prog` do not reach the filter); NULL or an empty program removes the hook.  dtype of the program == dtype of
 * the filter.  How it is executed:
 *   - a program that is nothing but real gains (MultiplyConst / DivideConst; complex constants with a zero imaginary part) is folded into the taps -- a FIR filter
 *     is linear, fir(g x) == (g b) * x -- and costs nothing in any kernel (the rounding differs from the two-block form in the last bits: one float product per
 *     tap instead of one per sample, same float32 level, same 1e-5 parity bar);
 *   - anything else (AddConst / SubtractConst, complex gains, a rotator) is a load / store hook of the register-window kernel (any tap count, any decimation, float
 *     or complex) or of the band-form matrix-pipe decimators (float: decimation 2 .. 12, complex: 3 .. 16, windows they hold, spans of >= 2^14 outputs): one launch, no
 *     intermediate stream in HBM.  Exception, by measurement: where a plain filter of the same shape takes a matrix-pipe or
 *     frequency-domain kernel AND the register-window kernel is far behind it (more than 96 taps -- 64 for complex -- on a span of >= 2^16 samples, float decimators with
 *     more than 12 taps per output on long spans), that kernel is worth more than the saved pass
 *     (add -> 256-tap FIR: 165 Gsamples/s hooked, 277 as an element-wise launch + the bf16 kernel), and the program runs as ONE element-wise launch in front of
 *     (behind) the filter's own inside this call: same results, same carried history.
 * The history the filter carries is always what the prologue in force made of the samples -- also when the prologue is replaced in mid-stream: the samples already in
 * the filter's memory keep the OLD program's values, exactly as when the blocks run one after the other.  GR4HIP_UNSUPPORTED: the program's dtype does not match. */
int gr4hip_fir_set_prologue(gr4hip_fir_t* fir, const gr4hip_ewise_t* prog);
int gr4hip_fir_set_epilogue(gr4hip_fir_t* fir, const gr4hip_ewise_t* prog);

/* Rotator<complex<float>>::processOne (blocks/math/.../Rotator.hpp:51-61): phase += inc (before the first sample),
 * single +-2pi wrap, y = x * (cos, sin); the accumulated phase is carried across calls.
 * Two evaluations of the phase (gr4hip_rotator_set_algo; both keep the same carried state, so they may be switched between calls):
 *   GR4HIP_ROTATOR_CLOSED_FORM (default): sample i of a call sees carried + (i + 1) inc, computed in float64 and reduced exactly -- the float64
 *     oracle's phase (<= 1e-5 against it however long the stream and however many calls it is cut into: the carried phase is kept in float64 by the
 *     handle, gr4hip_rotator_phase reports it rounded to float), one HBM-bound pass.  The default is MORE ACCURATE THAN, not identical to, the
 *     reference block: it does NOT reproduce the drift of the reference's float accumulator (~1e-7 rad per step), so against the reference's own output
 *     it is beyond 1e-5 after ~10^3..10^5 samples.  A caller who needs the CPU block's output bit for bit selects the recurrence (below; the host
 *     engine: gr::hip::options().rotator_reference_recurrence).
 *   GR4HIP_ROTATOR_RECURRENCE: the reference's float recurrence itself, bit-identical phase sequence and carried phase (a sequential walk: ~10^2..10^4
 *     times slower, for callers that need the reference's exact output). */
typedef struct gr4hip_rotator gr4hip_rotator_t;
typedef enum { GR4HIP_ROTATOR_CLOSED_FORM = 0, GR4HIP_ROTATOR_RECURRENCE = 1 } gr4hip_rotator_algo;
int gr4hip_rotator_create(gr4hip_rotator_t** rot, float phase_increment, float initial_phase);
int gr4hip_rotator_set_algo(gr4hip_rotator_t* rot, int algo);
int gr4hip_rotator_reset(gr4hip_rotator_t* rot, float initial_phase); /* settingsChanged: _accumulated_phase = initial_phase */
int gr4hip_rotator_process(gr4hip_rotator_t* rot, const void* d_in_c32, void* d_out_c32, size_t n, gr4hip_stream_t stream);
int gr4hip_rotator_phase(gr4hip_rotator_t* rot, float* phase, gr4hip_stream_t stream); /* synchronises the stream */
int gr4hip_rotator_destroy(gr4hip_rotator_t* rot);

/* ------------------------------------------------------------------------------------------------ float64 instantiations
 * The second registered type of the hot-path blocks: fir_filter<double> / iir_filter<double, form> (time_domain_filter.hpp:20, 57-60), FFT<double>
 * (fourier/fft.hpp:29: real double frames -> DataSet<double>) and Rotator<complex<double>> (Rotator.hpp:15).  Same semantics as the float32 entry points
 * above (history / state carried between calls, decimation = y[m D], all IIR forms evaluated as DF-II, an IIR section's a[0] taken as 1 whatever it holds -- not
 * divided by, as in gr4hip_iir_create -- and gr4hip_iir64_process refusing overlapping input and output ranges like gr4hip_iir_process, FFT outputs of a real-input block: magnitude and
 * phase of bins 0 .. N/2-1, Re / Im of bins N/2 .. N-1), plain FP64 kernels.  Envelope: FIR <= 2048 taps, decim <= 32; IIR <= 8 state values (4 biquads,
 * or one section of order <= 8); FFT powers of two 2 .. 8192; anything else returns GR4HIP_UNSUPPORTED from create (the caller keeps its CPU path). */
typedef struct gr4hip_fir64 gr4hip_fir64_t;
int gr4hip_fir64_create(gr4hip_fir64_t** fir, const double* h_taps, size_t ntaps, size_t decim);
int gr4hip_fir64_set_taps(gr4hip_fir64_t* fir, const double* h_taps, size_t ntaps); /* history kept unless it has to grow */
int gr4hip_fir64_reset(gr4hip_fir64_t* fir);
int gr4hip_fir64_process(gr4hip_fir64_t* fir, const double* d_in, size_t n_in, double* d_out, size_t* n_out, gr4hip_stream_t stream);
int gr4hip_fir64_destroy(gr4hip_fir64_t* fir);
typedef struct gr4hip_iir64 gr4hip_iir64_t;
int gr4hip_iir64_create(gr4hip_iir64_t** iir, int form, size_t nsections, const double* h_b, size_t nb, const double* h_a, size_t na);
int gr4hip_iir64_reset(gr4hip_iir64_t* iir);
int gr4hip_iir64_process(gr4hip_iir64_t* iir, const double* d_in, size_t n, double* d_out, gr4hip_stream_t stream);
int gr4hip_iir64_destroy(gr4hip_iir64_t* iir);
typedef struct gr4hip_fft64 gr4hip_fft64_t;
int gr4hip_fft64_create(gr4hip_fft64_t** fft, size_t fft_size, int window, int flags);
int gr4hip_fft64_process(gr4hip_fft64_t* fft, const double* d_in, size_t n_frames, double* d_mag, double* d_phase, double* d_re, double* d_im, gr4hip_stream_t stream);
int gr4hip_fft64_destroy(gr4hip_fft64_t* fft);
typedef struct gr4hip_rotator64 gr4hip_rotator64_t;
int gr4hip_rotator64_create(gr4hip_rotator64_t** rot, double phase_increment, double initial_phase);
int gr4hip_rotator64_reset(gr4hip_rotator64_t* rot, double initial_phase);
int gr4hip_rotator64_process(gr4hip_rotator64_t* rot, const void* d_in_c64, void* d_out_c64, size_t n, gr4hip_stream_t stream);
int gr4hip_rotator64_phase(gr4hip_rotator64_t* rot, double* phase);
int gr4hip_rotator64_destroy(gr4hip_rotator64_t* rot);

/* ------------------------------------------------------------------------------------------------ batched FIR (configs[3])
 * nchannels independent fir_filter<float> instances, per-channel taps h_taps[c][k], channel-major samples
 * d_in[c * in_stride + n]; evaluated as a block-Toeplitz contraction on the matrix pipe: more than 32 taps on spans of >= 32768 samples per channel with two-term
 * f16 splits under a per-segment block exponent (csrc/fir_f16.hip: three products per tap, every segment judged, see gr4hip_fir_set_algo above), otherwise with
 * float32 products on the f32 MFMA units.  d_in: in_stride >= n; d_out: 16-byte aligned, out_stride >= n and a multiple of 4; nothing outside the rows' [0, n) is
 * read or written.  The guard per path: the f16 kernel judges each channel's segments itself, the three-term bf16 kernel that replaces it under
 * GR4HIP_FIR_NO_F16X2 (or when a tap is not finite) is judged behind its launch, and the marked segments of either are evaluated again on the FP64 matrix pipe
 * (csrc/fir_exact.hip); the f32 MFMA kernel's sums stay below the reference's own float32 error (measured 0.5 x under a rejected tone) and are not judged. */
typedef struct gr4hip_fir_batched gr4hip_fir_batched_t;
int gr4hip_fir_batched_create(gr4hip_fir_batched_t** fb, size_t nchannels, const float* h_taps, size_t ntaps);
int gr4hip_fir_batched_reset(gr4hip_fir_batched_t* fb);
int gr4hip_fir_batched_process(gr4hip_fir_batched_t* fb, const float* d_in, size_t in_stride, size_t n, float* d_out, size_t out_stride,
                               gr4hip_stream_t stream);
int gr4hip_fir_batched_destroy(gr4hip_fir_batched_t* fb);

/* ------------------------------------------------------------------------------------------------ a15 (bench input)
 * device-side synthetic stream of SURVEY.md 8(d): unit-power Gaussian noise + tone.  The stream is cut into groups of 8 samples; group g has its own
 * generator Xoshiro256pp(seed ^ 0xd1b54a32d192ed03 (g + 1)) (algorithm/.../rng/Xoshiro256pp.hpp:22-96, constructor :33-39) and fills its 8 samples with
 * GaussianNoise<float>::fill / fillComplex (GaussianNoise.hpp:59-111: Marsaglia polar, amplitude / sqrt2 per component for complex), so every group
 * is the reference's own recipe and the groups are independent (any lane can generate any group).  It is NOT the single sequential reference stream
 * (tests that need that one upload it).  gr4hip_synth_draws returns the raw 64-bit draws of group g's generator: with seed = 0xd1b54a32d192ed03, g = 0
 * that generator is Xoshiro256pp(0), whose first draws are the reference's known answer (algorithm/test/qa_Xoshiro256pp.cpp:55-69). */
int gr4hip_synth_draws(uint64_t* d_out_u64, size_t n_draws, uint64_t seed, uint64_t group, gr4hip_stream_t stream);
int gr4hip_synth_c32(void* d_out_c32, size_t n, uint64_t seed, double tone_frel, float tone_amp, float noise_amp, gr4hip_stream_t stream);
int gr4hip_synth_f32(float* d_out, size_t n, uint64_t seed, double tone_frel, float tone_amp, float noise_amp, gr4hip_stream_t stream);

/* ------------------------------------------------------------------------------------------------ frequency estimators (blocks/filter/.../FrequencyEstimator.hpp)
 * FrequencyEstimatorTimeDomain<float> (:30-176, Krajewski et al. 2022) and FrequencyEstimatorFrequencyDomain<float> (:186-351, Gasior & Gonzalez 2004), float only
 * (the reference's double registrations have no entry point here).  Design notes: FREQ_EST.md.  One path per method,
 * parameterised by the chunk C >= 1: output m is the estimate after input sample (m + 1) C - 1 over the last W samples seen.  processOne is C = 1, the
 * decimating forms are C = 10 (time domain, Resampling<10U>, :179) and C = N (frequency domain, initialiseFFT sets input_chunk_size = N, :231-242).
 *   W (gr4hip_freqest_geometry): time domain N_est = n_periods * Size_t(fs / min(f_min, f_expected)) (fs / f_expected when f_min == 0), in float, truncated (:72);
 *   frequency domain N = bit_ceil(max(min_fft_size, size_t(fs / min(f_min, f_expected)))) (:232); search range [i_min, i_max) with i_min = floor(f_min / fs N),
 *   i_max = ceil(f_max / fs N) in float, both clamped to [1, N/2 - 1] (:300-306); an empty range (i_min >= i_max) gives k = i_max.
 * Every output is a fresh estimate or, on any fallback of the reference (settling: fewer than W samples since reset; B <= eps, z outside (-1, 1); peak at the edge,
 * non-positive or non-finite magnitudes, |denominator| < eps, |delta| >= 1), the previous output: a forward fill on the device across the launch and across calls.
 *   time domain: the one Bessel biquad at f_max (iir::designFilter<T, 0UZ>, :77 == gr4hip_iir_design(GR4HIP_BESSEL, order 2)) on the library's IIR path into a
 *     scratch buffer of the handle; the window sums B = sum b^2, C = sum 2ab (= (y[i-1] + y[i+1])^2 / 2 where |4 y[i]| >= eps) direct per output or sliding
 *     from a direct sum at the head of each run of outputs, in float64; z and acos in float64.  A NaN / Inf input poisons the biquad state: every later
 *     output is NaN until reset / set_params, as in the reference.
 *   frequency domain: only bins i_min - 1 .. i_max are evaluated.  The symmetric Hann window (window.hpp:92-97) is 1/2 - e^{j a i}/4 - e^{-j a i}/4, a = 2 pi / (N - 1),
 *     so each bin is three sliding sums S_theta(n) = sum_i x[n - i] e^{-j theta i} (theta = 2 pi k / N and +-a), updated in O(1) in float64 and anchored by a direct sum at
 *     the head of every tile of outputs (C < N); with C >= N every output is its own direct sum.  Non-finite samples enter the sums as 0 and are counted: a window
 *     that holds one gives the previous output (the reference's FFT turns it into non-finite magnitudes).  A search range of more than 2046 bins
 *     (i_max - i_min + 2 > 2048) returns GR4HIP_UNSUPPORTED.
 *   GR4HIP_UNSUPPORTED also for W > 2^20, N < 4 and f_max <= 0 (the reference's doc calls f_max < 0 "disable" but its code designs the low-pass anyway);
 *   GR4HIP_INVALID_ARGUMENT for what settingsChanged rejects (f_min < 0, f_max >= fs/2, f_expected < 0, f_expected >= fs/2; :62-69, :222-229), for f_expected == 0
 *   (the reference divides by it), non-finite settings, fs <= 0, n_periods == 0 (time domain), chunk == 0 and n_in % chunk != 0.  All of it is checked on the
 *   host before any device work.
 * The last estimate: create and reset leave f_expected (reset(), :82-85, :244-247: a created handle is a block that has been reset); set_params keeps it
 * (settingsChanged only re-initialises: histories emptied).  Both are host-side notes applied by the next process call on its stream. */
typedef struct gr4hip_freqest gr4hip_freqest_t;
typedef enum { GR4HIP_FREQEST_TIME_DOMAIN = 0, GR4HIP_FREQEST_FREQUENCY_DOMAIN = 1 } gr4hip_freqest_method;
typedef struct {
    float  sample_rate, f_min, f_expected, f_max, epsilon;
    size_t n_periods;    /* time domain */
    size_t min_fft_size; /* frequency domain */
    size_t chunk;        /* C: inputs per output */
} gr4hip_freqest_params;
int gr4hip_freqest_params_default(int method, gr4hip_freqest_params* p); /* the blocks' defaults (fs 1000, 40 / 50 / 60 Hz, eps 1e-8, n_periods 4, min_fft_size 256); chunk 1 */
/* host only: W (N_est or N) and, for the frequency domain, the clamped search range (0, 0 for the time domain); same validation as create */
int gr4hip_freqest_geometry(int method, const gr4hip_freqest_params* p, size_t* window, size_t* i_min, size_t* i_max);
int gr4hip_freqest_create(gr4hip_freqest_t** fe, int method, const gr4hip_freqest_params* p);
int gr4hip_freqest_set_params(gr4hip_freqest_t* fe, const gr4hip_freqest_params* p); /* settingsChanged: histories emptied, the last estimate kept */
int gr4hip_freqest_reset(gr4hip_freqest_t* fe);                                      /* reset(): histories emptied, the last estimate = f_expected */
/* n_in a multiple of chunk; writes n_in / chunk outputs (*n_out, may be NULL) */
int gr4hip_freqest_process(gr4hip_freqest_t* fe, const float* d_in, size_t n_in, float* d_out, size_t* n_out, gr4hip_stream_t stream);
int gr4hip_freqest_destroy(gr4hip_freqest_t* fe);

/* ------------------------------------------------------------------------------------------------ IQ demodulator (FrequencyEstimator.hpp:356-653)
 * IQDemodulator<T> (T = float: GR4HIP_F32, double: GR4HIP_F64), a lock-in amplifier: inputs ref (the DDS reference) and resp (the response), one output per
 * chunk of C inputs on each of amplitude (A_resp / A_ref), phase and frequency.  Design notes: IQ_DEMOD.md.  Restates IQDemodulator<T> exactly:
 *   coefficients in T as initialiseFilters (:468-506) computes them: alpha_hp = exp(T(-2) pi_v<T> T(f_high_pass) / T(sample_rate)), alpha_lp = 1 - exp(...)
 *   likewise, the derivative taps {1,0,-1}, {0.2,0.1,0,-0.1,-0.2}, {3,2,1,0,-1,-2,-3}/28 in T, delays 1 / 2 / 3; then widened: every state is float64.
 *   Per sample n since the last re-initialisation:  h[n] = alpha_hp (h[n-1] + v[n] - v[n-1]) per input (v[-1] = h[-1] = 0);  rQ = sum_k tap[k] h_ref[n-k] once
 *   n + 1 >= K, else 0;  rI = h_ref[n-d], xI = h_resp[n-d] once n >= d, else 0 (the HistoryBuffer size tests of :548-555, across calls);  the products
 *   xI rI, xI rQ, rI^2, rQ^2, xI^2 into five low-passes s += alpha_lp (p - s).  At the last sample of every chunk, step 5 (:571-640) in float64: amplitude,
 *   G(omega) per method, three rounds of asin iterations with an Aitken step, atan2(Q, I sqrt(Pd / Pr)), invert_phase, degrees; rounded to T.  Outputs the
 *   reference gives as 0 (Pr <= eps, Px <= eps, ...) are exactly 0.  A non-finite input poisons the states until re-initialisation, as in the reference:
 *   from there on every output is 0.  Where the reference's float arithmetic is ill-conditioned (DC-only input, whose high-passed value decays below rounding;
 *   |ratio / G| near 1 in the asin) the device gives the float64 result, not the float32 noise.
 * GR4HIP_INVALID_ARGUMENT, checked on the host before any device work: what settingsChanged rejects (!(0 < f_hp < f_lp < fs / 2), in float, :461), non-finite
 * settings, sample_rate <= 0, an unknown derivative_method or phase_unit, chunk == 0, n_in % chunk != 0, a dtype other than F32 / F64.
 * reset() and set_params(reinitialise = 1) re-initialise the filters (states and history zeroed); set_params(reinitialise = 0) keeps them and takes phase_unit,
 * invert_phase, epsilon and chunk -- the filter settings must then be unchanged.  reinitialise mirrors settingsChanged (:454-466): the caller passes whether the
 * update named sample_rate, f_high_pass, f_low_pass or derivative_method.  Both are host-side notes applied by the next process call on its stream. */
typedef struct gr4hip_iqdemod gr4hip_iqdemod_t;
typedef struct {
    float  sample_rate, f_high_pass, f_low_pass;
    int    phase_unit;        /* 0 radians, 1 degrees */
    int    invert_phase;      /* bool */
    int    derivative_method; /* 0 symmetric difference, 1 Savitzky-Golay 5, 2 Savitzky-Golay 7 */
    double epsilon;           /* rounded to T */
    size_t chunk;             /* C: inputs per output (input_chunk_size) */
} gr4hip_iqdemod_params;
int gr4hip_iqdemod_params_default(gr4hip_iqdemod_params* p); /* the block's defaults (62.5 MHz, 100 Hz, 10 kHz, radians, eps 1e-12), chunk 1024 */
int gr4hip_iqdemod_check(int dtype, const gr4hip_iqdemod_params* p); /* host only: the validation of create */
int gr4hip_iqdemod_create(gr4hip_iqdemod_t** h, int dtype, const gr4hip_iqdemod_params* p);
int gr4hip_iqdemod_set_params(gr4hip_iqdemod_t* h, const gr4hip_iqdemod_params* p, int reinitialise);
int gr4hip_iqdemod_reset(gr4hip_iqdemod_t* h);
/* d_ref / d_resp: n_in samples of T, n_in a multiple of chunk; writes n_in / chunk samples of T to each output (*n_out, may be NULL) */
int gr4hip_iqdemod_process(gr4hip_iqdemod_t* h, const void* d_ref, const void* d_resp, size_t n_in, void* d_amp, void* d_phase, void* d_freq, size_t* n_out,
                           gr4hip_stream_t stream);
int gr4hip_iqdemod_destroy(gr4hip_iqdemod_t* h);

/* ------------------------------------------------------------------------------------------------ Power metrics (blocks/electrical/.../PowerEstimators.hpp:21-131)
 * gr::electrical::PowerMetrics<float, nPhases>: per phase a voltage input u and a current input i; one output per chunk of `decimate` inputs on each of P (active
 * power), Q (reactive), S (apparent), U_rms and I_rms.  Design notes: POWER_METRICS.md.  Restates processBulk (:97-130) exactly:
 *   uh = HP(u), ih = HP(i): one biquad each, iir::designFilter<float>(HIGHPASS, {order 2, fHigh = high_pass, fs = sample_rate}, BUTTERWORTH) (:69-71); the
 *   identity when high_pass <= 0 (:73).  ema_p = LP(uh ih), ema_u2 = LP(uh uh), ema_i2 = LP(ih ih): one biquad each, designFilter<float>(LOWPASS, {order 2,
 *   fLow = min(0.5 sample_rate / decimate, low_pass)}) with the cutoff formed in double (:83-87).  Every filter runs in direct form II as Filter<float>::processOne
 *   does (FilterTool.hpp:130-136).  At every sample whose index since the last re-initialisation is a multiple of decimate (:111, the FIRST sample of a chunk),
 *   after that sample went through all filters: U_rms = sqrt(ema_u2), I_rms = sqrt(ema_i2), S = U_rms I_rms, Q = sqrt(max(S^2 - P^2, 0)), P = ema_p (:113-123).
 *   A negative moving average (a second-order low-pass rings below zero behind a burst) gives NaN for that RMS and with it for S and Q, as math::sqrt and
 *   std::max(NaN, 0) do.  The coefficients are gr4hip_iir_design's float ones, widened; every state, product and the final step are float64 and the outputs are
 *   rounded to float once: where the reference's float direct-form-II states (about 1e6 times the signal at 2 Hz / 10 kHz) make its outputs noisy at the 1e-3
 *   level, the device gives the float64 result.  A non-finite input poisons the filters it reaches until re-initialisation, as in the reference: from two samples
 *   behind it every output of that phase that depends on the input is NaN (a bad u: all but I_rms; a bad i: all but U_rms); other phases are untouched.  All-zero
 *   input gives exactly 0.
 * d_u / d_i: n_phases rows of n_in floats, in_stride elements apart; every output: n_phases rows of n_in / decimate floats, out_stride apart; any output pointer
 * may be NULL.  n_in == 0 is OK and writes nothing.
 * GR4HIP_INVALID_ARGUMENT, checked on the host before any device work: a non-finite or non-positive sample_rate or low_pass, a non-finite high_pass or one
 * >= sample_rate / 2, decimate == 0, n_phases outside 1 ... 16, n_in % decimate != 0, a stride smaller than its row, an input overlapping an output, a design
 * that is not one biquad or has a pole outside the unit circle.  A pole ON the circle is taken: the float design of a cutoff below about 2e-4 sample_rate puts
 * one at z = 1 exactly (1 + a1 + a2 rounds to 0; the low-pass then has b0 = 0 and gives 0, the high-pass becomes a first-order one), the reference runs such
 * filters, and the exact carries need no decay.
 * set_params always re-initialises (settingsChanged rebuilds every filter, :95; n_phases is fixed at create); reset zeroes the states.  Both are host-side notes
 * applied by the next process call on its stream.  process queues its kernels and returns without waiting for them, with one exception: the handle keeps
 * 160 bytes of carry scratch per phase and segment of the longest call so far, and a call longer than every earlier one frees and allocates it again, which
 * waits for the whole device (hipFree).  A caller that must not stall makes its longest call first. */
#define GR4HIP_POWERMETRICS_SEGMENT 4096 /* samples per workgroup segment: where the carries change hands (tests place their boundaries by it) */
typedef struct gr4hip_powermetrics gr4hip_powermetrics_t;
typedef struct {
    float  sample_rate, high_pass, low_pass; /* (:46-48) */
    size_t decimate;                         /* (:49) inputs per output, input_chunk_size */
    size_t n_phases;                         /* nPhases */
} gr4hip_powermetrics_params;
int    gr4hip_powermetrics_params_default(gr4hip_powermetrics_params* p); /* 10 kHz, 2 Hz, 90 Hz, decimate 100, one phase */
int    gr4hip_powermetrics_check(const gr4hip_powermetrics_params* p);    /* host only: the validation of create */
size_t gr4hip_powermetrics_segment(void);                                 /* GR4HIP_POWERMETRICS_SEGMENT of the built library */
int    gr4hip_powermetrics_create(gr4hip_powermetrics_t** h, const gr4hip_powermetrics_params* p);
int    gr4hip_powermetrics_set_params(gr4hip_powermetrics_t* h, const gr4hip_powermetrics_params* p);
int    gr4hip_powermetrics_reset(gr4hip_powermetrics_t* h);
int    gr4hip_powermetrics_process(gr4hip_powermetrics_t* h, const float* d_u, const float* d_i, size_t in_stride, size_t n_in, float* d_P, float* d_Q, float* d_S,
                                   float* d_Urms, float* d_Irms, size_t out_stride, size_t* n_out, gr4hip_stream_t stream);
int    gr4hip_powermetrics_destroy(gr4hip_powermetrics_t* h);

/* ------------------------------------------------------------------------------------------------ Power factor and system unbalance (PowerEstimators.hpp:144-257)
 * The two blocks PowerMetrics feeds, stateless and per sample like gr4hip_math_nary; the rows have the stride layout of gr4hip_powermetrics_process, so its
 * outputs chain straight in without a copy.  dtype is GR4HIP_F32 or GR4HIP_F64 (the UncertainValue instantiations are left out, as for PowerMetrics).  The
 * arithmetic is gr4/electrical_ops.hpp, shared with the host mirror blocks; design notes: POWER_QUALITY.md.
 *
 * gr4hip_powerfactor_process replaces gr::electrical::PowerFactor<T, nPhases>::processBulk (:161-181): per phase and sample c = (S != 0) ? P / S : 0, clamped to
 * [-1, 1] as std::clamp does (a NaN stays NaN, -0.0 stays -0.0); power_factor = c, phase = acos(c) (float samples: acos in float64 on the float argument, rounded
 * once).  d_P / d_S: n_phases (1 ... 16) rows of n elements, in_stride elements apart; d_power_factor / d_phase: the same shape, out_stride apart.
 *
 * gr4hip_unbalance_process replaces gr::electrical::SystemUnbalance<T, nPhases>::processBulk (:217-256): per sample over the n_phases (2 ... 16) rows of d_Urms,
 * d_Irms and d_P, in_stride apart: P_total = ((0 + P_0) + P_1) + ...; for U and I avg = (((0 + x_0) + x_1) + ...) / n_phases; the voltage's largest deviation is
 * the left fold m = (m < |x_i - avg|) ? |x_i - avg| : m from 0 (std::transform_reduce with std::max, :234-237), the current's is |best - avg| of the
 * std::max_element under |a - avg| < |b - avg| (:243-245); unbalance = (avg > 0) ? (dmax / avg) * 100 : 0.  The two forms differ on one input: every phase +inf
 * gives 0 for the voltage and NaN for the current.  Each output is ONE row of n elements.
 *
 * Both: any output pointer may be NULL (an unconnected port; what only it needs is neither read nor computed).  n == 0 is OK and writes nothing.  Pointers need
 * their element's alignment only; rows that share a misalignment from 16 bytes move 16 bytes per lane, a row that disagrees is moved element by element.
 * GR4HIP_INVALID_ARGUMENT, checked on the host before any device work: a dtype other than F32 / F64, a phase count outside the range, a NULL input, a pointer not
 * aligned to its element, a stride smaller than n, an input overlapping an output.  The call queues one kernel on `stream` and returns. */
int    gr4hip_powerfactor_process(int dtype, size_t n_phases, const void* d_P, const void* d_S, size_t in_stride, void* d_power_factor, void* d_phase, size_t out_stride,
                                  size_t n, gr4hip_stream_t stream);
int    gr4hip_unbalance_process(int dtype, size_t n_phases, const void* d_Urms, const void* d_Irms, const void* d_P, size_t in_stride, void* d_P_total,
                                void* d_U_unbalance, void* d_I_unbalance, size_t n, gr4hip_stream_t stream);
size_t gr4hip_electrical_tile(void); /* items per workgroup of both kernels: tests place their edges by it */

/* ------------------------------------------------------------------------------------------------ Schmitt trigger (algorithm/.../SchmittTrigger.hpp:39-357)
 * gr::trigger::SchmittTrigger<T, Method, 32>, the detector of gr::blocks::basic::SchmittTrigger (blocks/basic/.../Trigger.hpp:45: N_HISTORY = 32), for T in
 * {int16, int32, float, double}: processOne (:103-222) applied to every sample of the stream exactly once, in order, whatever the chunking into calls; the
 * output is the ordered list of the samples at which it returned RISING or FALLING, with lastEdgeIdx and value(lastEdgeOffset).  Design notes: SCHMITT_TRIGGER.md.
 *   thresholds: upper = offset + threshold, lower = offset - threshold in the value type (:67).
 *   a created or reset handle is a detector after reset() (:90-101): _lastState false, nothing accumulated, a history of 32 zeros (the first yPrev is 0).
 *   NO_INTERPOLATION (:107-121): RISING where !_lastState and x >= upper, FALLING where _lastState and x <= lower; edge_idx 0, edge_offset 0, n_fit 0.
 *   BASIC_LINEAR_INTERPOLATION (:124-163): the same edges; computeEdgePosition (:133-142) on float(yPrev), float(yCurr), float(offset): {0, 0} where the two
 *     are equal, else crossingPos = -1 + (offset - y1) / (y2 - y1), edge_idx = round(crossingPos), edge_offset = crossingPos - edge_idx; n_fit 2.
 *   LINEAR_INTERPOLATION (:166-222): the state is (_lastState, in zone, index at which the zone was entered), accumulatedSamples = i - i_entry + 1.  A zone is
 *     entered only while none is open (yPrev <= lower && yCurr > lower while low, yPrev >= upper && yCurr < upper while high, :177-183), an edge needs an open
 *     zone (:189-190) -- a stream that starts inside the band gives no edge until it has left it on the far side once --, a zone is abandoned where the sample
 *     leaves the band on the near side (:215-217).  At an edge findCrossingIndexLinearRegression (:294-324) runs over the n = min(max(accumulated, 2), 32)
 *     newest samples, newest first, in comp_t (T for float / double, float for the integer types), every operation rounded on its own in the reference's order;
 *     relativeIndex = value_t(crossing) - value_t(n - 1) (:198; an integer T truncates the crossing, and its offset is 0), edge_idx = round(relativeIndex),
 *     edge_offset = float(relativeIndex) - float(edge_idx) (:201-205); n_fit = n.
 *   degenerate fits: a crossing that is not finite, or whose index does not fit int32 after round (an integer T: whose truncation or relativeIndex leaves T's
 *     range), is undefined behaviour in the reference (a zero slope, a NaN in the window; for BASIC a NaN yPrev).  The device reports that edge with
 *     GR4HIP_SCHMITT_DEGENERATE, edge_idx 0, edge_offset 0; the state flips as it does in the reference.
 *   a NaN sample compares false everywhere and holds the state.
 * d_in: n_in samples of params.dtype.  d_edges: room for `capacity` edges, written in order of `sample`; *d_n_edges (device memory) receives the number of edges
 * DETECTED: only the first `capacity` are written, and the state advances over the whole call either way.  n_in == 0 is OK (*d_n_edges = 0).
 * GR4HIP_UNSUPPORTED for POLYNOMIAL_INTERPOLATION (:224-289: it needs the Savitzky-Golay coefficient design, which the detector is not wired to -- gr4hip_savgol_design
 * below came later, and the error text still says the library does not have it; no other method is taken in its place).  GR4HIP_INVALID_ARGUMENT, checked on the host before any device work: a non-finite offset, a non-finite or negative threshold, an
 * unknown method or dtype, for the integer types a fractional offset / threshold or ones whose sum or difference leaves the type's range, for float ones that
 * are not finite as float.  set_params resets the detector as settingsChanged does (Trigger.hpp:76-80; the dtype is fixed at create); reset is reset() (:90-101).
 * Both are host-side notes applied by the next process call on its stream.  process queues its three launches and returns without waiting for them, with one
 * exception: the handle keeps 56 bytes of scratch per segment of the longest call so far, and a call longer than every earlier one frees and allocates it
 * again, which waits for the whole device (hipFree).  A caller that must not stall makes its longest call first. */
#define GR4HIP_SCHMITT_SEGMENT 4096 /* samples per workgroup segment: where the carries change hands (tests place their boundaries by it) */
/* the longest call: GR4HIP_INVALID_ARGUMENT beyond it, before any device work.  The carry walk's workgroups do not wait for one another: each composes the
 * segments in front of its tile itself, so that work grows with the square of the call's length (83 us of a 1.36 ms call at 2^27 samples; SCHMITT_TRIGGER.md
 * "Rates and limits").  A longer stream goes in several calls: the handle carries the state, and the edges are the same whatever the chunking. */
#define GR4HIP_SCHMITT_MAX_SAMPLES 4294967296ULL /* 2^32 */
typedef struct gr4hip_schmitt gr4hip_schmitt_t;
typedef enum { /* gr::trigger::InterpolationMethod (:17-22) */
    GR4HIP_SCHMITT_NO_INTERPOLATION = 0, GR4HIP_SCHMITT_BASIC_LINEAR_INTERPOLATION = 1, GR4HIP_SCHMITT_LINEAR_INTERPOLATION = 2,
    GR4HIP_SCHMITT_POLYNOMIAL_INTERPOLATION = 3 /* GR4HIP_UNSUPPORTED */
} gr4hip_schmitt_method;
enum { /* kind_flags: the low two bits are gr::trigger::EdgeDetection (:24) */
    GR4HIP_SCHMITT_RISING = 1, GR4HIP_SCHMITT_FALLING = 2, GR4HIP_SCHMITT_KIND_MASK = 3, GR4HIP_SCHMITT_DEGENERATE = 4
};
typedef struct {
    double offset, threshold; /* _offset, _threshold (:45-46), converted to the value type */
    int    method;            /* gr4hip_schmitt_method */
    int    dtype;             /* GR4HIP_I16, GR4HIP_I32, GR4HIP_F32 or GR4HIP_F64 (Trigger.hpp:20-22) */
} gr4hip_schmitt_params;
typedef struct {
    int64_t  sample;      /* index within this call's d_in of the sample at which processOne returned the edge */
    int32_t  edge_idx;    /* lastEdgeIdx (:56) */
    float    edge_offset; /* value(lastEdgeOffset) (:57) */
    uint32_t kind_flags;
    uint32_t n_fit;       /* the regression's n (:194); 0 for NO, 2 for BASIC */
} gr4hip_schmitt_edge;    /* 24 bytes */
int    gr4hip_schmitt_params_default(gr4hip_schmitt_params* p); /* offset 0, threshold 1 (:45-46), NO_INTERPOLATION, float */
int    gr4hip_schmitt_check(const gr4hip_schmitt_params* p);    /* host only: the validation of create */
size_t gr4hip_schmitt_segment(void);                            /* GR4HIP_SCHMITT_SEGMENT of the built library */
size_t gr4hip_schmitt_walk_tile(void);                          /* segments per workgroup of the carry walk: a call of more than this many segments has its carries
                                                                   from more than one workgroup, each composing the segments in front of its tile (tests size by it) */
int    gr4hip_schmitt_create(gr4hip_schmitt_t** h, const gr4hip_schmitt_params* p);
int    gr4hip_schmitt_set_params(gr4hip_schmitt_t* h, const gr4hip_schmitt_params* p);
int    gr4hip_schmitt_reset(gr4hip_schmitt_t* h);
int    gr4hip_schmitt_process(gr4hip_schmitt_t* h, const void* d_in, size_t n_in, gr4hip_schmitt_edge* d_edges, size_t capacity, unsigned long long* d_n_edges,
                              gr4hip_stream_t stream);
int    gr4hip_schmitt_destroy(gr4hip_schmitt_t* h);

/* ------------------------------------------------------------------------------------------------ SVD denoiser (blocks/filter/.../SvdDenoiser.hpp:14-91)
 * gr::filter::SvdDenoiser<T> over gr::algorithm::svd_filter::SvdDenoiser<T> (algorithm/filter/SvdFilter.hpp:143-236) for T in {float, double, complex<float>,
 * complex<double>}, with the Default boundary policy and default value 0 the block always uses (SvdDenoiser.hpp:58-66).  Design notes: SVD_DENOISER.md.
 *   W = max(window_size, 2), L = hankel_rows ? hankel_rows : W / 2, K = W - L + 1, hop = max(1, size_t(RealT(W) * hop_fraction)) with the product in RealT
 *   (SvdFilter.hpp:183), delay = (W - 1) / 2, safe = min(W - 1 - delay, W > hop ? W - hop : 0) (:174-176).
 *   processOne (:190-202) on every sample of the stream exactly once, whatever the chunking into calls: at every sample whose index n since the last reset is a
 *   multiple of hop the window w[0 .. W) -- the last W samples ending at n, oldest first, zeros in front of the stream -- gives H[i][j] = w[i + j]; its singular
 *   values sigma_0 >= sigma_1 >= ... rounded to RealT go through computeEffectiveRank (:43-65) in RealT arithmetic, k = min(max(rank, 1), min(L, K)); d[0 .. W) is
 *   the anti-diagonal average (hankelAverage) of the rank-k approximation (:72-115) and samples n ... n + hop - 1 output d[safe .. safe + hop), rounded to T.
 *   The device computes the singular triplets in float64 for all four types (one-sided Jacobi), so for float it gives the exact low-rank answer rounded once.
 *   An all-zero window gives zeros.  A window that holds a non-finite sample, or whose Jacobi sweeps did not converge within their fixed bound, gives quiet NaN for
 *   all of its hop outputs and is counted.
 * GR4HIP_INVALID_ARGUMENT, checked on the host before any device work: a non-finite or negative relative_threshold or absolute_threshold, a non-finite
 * energy_fraction, a hop_fraction that is not finite or outside [0, 1] (hop > W: the reference copies past its window, :178), hankel_rows > W (the reference's
 * hankel() throws), an unknown dtype, d_in and d_out overlapping (a later window reads inputs an earlier window's outputs would have overwritten).
 * GR4HIP_UNSUPPORTED from check / create / set_params: W > GR4HIP_SVDDENOISE_MAX_WINDOW for float / double, W > GR4HIP_SVDDENOISE_MAX_WINDOW_COMPLEX for the
 * complex types (the matrix lives in LDS with one lane per column); the caller keeps its CPU path.
 * set_params is setParameters (:221-229), which resets; reset is reset() (:204-212): the history is zeros again and nothing is pending.  Both are host-side notes
 * applied by the next process call on its stream.  process queues one launch and returns without waiting for it; n_out == n_in, n_in == 0 is OK.  The handle
 * carries the last W - 1 inputs and the outputs of the current hop on the device, and the position within the hop on the host.
 * stats: windows started since create (host count) and, of those, the ones that gave NaN (device counter): it queues a copy behind the handle's last process call,
 * on that call's stream, into page-locked memory and waits for that stream only. */
#define GR4HIP_SVDDENOISE_MAX_WINDOW 128
#define GR4HIP_SVDDENOISE_MAX_WINDOW_COMPLEX 64
typedef struct gr4hip_svddenoise gr4hip_svddenoise_t;
typedef struct {
    int      dtype;              /* GR4HIP_F32, GR4HIP_F64, GR4HIP_C32 or GR4HIP_C64 (SvdDenoiser.hpp:12) */
    size_t   window_size;        /* (:37) */
    size_t   hankel_rows;        /* (:38) 0: window_size / 2 */
    uint64_t max_rank;           /* (:39) */
    double   relative_threshold; /* (:41) converted to RealT */
    double   absolute_threshold; /* (:44) converted to RealT */
    double   energy_fraction;    /* (:47) converted to RealT */
    double   hop_fraction;       /* (:50) converted to RealT */
} gr4hip_svddenoise_params;
int    gr4hip_svddenoise_params_default(gr4hip_svddenoise_params* p, int dtype); /* (:37-51) 64, 0, max, eps(RealT), eps(RealT), 1, 0.25: the thresholds depend on dtype */
int    gr4hip_svddenoise_check(const gr4hip_svddenoise_params* p);               /* host only: the validation of create */
size_t gr4hip_svddenoise_windows_per_group(void);                                /* windows per workgroup of the built library (1: one wave per window) */
int    gr4hip_svddenoise_create(gr4hip_svddenoise_t** h, const gr4hip_svddenoise_params* p);   /* the block's start() (:69-74) */
int    gr4hip_svddenoise_set_params(gr4hip_svddenoise_t* h, const gr4hip_svddenoise_params* p); /* settingsChanged (:76-86) -> setParameters: a reset */
int    gr4hip_svddenoise_reset(gr4hip_svddenoise_t* h);                                          /* reset() (:88) */
int    gr4hip_svddenoise_process(gr4hip_svddenoise_t* h, const void* d_in, size_t n_in, void* d_out, gr4hip_stream_t stream); /* processOne (:90) per sample */
int    gr4hip_svddenoise_stats(gr4hip_svddenoise_t* h, unsigned long long* windows, unsigned long long* not_converged);
int    gr4hip_svddenoise_sweeps(gr4hip_svddenoise_t* h, unsigned long long* sweeps); /* Jacobi sweeps of all windows since create (as stats: waits for the handle's stream) */
int    gr4hip_svddenoise_destroy(gr4hip_svddenoise_t* h);

/* ------------------------------------------------------------------------------------------------ Signal generator (blocks/basic/.../SignalGenerator.hpp:25-87)
 * gr::basic::SignalGenerator<T> as a device source for T in {float, double, complex<float>, int16}: sample n of the stream is what the n-th call of
 * SignalGeneratorCore<T>::generateSample() returns (SignalGenerator.hpp:68-83; NOT the bulk fill() / fillComplex(), which round differently), whatever the cutting
 * of the stream into calls.  Design notes and measured bounds: SIGNAL_GENERATOR.md.
 *   compute type F (SignalGeneratorCore.hpp:27-41): double for the scalar types, float for complex<float>; the float settings are cast to F.
 *   time (ToneGenerator.hpp:47,224-225): t_0 = 0, t_{n+1} = fl(t_n + fl(1 / sample_rate)) in F, reproduced exactly from a host-built table of linear segments that
 *     covers 2^64 samples -- including the stall of F = float near n = 2^24 at 1 kHz, where the increment rounds to nothing.  Only tone samples advance it.
 *   tones (:235-255; complex :77-102): Const, Sin, Cos, Square, Saw, Triangle evaluated in F operation by operation; frequency <= 0 makes every tone Const (:48).
 *   FastSin / FastCos (:216-232): the reference multiplies a phasor by a rounded rotation once per sample and renormalises every 65536 samples.  DEVIATION: the device
 *     evaluates the closed form of the same rounded constants in float64, |rot|^(k mod 65536) exp(j (arg p0 + k arg rot)) with k the samples since configure (the
 *     magnitude starts at |p0| before the first renormalisation), and rounds once.  It differs from the recurrence by the recurrence's own rounding walk: at most
 *     1.2e-4 (complex<float>) and 6.3e-12 (double) over the first 200 000 samples at 37.5 Hz / 1 kHz, amplitude 1.5; the walk grows with the stream.
 *   noise (NoiseGenerator.hpp:78,112-118,157-164; Xoshiro256pp.hpp:32-66): one xoshiro256++ stream seeded by splitmix64; Uniform 2 u01 - 1, Triangular u01 + u01 - 1,
 *     complex: real part first; Gaussian by Marsaglia's polar method with the cached second variate (GaussianNoise.hpp:33-55), complex {A (g1 / sqrt2) + O, A (g2 / sqrt2)}.
 *     Bit for bit for Uniform and Triangular; Gaussian up to the device's log.  The stream's state lives on the device: a call continues it without a host round trip.
 *   integer T: truncated and clamped (SignalGeneratorCore.hpp:49-60).
 * check (host only; also the first step of create / configure): GR4HIP_INVALID_ARGUMENT for a non-finite setting, sample_rate <= 0, an unknown signal type or dtype,
 *   and for a sample_rate whose reciprocal is not finite in F.  DEVIATION: the reference would compute with inf / NaN there.  GR4HIP_UNSUPPORTED for every other
 *   registered sample type.
 * create is the block's start(): configure + reset.  configure is settingsChanged (the mirror's, gr4/blocks.hpp): the noise is re-seeded, the spare dropped, the
 *   phasor and its count start again; the time base keeps running (from the current time with the new tick when sample_rate changed); dtype is fixed.  reset also
 *   zeroes the time.  Both are host-side notes that the next process call applies on its stream.
 * process queues a fixed number of launches (1 for Const and the tones, 2 for Uniform / Triangular, 4 for Gaussian; the first call after create / configure /
 *   reset also carries the new seed state and time table to the device, as the arguments of small launches) and returns without waiting; d_out needs the
 *   alignment of its sample type only (4 bytes for complex<float>); n == 0 is a no-op; n <= 2^40 per call.
 * GR4HIP_SIGGEN_GAUSS_PERMILLE (gr4hip_developer_switch) sets how many attempts the parallel Gaussian kernels test per 1000 needed pairs; a tail kernel, queued in
 *   every call, finishes sequentially what they did not give, so the values do not depend on it. */
typedef struct gr4hip_siggen gr4hip_siggen_t;
typedef enum { /* SignalGeneratorCore.hpp:16 */
    GR4HIP_SIGGEN_CONST = 0, GR4HIP_SIGGEN_SIN, GR4HIP_SIGGEN_COS, GR4HIP_SIGGEN_SQUARE, GR4HIP_SIGGEN_SAW, GR4HIP_SIGGEN_TRIANGLE, GR4HIP_SIGGEN_FAST_SIN,
    GR4HIP_SIGGEN_FAST_COS, GR4HIP_SIGGEN_UNIFORM_NOISE, GR4HIP_SIGGEN_TRIANGULAR_NOISE, GR4HIP_SIGGEN_GAUSSIAN_NOISE
} gr4hip_siggen_type;
typedef struct {
    int                dtype;       /* GR4HIP_F32, GR4HIP_F64, GR4HIP_C32 or GR4HIP_I16 */
    int                signal_type; /* gr4hip_siggen_type */
    float              sample_rate, frequency, amplitude, offset, phase; /* SignalGenerator.hpp:40-46 */
    unsigned long long seed;        /* (:47) */
} gr4hip_siggen_params;
int    gr4hip_siggen_check(const gr4hip_siggen_params* p);                            /* host only: the validation of create */
int    gr4hip_siggen_create(gr4hip_siggen_t** h, const gr4hip_siggen_params* p);      /* start() (SignalGenerator.hpp:57-61): configure + reset */
int    gr4hip_siggen_configure(gr4hip_siggen_t* h, const gr4hip_siggen_params* p);    /* settingsChanged (:63-66): the time keeps running */
int    gr4hip_siggen_reset(gr4hip_siggen_t* h);                                       /* reset() (SignalGeneratorCore.hpp:90-93) */
int    gr4hip_siggen_process(gr4hip_siggen_t* h, void* d_out, size_t n, gr4hip_stream_t stream); /* n x generateSample() (:68-83, SignalGeneratorCore.hpp:95-106) */
void   gr4hip_siggen_destroy(gr4hip_siggen_t* h);
size_t gr4hip_siggen_run(void);  /* consecutive samples one lane generates */
size_t gr4hip_siggen_tile(void); /* samples of one workgroup: where the start states change hands */
/* host-only helpers (no device): the xoshiro256++ state n_draws draws further on (Xoshiro256pp.hpp:41-52 applied n_draws times, through the T^(2^k) matrices), and
 * the reference's time t_n (ToneGenerator.hpp:224-225) for n = n0 .. n0 + count - 1 from the segment table, as double (exact for F = float) */
int    gr4hip_siggen_jump_host(const unsigned long long in[4], unsigned long long n_draws, unsigned long long out[4]);
int    gr4hip_siggen_time_host(int dtype, float sample_rate, unsigned long long n0, size_t count, double* t_out);

/* ------------------------------------------------------------------------------------------------ Type converters (blocks/basic/.../ConverterBlocks.hpp:13-277)
 * The fourteen blocks of gr::blocks::type::converter as ONE streaming kernel family: load -> optional prologue program -> conversion -> optional epilogue program ->
 * store.  Semantics, deviations and measured bounds: CONVERTERS.md.  An ITEM is what one processOne call consumes per input port: one sample, except for the two
 * interleaved kinds, whose interleaved port carries two elements per item (Resampling<1, 2, true> / <2, 1, true>, :237, :260).
 *   Convert / ScalingConvert (:15-59): static_cast<R>(input * scale), the product in the PROMOTED type of T (int for the 8- and 16-bit types), scale of type T
 *     (1 for Convert: x * 1 is x bit for bit, so both kinds share one set of kernels).  All 10 x 10 arithmetic pairs.
 *   Abs (:63-81): unsigned T through its signed type and narrowed back; float / double: the sign bit cleared; complex: hypot.  12 types.
 *   Real, Imag, Arg (:85-126), ToRealImag (:164-178), ToMagPhase (:199-213): complex<float>, complex<double>.  Arg is atan2(im, re) with signed zeros.
 *   RadiansToDegree, DegreeToRadians (:130-160): (x / pi) * 180 and (x / 180) * pi, two IEEE operations in this order.  float, double.
 *   RealImagToComplex (:182-195), MagPhaseToComplex (:217-231: {r cos t, r sin t}): float, double.
 *   ComplexToInterleaved (:235-254), InterleavedToComplex (:258-277): {complex<float>, complex<double>} x {float, double, int8, int16} (the templates' constraint,
 *     wider than their registration), a static_cast per component.
 * DEVIATIONS (undefined in the reference, defined here): float -> integer saturates and NaN -> 0; signed overflow of input * scale and of abs wraps modulo 2^w.
 * complex<float> / float transcendentals (Abs, Arg, ToMagPhase, MagPhaseToComplex) are evaluated in float64 on the float arguments and rounded once.
 * check (host only; also the first step of create): GR4HIP_INVALID_ARGUMENT for an unknown kind or dtype and for every kind / dtype pair the requires clauses
 *   exclude; out_dtype must be the block's R.
 * process: d_in / d_out are arrays of n_in-port / n_out-port device pointers (gr4hip_convert_ports), each with the alignment of its ELEMENT type only.  A NULL
 *   entry of d_out is an unconnected port and is skipped.  n_in counts elements of input 0 (an odd count is GR4HIP_INVALID_ARGUMENT for InterleavedToComplex);
 *   *n_out receives the elements written to output 0.  One launch, no wait.
 * set_prologue / set_epilogue copy the program (as gr4hip_fir_set_prologue); NULL takes it off.  The prologue's dtype must be in_dtype and the kind must have one
 *   input, the epilogue's out_dtype and one output (else GR4HIP_UNSUPPORTED).  A rotator op sees the absolute index of the (complex) sample since create / reset.
 * set_scale / set_* / reset are host-side notes: the next process call carries them on its stream. */
typedef struct gr4hip_convert gr4hip_convert_t;
typedef enum {
    GR4HIP_CONVERT = 0, GR4HIP_SCALING_CONVERT, GR4HIP_CONVERT_ABS, GR4HIP_CONVERT_REAL, GR4HIP_CONVERT_IMAG, GR4HIP_CONVERT_ARG, GR4HIP_RADIANS_TO_DEGREE,
    GR4HIP_DEGREE_TO_RADIANS, GR4HIP_TO_REAL_IMAG, GR4HIP_REAL_IMAG_TO_COMPLEX, GR4HIP_TO_MAG_PHASE, GR4HIP_MAG_PHASE_TO_COMPLEX, GR4HIP_COMPLEX_TO_INTERLEAVED,
    GR4HIP_INTERLEAVED_TO_COMPLEX
} gr4hip_convert_kind;
typedef struct {
    int    kind;      /* gr4hip_convert_kind */
    int    in_dtype;  /* T of the input port(s) */
    int    out_dtype; /* R of the output port(s) */
    double scale;     /* ScalingConvert::scale (:46), converted to in_dtype; ignored by the other kinds */
} gr4hip_convert_params;
int    gr4hip_convert_params_default(gr4hip_convert_params* p, int kind, int in_dtype); /* out_dtype = the block's R (in_dtype for the two-type kinds), scale = 1 (:46) */
int    gr4hip_convert_params_check(const gr4hip_convert_params* p);                      /* host only: the requires clauses (:16, :38, :64, :130, :236, :259) */
int    gr4hip_convert_create(gr4hip_convert_t** h, const gr4hip_convert_params* p);
int    gr4hip_convert_destroy(gr4hip_convert_t* h);
int    gr4hip_convert_set_scale(gr4hip_convert_t* h, double scale);                      /* settingsChanged of ScalingConvert::scale (:46) */
int    gr4hip_convert_reset(gr4hip_convert_t* h);                                        /* stream position back to 0 (only rotator ops of the hooks read it) */
int    gr4hip_convert_ports(const gr4hip_convert_t* h, size_t* n_in, size_t* n_out, size_t* in_chunk, size_t* out_chunk); /* GR_MAKE_REFLECTABLE port lists; Resampling<> chunks */
int    gr4hip_convert_process(gr4hip_convert_t* h, const void* const* d_in, void* const* d_out, size_t n_in, size_t* n_out, gr4hip_stream_t stream); /* processOne / processBulk (:25, :51, :73, :95, :110, :125, :140, :157, :175, :192, :210, :228, :247, :271) */
int    gr4hip_convert_set_prologue(gr4hip_convert_t* h, const gr4hip_ewise_t* prog);     /* Merge<A, "out", Convert, "in"> (BlockMerging.hpp:126-240) */
int    gr4hip_convert_set_epilogue(gr4hip_convert_t* h, const gr4hip_ewise_t* prog);     /* Merge<Convert, "out", B, "in"> */
size_t gr4hip_convert_tile(const gr4hip_convert_params* p);                              /* items one workgroup of the aligned body converts (0: invalid params) */

/* ------------------------------------------------------------------------------------------------ Savitzky-Golay (blocks/filter/.../SavitzkyGolayFilter.hpp:17-164)
 * gr::filter::SavitzkyGolayFilter<T> and SavitzkyGolayDataSetFilter<T> over algorithm/filter/SavitzkyGolay.hpp, T in {float, double}.  Design notes, the evidence
 * for the truncation rule and the measured bounds: SAVITZKY_GOLAY.md.
 * gr4hip_savgol_design (host only, no device) restates computeCoefficients<T> (SavitzkyGolay.hpp:93-151):
 *   W = max(window_size, 1), p = min(poly_order, W - 1), d = min(deriv_order, p), delta = max(T(delta), eps_T) (:95-98: delta <= 0 is clamped, not refused);
 *   D = (W - 1) / 2 for Centred, W - 1 for Causal (:105); A[i][j] = (i - D)^j by the running product (:108-115), in float64;
 *   the singular values of A come from a one-sided Jacobi in float64, and sigma_k is dropped when sigma_k < eps_T max(W, p + 1) sigma_0 (:128-133) with T's
 *   epsilon: the reference's float design truncates at ordinary settings (W 51, p 4 keeps 4 of 5), and the truncated filter is the one it computes with;
 *   row d of the truncated pseudo-inverse is rounded to T, then multiplied in T by T(d!) / std::pow(delta, T(d)) (:147-148; d! in size_t arithmetic, :43-49);
 *   h_coeffs_out receives W values of T, coeffs[k] belonging to the offset k - D.
 *   info_out (may be NULL): the clamped settings, the kept rank, sigma_0, the smallest kept sigma, the threshold, and `ambiguous`: some sigma_k lies within
 *   16 eps_T sigma_0 of the threshold, where the reference's own T-precision SVD could decide either way.  16 is a chosen safety factor over the ~ eps sigma_0
 *   error of a backward-stable SVD, not a measured one.  The flag is information: nothing is refused because of it.
 *   GR4HIP_INVALID_ARGUMENT: a dtype other than F32 / F64, an unknown alignment, a NULL output.  GR4HIP_UNSUPPORTED: W (p + 1) > 2^22, or a power that is not finite.
 * gr4hip_savgol_pinv_row: the same row of the same truncated pseudo-inverse in float64, before the rounding to T and the scale (what the tests bound).
 * gr4hip_savgol_zp_*: applyZeroPhase (:177-193) as the DataSet block calls it (SavitzkyGolayFilter.hpp:121-137, 154-159: Centred, delta 1), on each of `batch` rows
 *   of n samples, row r at d_in / d_out + r * row_stride samples:
 *     t[j] = sum_k c[k] x[b(j + k - D)], rounded to T (the reference's std::vector<T> temp); out[n] = sum_k c[k] t[b(n - k + D)]
 *   with b = reflectIndex / replicateIndex (:51-77) -- the literal apply, reverse, apply, reverse.  Both passes are one launch, sums in float64 for both types, and
 *   t stays in LDS.  Rows need the alignment of T only; nothing outside the n samples of a row is read or written.  process queues the launch and returns without
 *   waiting.  n == 0 (or batch == 0) is a no-op returning OK (:180).  The coefficients travel in the kernel's arguments, so set_params (settingsChanged, :142-147)
 *   is a host-side note and the handle owns no device memory; the dtype is fixed at create.
 *   GR4HIP_UNSUPPORTED from create / set_params: max(window_size, 1) > GR4HIP_SAVGOL_ZP_MAX_WINDOW (the caller keeps its CPU path).  GR4HIP_INVALID_ARGUMENT: an unknown
 *   dtype or boundary policy, a buffer not aligned to its samples, row_stride < n with more than one row, d_in and d_out overlapping, more than 2^31 - 1 tiles.
 * The streaming block has no entry point of its own: processOne (SavitzkyGolay.hpp:226-233) with the Default boundary policy the block always uses
 *   (SavitzkyGolayFilter.hpp:48-57) is y[n] = sum_k c[k] x[n - (W - 1) + k] over a history of zeros, i.e. fir_filter with b[k] = c[W - 1 - k]: gr4hip_fir_* with
 *   GR4HIP_FIR_EXACT_F32 for float, gr4hip_fir64_* for double.  A settings change calls set_taps AND reset, because setParameters clears the history (:253-260). */
#define GR4HIP_SAVGOL_ZP_MAX_WINDOW 255
typedef enum { GR4HIP_SAVGOL_CENTRED = 0, GR4HIP_SAVGOL_CAUSAL = 1 } gr4hip_savgol_alignment;   /* algorithm::savitzky_golay::Alignment (:19-22) */
typedef enum { GR4HIP_SAVGOL_REFLECT = 0, GR4HIP_SAVGOL_REPLICATE = 1 } gr4hip_savgol_boundary; /* the two BoundaryPolicy values the DataSet block sets (:126-128) */
typedef struct {
    size_t window_size, poly_order, deriv_order; /* after the clamps */
    size_t rank;                                 /* singular values kept */
    double sigma_max, sigma_min_kept, threshold; /* sigma_0, the smallest kept one, eps_T max(W, p + 1) sigma_0 */
    int    ambiguous;
} gr4hip_savgol_info;
typedef struct {
    int    dtype;                                /* GR4HIP_F32 or GR4HIP_F64 (SavitzkyGolayFilter.hpp:87) */
    size_t window_size, poly_order, deriv_order; /* (:111-113) */
    int    boundary_policy;                      /* gr4hip_savgol_boundary (:114: "Replicate", anything else is Reflect) */
} gr4hip_savgol_zp_params;
typedef struct gr4hip_savgol_zp gr4hip_savgol_zp_t;
int    gr4hip_savgol_design(int dtype, size_t window_size, size_t poly_order, size_t deriv_order, double delta, int alignment, void* h_coeffs_out,
                            gr4hip_savgol_info* info_out);
int    gr4hip_savgol_pinv_row(int dtype, size_t window_size, size_t poly_order, size_t deriv_order, int alignment, double* h_row_out, gr4hip_savgol_info* info_out);
size_t gr4hip_savgol_zp_tile(void); /* outputs per workgroup: a row of at most this many samples is one workgroup's (tests place their edges by it) */
int    gr4hip_savgol_zp_create(gr4hip_savgol_zp_t** h, const gr4hip_savgol_zp_params* p);     /* start() -> updateCoefficients (:132-140) */
int    gr4hip_savgol_zp_set_params(gr4hip_savgol_zp_t* h, const gr4hip_savgol_zp_params* p); /* settingsChanged (:142-147) */
int    gr4hip_savgol_zp_coeffs(const gr4hip_savgol_zp_t* h, void* h_coeffs_out, gr4hip_savgol_info* info_out); /* the W coefficients in T the handle filters with */
int    gr4hip_savgol_zp_process(gr4hip_savgol_zp_t* h, const void* d_in, void* d_out, size_t n, size_t batch, size_t row_stride, gr4hip_stream_t stream); /* processOne (:149-163) */
int    gr4hip_savgol_zp_destroy(gr4hip_savgol_zp_t* h);

#ifdef __cplusplus
}
#endif
#endif /* GR4HIP_H */
