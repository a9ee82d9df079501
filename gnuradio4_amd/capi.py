"""ctypes binding of libgr4hip.so (include/gr4hip.h).  The HIP kernel library is mandatory: there is no CPU fallback
in this package -- a missing or unloadable library raises immediately (tests on a GPU box must exercise native code)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgr4hip.so")

OK, DONE, INSUFFICIENT_INPUT, INSUFFICIENT_OUTPUT = 0, -1, -2, -3
ERROR, INVALID_ARGUMENT, RUNTIME_ERROR, UNSUPPORTED, NO_DEVICE = -100, -101, -102, -103, -104
U8, U16, U32, U64, I8, I16, I32, I64, F32, F64, C32, C64, UF32, UF64 = range(14)  # UF32 / UF64: gr::UncertainValue<float | double>, {value, uncertainty} pairs
ADD, SUB, MUL, DIV = range(4)
DF_I, DF_II, DF_I_TRANSPOSED, DF_II_TRANSPOSED = range(4)
WINDOWS = ["None", "Rectangular", "Hamming", "Hann", "HannExp", "Blackman", "Nuttall", "BlackmanHarris",
           "BlackmanNuttall", "FlatTop", "Exponential", "Kaiser"]
FFT_OUTPUT_IN_DB, FFT_OUTPUT_IN_DEG, FFT_UNWRAP_PHASE = 1, 2, 4
SPECINT_MEAN = 1
IFFT_SCALE = 1
XCORR_MEAN = 1
XCORR_MAX_STREAMS = 32
CHAIN_AUTO, CHAIN_UNFUSED, CHAIN_FUSED_TD, CHAIN_FUSED_FD, CHAIN_TIME_DOMAIN = range(5)
GUARD_STRICT, GUARD_DEFERRED, GUARD_OFF = range(3)
FIR_AUTO, FIR_TIME_DOMAIN, FIR_EXACT_F32, FIR_TIME_DOMAIN_F32, FIR_TIME_DOMAIN_BF16X3 = range(5)
ROTATOR_CLOSED_FORM, ROTATOR_RECURRENCE = range(2)
IIR_AUTO, IIR_PARALLEL, IIR_SEQUENTIAL_F32 = range(3)
FIR_IIR_AUTO, FIR_IIR_ONE_LAUNCH, FIR_IIR_TWO_LAUNCHES = range(3)
SYNTH_MIX = 0xd1b54a32d192ed03  # group g of a synth stream: Xoshiro256pp(seed ^ SYNTH_MIX * (g + 1)) (include/gr4hip.h)


class Gr4HipError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str):
        self.status = status
        super().__init__(f"{where}: status {status} ({detail})")


# every symbol include/gr4hip.h declares: (name, restype, argtypes)
_vp, _sz, _i, _f, _d = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_double
_pvp, _psz, _pi, _pf = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_float)
SIGNATURES = {
    "gr4hip_abi_version": (_i, []),
    "gr4hip_last_error": (C.c_char_p, []),
    "gr4hip_status_string": (C.c_char_p, [_i]),
    "gr4hip_device_count": (_i, [_pi]),
    "gr4hip_set_device": (_i, [_i]),
    "gr4hip_get_device": (_i, [_pi]),
    "gr4hip_device_name": (_i, [_i, C.c_char_p, _sz]),
    "gr4hip_malloc": (_i, [_pvp, _sz]),
    "gr4hip_free": (_i, [_vp]),
    "gr4hip_malloc_host": (_i, [_pvp, _sz]),
    "gr4hip_free_host": (_i, [_vp]),
    "gr4hip_host_ring_create": (_i, [_pvp, _sz]),
    "gr4hip_host_ring_destroy": (_i, [_vp, _sz]),
    "gr4hip_memcpy_h2d": (_i, [_vp, _vp, _sz, _vp]),
    "gr4hip_memcpy_d2h": (_i, [_vp, _vp, _sz, _vp]),
    "gr4hip_memcpy_d2d": (_i, [_vp, _vp, _sz, _vp]),
    "gr4hip_memset": (_i, [_vp, _i, _sz, _vp]),
    "gr4hip_stream_create": (_i, [_pvp]),
    "gr4hip_stream_destroy": (_i, [_vp]),
    "gr4hip_stream_synchronize": (_i, [_vp]),
    "gr4hip_stream_query": (_i, [_vp, C.POINTER(C.c_int)]),
    "gr4hip_event_create": (_i, [_pvp]),
    "gr4hip_event_destroy": (_i, [_vp]),
    "gr4hip_event_record": (_i, [_vp, _vp]),
    "gr4hip_event_synchronize": (_i, [_vp]),
    "gr4hip_event_query": (_i, [_vp, _pi]),
    "gr4hip_stream_wait_event": (_i, [_vp, _vp]),
    "gr4hip_event_elapsed_ms": (_i, [_vp, _vp, _pf]),
    "gr4hip_ring_create": (_i, [_pvp, _sz]),
    "gr4hip_ring_destroy": (_i, [_vp]),
    "gr4hip_ring_base": (_i, [_vp, _pvp]),
    "gr4hip_ring_size": (_i, [_vp, _psz]),
    "gr4hip_fir64_create": (_i, [_pvp, _vp, _sz, _sz]),
    "gr4hip_fir64_set_taps": (_i, [_vp, _vp, _sz]),
    "gr4hip_fir64_reset": (_i, [_vp]),
    "gr4hip_fir64_process": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_fir64_destroy": (_i, [_vp]),
    "gr4hip_iir64_create": (_i, [_pvp, _i, _sz, _vp, _sz, _vp, _sz]),
    "gr4hip_iir64_reset": (_i, [_vp]),
    "gr4hip_iir64_process": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "gr4hip_iir64_destroy": (_i, [_vp]),
    "gr4hip_fft64_create": (_i, [_pvp, _sz, _i, _i]),
    "gr4hip_fft64_process": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "gr4hip_fft64_destroy": (_i, [_vp]),
    "gr4hip_rotator64_create": (_i, [_pvp, _d, _d]),
    "gr4hip_rotator64_reset": (_i, [_vp, _d]),
    "gr4hip_rotator64_process": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "gr4hip_rotator64_phase": (_i, [_vp, C.POINTER(C.c_double)]),
    "gr4hip_rotator64_destroy": (_i, [_vp]),
    "gr4hip_fir_create": (_i, [_pvp, _i, _vp, _sz, _sz]),
    "gr4hip_fir_set_taps": (_i, [_vp, _vp, _sz]),
    "gr4hip_fir_set_algo": (_i, [_vp, _i]),
    "gr4hip_fir_reset": (_i, [_vp]),
    "gr4hip_fir_process": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_fir_destroy": (_i, [_vp]),
    "gr4hip_fir_interp_create": (_i, [_pvp, _i, _vp, _sz, _sz]),
    "gr4hip_fir_interp_set_taps": (_i, [_vp, _vp, _sz]),
    "gr4hip_fir_interp_reset": (_i, [_vp]),
    "gr4hip_fir_interp_process": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_fir_interp_destroy": (_i, [_vp]),
    "gr4hip_resamp_create": (_i, [_pvp, _i, _vp, _sz, _sz, _sz]),
    "gr4hip_resamp_set_taps": (_i, [_vp, _vp, _sz]),
    "gr4hip_resamp_reset": (_i, [_vp]),
    "gr4hip_resamp_process": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_resamp_destroy": (_i, [_vp]),
    "gr4hip_resamp_tile": (_sz, []),
    "gr4hip_resamp_design": (_i, [_vp, _sz, _psz, _sz, _sz, _sz, _i, _d]),
    "gr4hip_cfir_create": (_i, [_pvp, _vp, _sz, _sz]),
    "gr4hip_cfir_set_taps": (_i, [_vp, _vp, _sz]),
    "gr4hip_cfir_reset": (_i, [_vp]),
    "gr4hip_cfir_set_guard_mode": (_i, [_vp, _i]),
    "gr4hip_cfir_process": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_cfir_destroy": (_i, [_vp]),
    "gr4hip_cfir_tile": (_sz, []),
    "gr4hip_cfir_segment": (_sz, []),
    "gr4hip_cfir_band_table": (_i, [_vp, _sz, _sz, _vp, _sz, _psz, C.POINTER(C.c_long)]),
    "gr4hip_pfb_design": (_i, [_vp, _sz, _sz, _i, _f]),
    "gr4hip_pfb_create": (_i, [_pvp, _i, _sz, _sz, _vp, _i]),
    "gr4hip_pfb_set_taps": (_i, [_vp, _vp, _sz]),
    "gr4hip_pfb_reset": (_i, [_vp]),
    "gr4hip_pfb_process": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "gr4hip_pfb_destroy": (_i, [_vp]),
    "gr4hip_ifft_create": (_i, [_pvp, _i, _sz, _i, _i]),
    "gr4hip_ifft_process": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "gr4hip_ifft_destroy": (_i, [_vp]),
    "gr4hip_pfb_synth_create": (_i, [_pvp, _sz, _sz, _vp, _i]),
    "gr4hip_pfb_synth_set_taps": (_i, [_vp, _vp, _sz]),
    "gr4hip_pfb_synth_reset": (_i, [_vp]),
    "gr4hip_pfb_synth_process": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "gr4hip_pfb_synth_destroy": (_i, [_vp]),
    "gr4hip_specint_create": (_i, [_pvp, _sz, _sz, _i]),
    "gr4hip_specint_reset": (_i, [_vp]),
    "gr4hip_specint_set_length": (_i, [_vp, _sz]),
    "gr4hip_specint_pending": (_i, [_vp, _sz, _psz]),
    "gr4hip_specint_process": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_specint_destroy": (_i, [_vp]),
    "gr4hip_specint_leaf": (_sz, []),
    "gr4hip_fft_mag2_integrate": (_i, [_vp, _vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_pfb_power_integrate": (_i, [_vp, _vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_stft_create": (_i, [_pvp, _i, _sz, _sz, _i, _i]),
    "gr4hip_stft_reset": (_i, [_vp]),
    "gr4hip_stft_pending": (_i, [_vp, _sz, _psz]),
    "gr4hip_stft_process": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _psz, _vp]),
    "gr4hip_stft_spectrum": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_stft_mag2": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_stft_mag2_integrate": (_i, [_vp, _vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_stft_destroy": (_i, [_vp]),
    "gr4hip_xcorr_create": (_i, [_pvp, _sz, _sz, _sz, _i]),
    "gr4hip_xcorr_reset": (_i, [_vp]),
    "gr4hip_xcorr_set_length": (_i, [_vp, _sz]),
    "gr4hip_xcorr_pending": (_i, [_vp, _sz, _psz]),
    "gr4hip_xcorr_process": (_i, [_vp, _pvp, _sz, _vp, _psz, _vp]),
    "gr4hip_xcorr_destroy": (_i, [_vp]),
    "gr4hip_xcorr_leaf": (_sz, []),
    "gr4hip_xcorr_coherence": (_i, [_vp, _sz, _sz, _sz, _sz, _sz, _vp, _vp, _vp]),
    "gr4hip_beamform_create": (_i, [_pvp, _sz, _sz, _sz]),
    "gr4hip_beamform_set_weights": (_i, [_vp, _vp, _vp]),
    "gr4hip_beamform_process": (_i, [_vp, _pvp, _sz, _pvp, _sz, _vp]),
    "gr4hip_beamform_power_integrate": (_i, [_vp, _vp, _pvp, _sz, _vp, _psz, _vp]),
    "gr4hip_beamform_destroy": (_i, [_vp]),
    "gr4hip_mvdr_create": (_i, [_pvp, _sz, _sz, _sz]),
    "gr4hip_mvdr_set_steering": (_i, [_vp, _vp, _vp]),
    "gr4hip_mvdr_set_loading": (_i, [_vp, _d]),
    "gr4hip_mvdr_process": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "gr4hip_mvdr_stats": (_i, [_vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "gr4hip_mvdr_destroy": (_i, [_vp]),
    "gr4hip_decimate": (_i, [_i, _vp, _sz, _sz, _vp, _psz, _vp]),
    "gr4hip_iir_create": (_i, [_pvp, _i, _sz, _vp, _sz, _vp, _sz]),
    "gr4hip_iir_reset": (_i, [_vp]),
    "gr4hip_iir_process": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "gr4hip_iir_status": (_i, [_vp, _vp]),
    "gr4hip_iir_set_algo": (_i, [_vp, _i]),
    "gr4hip_iir_get_algo": (_i, [_vp, _pi, _pf, _pf]),
    "gr4hip_iir_destroy": (_i, [_vp]),
    "gr4hip_fir_iir_process": (_i, [_vp, _vp, _vp, _sz, _vp, _psz, _i, _vp]),
    "gr4hip_filter_params_default": (_i, [_vp]),
    "gr4hip_fir_design": (_i, [_i, _vp, _i, _vp, _sz, _psz]),
    "gr4hip_iir_design": (_i, [_i, _vp, _i, _vp, _vp, _sz, _psz]),
    "gr4hip_fft_create": (_i, [_pvp, _i, _sz, _i, _i]),
    "gr4hip_fft_process": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gr4hip_fft_spectrum": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "gr4hip_fft_mag2": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "gr4hip_fft_set_epilogue": (_i, [_vp, _vp]),
    "gr4hip_fft_destroy": (_i, [_vp]),
    "gr4hip_fft_plan": (_i, [_sz, _pi, _vp, _pi]),
    "gr4hip_window_create": (_i, [_i, _vp, _sz, _f]),
    "gr4hip_window_create_f64": (_i, [_i, _vp, _sz, _d]),
    "gr4hip_chain_create": (_i, [_pvp, _vp, _sz, _sz, _i, _i]),
    "gr4hip_chain_reset": (_i, [_vp]),
    "gr4hip_chain_process": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_chain_get_algo": (_i, [_vp, _pi]),
    "gr4hip_chain_last_power_ratio": (_i, [_vp, _pf, _pi, _vp]),
    "gr4hip_chain_last_guard_fractions": (_i, [_vp, _pf, _pf, _vp]),
    "gr4hip_chain_set_max_workgroups": (_i, [_vp, C.c_uint]),
    "gr4hip_chain_set_guard_mode": (_i, [_vp, _i]),
    "gr4hip_fir_set_guard_mode": (_i, [_vp, _i]),
    "gr4hip_developer_switch": (_i, [C.c_char_p, _i]),
    "gr4hip_chain_process_multi": (_i, [_vp, _sz, _vp, _sz, _vp, _vp, _psz, _vp]),
    "gr4hip_chain_destroy": (_i, [_vp]),
    "gr4hip_fanin_unique_id": (_i, [_vp]),
    "gr4hip_fanin_create": (_i, [_pvp, _vp, _i, _i]),
    "gr4hip_fanin_rank": (_i, [_vp, _pi, _pi]),
    "gr4hip_fanin_reduce_scatter_sum_f32": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "gr4hip_fanin_all_to_all_sum_f32": (_i, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "gr4hip_fanin_all_reduce_sum_f32": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "gr4hip_fanin_destroy": (_i, [_vp]),
    "gr4hip_math_const": (_i, [_i, _i, _vp, _vp, _sz, _vp, _vp]),
    "gr4hip_math_nary": (_i, [_i, _i, _vp, _sz, _vp, _sz, _vp]),
    "gr4hip_ewise_create": (_i, [_pvp, _i]),
    "gr4hip_ewise_append_const": (_i, [_vp, _i, _vp]),
    "gr4hip_ewise_append_rotator": (_i, [_vp, _f, _f]),
    "gr4hip_ewise_length": (_i, [_vp, _psz]),
    "gr4hip_ewise_reset": (_i, [_vp]),
    "gr4hip_ewise_position": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "gr4hip_ewise_process": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "gr4hip_ewise_decimate": (_i, [_vp, _vp, _sz, _sz, _vp, _psz, _vp]),
    "gr4hip_ewise_destroy": (_i, [_vp]),
    "gr4hip_fir_set_prologue": (_i, [_vp, _vp]),
    "gr4hip_fir_set_epilogue": (_i, [_vp, _vp]),
    "gr4hip_rotator_create": (_i, [_pvp, _f, _f]),
    "gr4hip_rotator_set_algo": (_i, [_vp, _i]),
    "gr4hip_rotator_reset": (_i, [_vp, _f]),
    "gr4hip_rotator_process": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "gr4hip_rotator_phase": (_i, [_vp, _pf, _vp]),
    "gr4hip_rotator_destroy": (_i, [_vp]),
    "gr4hip_fir_batched_create": (_i, [_pvp, _sz, _vp, _sz]),
    "gr4hip_fir_batched_reset": (_i, [_vp]),
    "gr4hip_fir_batched_process": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _vp]),
    "gr4hip_fir_batched_destroy": (_i, [_vp]),
    "gr4hip_synth_draws": (_i, [_vp, _sz, C.c_uint64, C.c_uint64, _vp]),
    "gr4hip_synth_c32": (_i, [_vp, _sz, C.c_uint64, _d, _f, _f, _vp]),
    "gr4hip_synth_f32": (_i, [_vp, _sz, C.c_uint64, _d, _f, _f, _vp]),
    "gr4hip_freqest_params_default": (_i, [_i, _vp]),
    "gr4hip_freqest_geometry": (_i, [_i, _vp, _psz, _psz, _psz]),
    "gr4hip_freqest_create": (_i, [_pvp, _i, _vp]),
    "gr4hip_freqest_set_params": (_i, [_vp, _vp]),
    "gr4hip_freqest_reset": (_i, [_vp]),
    "gr4hip_freqest_process": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "gr4hip_freqest_destroy": (_i, [_vp]),
    "gr4hip_iqdemod_params_default": (_i, [_vp]),
    "gr4hip_iqdemod_check": (_i, [_i, _vp]),
    "gr4hip_iqdemod_create": (_i, [_pvp, _i, _vp]),
    "gr4hip_iqdemod_set_params": (_i, [_vp, _vp, _i]),
    "gr4hip_iqdemod_reset": (_i, [_vp]),
    "gr4hip_iqdemod_process": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _psz, _vp]),
    "gr4hip_iqdemod_destroy": (_i, [_vp]),
    "gr4hip_powermetrics_params_default": (_i, [_vp]),
    "gr4hip_powermetrics_check": (_i, [_vp]),
    "gr4hip_powermetrics_segment": (_sz, []),
    "gr4hip_powermetrics_create": (_i, [_pvp, _vp]),
    "gr4hip_powermetrics_set_params": (_i, [_vp, _vp]),
    "gr4hip_powermetrics_reset": (_i, [_vp]),
    "gr4hip_powermetrics_process": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _psz, _vp]),
    "gr4hip_powermetrics_destroy": (_i, [_vp]),
    "gr4hip_powerfactor_process": (_i, [_i, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _vp]),
    "gr4hip_unbalance_process": (_i, [_i, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    "gr4hip_electrical_tile": (_sz, []),
    "gr4hip_schmitt_params_default": (_i, [_vp]),
    "gr4hip_schmitt_check": (_i, [_vp]),
    "gr4hip_schmitt_segment": (_sz, []),
    "gr4hip_schmitt_walk_tile": (_sz, []),
    "gr4hip_schmitt_create": (_i, [_pvp, _vp]),
    "gr4hip_schmitt_set_params": (_i, [_vp, _vp]),
    "gr4hip_schmitt_reset": (_i, [_vp]),
    "gr4hip_schmitt_process": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "gr4hip_schmitt_destroy": (_i, [_vp]),
    "gr4hip_svddenoise_params_default": (_i, [_vp, _i]),
    "gr4hip_svddenoise_check": (_i, [_vp]),
    "gr4hip_svddenoise_windows_per_group": (_sz, []),
    "gr4hip_svddenoise_create": (_i, [_pvp, _vp]),
    "gr4hip_svddenoise_set_params": (_i, [_vp, _vp]),
    "gr4hip_svddenoise_reset": (_i, [_vp]),
    "gr4hip_svddenoise_process": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "gr4hip_svddenoise_stats": (_i, [_vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "gr4hip_svddenoise_sweeps": (_i, [_vp, C.POINTER(C.c_ulonglong)]),
    "gr4hip_svddenoise_destroy": (_i, [_vp]),
    "gr4hip_siggen_check": (_i, [_vp]),
    "gr4hip_siggen_create": (_i, [_pvp, _vp]),
    "gr4hip_siggen_configure": (_i, [_vp, _vp]),
    "gr4hip_siggen_reset": (_i, [_vp]),
    "gr4hip_siggen_process": (_i, [_vp, _vp, _sz, _vp]),
    "gr4hip_siggen_destroy": (None, [_vp]),
    "gr4hip_siggen_run": (_sz, []),
    "gr4hip_siggen_tile": (_sz, []),
    "gr4hip_siggen_jump_host": (_i, [C.POINTER(C.c_ulonglong), C.c_ulonglong, C.POINTER(C.c_ulonglong)]),
    "gr4hip_siggen_time_host": (_i, [_i, _f, C.c_ulonglong, _sz, C.POINTER(C.c_double)]),
    "gr4hip_convert_params_default": (_i, [_vp, _i, _i]),
    "gr4hip_convert_params_check": (_i, [_vp]),
    "gr4hip_convert_create": (_i, [_pvp, _vp]),
    "gr4hip_convert_destroy": (_i, [_vp]),
    "gr4hip_convert_set_scale": (_i, [_vp, _d]),
    "gr4hip_convert_reset": (_i, [_vp]),
    "gr4hip_convert_ports": (_i, [_vp, _psz, _psz, _psz, _psz]),
    "gr4hip_convert_process": (_i, [_vp, _pvp, _pvp, _sz, _psz, _vp]),
    "gr4hip_convert_set_prologue": (_i, [_vp, _vp]),
    "gr4hip_convert_set_epilogue": (_i, [_vp, _vp]),
    "gr4hip_convert_tile": (_sz, [_vp]),
    "gr4hip_savgol_design": (_i, [_i, _sz, _sz, _sz, _d, _i, _vp, _vp]),
    "gr4hip_savgol_pinv_row": (_i, [_i, _sz, _sz, _sz, _i, _vp, _vp]),
    "gr4hip_savgol_zp_tile": (_sz, []),
    "gr4hip_savgol_zp_create": (_i, [_pvp, _vp]),
    "gr4hip_savgol_zp_set_params": (_i, [_vp, _vp]),
    "gr4hip_savgol_zp_coeffs": (_i, [_vp, _vp, _vp]),
    "gr4hip_savgol_zp_process": (_i, [_vp, _vp, _vp, _sz, _sz, _sz, _vp]),
    "gr4hip_savgol_zp_destroy": (_i, [_vp]),
}

class FilterParams(C.Structure):
    _fields_ = [("order", C.c_size_t), ("f_low", _d), ("f_high", _d), ("gain", _d), ("ripple_db", _d), ("attenuation_db", _d),
                ("beta", _d), ("fs", _d)]


FREQEST_TIME_DOMAIN, FREQEST_FREQUENCY_DOMAIN = range(2)


class FreqEstParams(C.Structure):
    """gr4hip_freqest_params: the settings of FrequencyEstimatorTimeDomain / ...FrequencyDomain (FrequencyEstimator.hpp:46-51, 202-207) plus the chunk"""
    _fields_ = [("sample_rate", _f), ("f_min", _f), ("f_expected", _f), ("f_max", _f), ("epsilon", _f),
                ("n_periods", C.c_size_t), ("min_fft_size", C.c_size_t), ("chunk", C.c_size_t)]


class IQDemodParams(C.Structure):
    """gr4hip_iqdemod_params: the settings of IQDemodulator<T> (FrequencyEstimator.hpp:423-429) plus the chunk"""
    _fields_ = [("sample_rate", _f), ("f_high_pass", _f), ("f_low_pass", _f), ("phase_unit", _i), ("invert_phase", _i), ("derivative_method", _i),
                ("epsilon", _d), ("chunk", C.c_size_t)]


class PowerMetricsParams(C.Structure):
    """gr4hip_powermetrics_params: the settings of PowerMetrics<float, nPhases> (PowerEstimators.hpp:46-49) plus the number of phases"""
    _fields_ = [("sample_rate", _f), ("high_pass", _f), ("low_pass", _f), ("decimate", C.c_size_t), ("n_phases", C.c_size_t)]


SCHMITT_NO_INTERPOLATION, SCHMITT_BASIC_LINEAR_INTERPOLATION, SCHMITT_LINEAR_INTERPOLATION, SCHMITT_POLYNOMIAL_INTERPOLATION = range(4)
SCHMITT_RISING, SCHMITT_FALLING, SCHMITT_KIND_MASK, SCHMITT_DEGENERATE = 1, 2, 3, 4
SCHMITT_EDGE_BYTES = 24  # gr4hip_schmitt_edge: {int64 sample, int32 edge_idx, float edge_offset, uint32 kind_flags, uint32 n_fit}


class SchmittParams(C.Structure):
    """gr4hip_schmitt_params: offset and threshold of gr::trigger::SchmittTrigger (SchmittTrigger.hpp:45-46), its interpolation method and the sample type"""
    _fields_ = [("offset", _d), ("threshold", _d), ("method", _i), ("dtype", _i)]


SVDDENOISE_MAX_WINDOW, SVDDENOISE_MAX_WINDOW_COMPLEX = 128, 64


class SvdDenoiseParams(C.Structure):
    """gr4hip_svddenoise_params: the sample type and the seven settings of gr::filter::SvdDenoiser<T> (SvdDenoiser.hpp:37-51)"""
    _fields_ = [("dtype", _i), ("window_size", C.c_size_t), ("hankel_rows", C.c_size_t), ("max_rank", C.c_uint64), ("relative_threshold", _d),
                ("absolute_threshold", _d), ("energy_fraction", _d), ("hop_fraction", _d)]


SIGGEN_TYPES = ["Const", "Sin", "Cos", "Square", "Saw", "Triangle", "FastSin", "FastCos", "UniformNoise", "TriangularNoise", "GaussianNoise"]


class SigGenParams(C.Structure):
    """gr4hip_siggen_params: the sample type and the settings of gr::basic::SignalGenerator<T> (SignalGenerator.hpp:40-47)"""
    _fields_ = [("dtype", _i), ("signal_type", _i), ("sample_rate", _f), ("frequency", _f), ("amplitude", _f), ("offset", _f), ("phase", _f),
                ("seed", C.c_ulonglong)]


CONVERT_KINDS = ["Convert", "ScalingConvert", "Abs", "Real", "Imag", "Arg", "RadiansToDegree", "DegreeToRadians", "ToRealImag", "RealImagToComplex", "ToMagPhase",
                 "MagPhaseToComplex", "ComplexToInterleaved", "InterleavedToComplex"]  # gr4hip_convert_kind, under the reference's block names


class ConvertParams(C.Structure):
    """gr4hip_convert_params: which of the fourteen converter blocks (ConverterBlocks.hpp), its port types and ScalingConvert's scale"""
    _fields_ = [("kind", _i), ("in_dtype", _i), ("out_dtype", _i), ("scale", _d)]


SAVGOL_CENTRED, SAVGOL_CAUSAL = range(2)
SAVGOL_REFLECT, SAVGOL_REPLICATE = range(2)
SAVGOL_ZP_MAX_WINDOW = 255


class SavgolInfo(C.Structure):
    """gr4hip_savgol_info: the clamped settings of a Savitzky-Golay design, the kept rank of its truncated pseudo-inverse and the singular values that decided it"""
    _fields_ = [("window_size", C.c_size_t), ("poly_order", C.c_size_t), ("deriv_order", C.c_size_t), ("rank", C.c_size_t), ("sigma_max", _d),
                ("sigma_min_kept", _d), ("threshold", _d), ("ambiguous", _i)]


class SavgolZpParams(C.Structure):
    """gr4hip_savgol_zp_params: the sample type and the settings of gr::filter::SavitzkyGolayDataSetFilter<T> (SavitzkyGolayFilter.hpp:111-114)"""
    _fields_ = [("dtype", _i), ("window_size", C.c_size_t), ("poly_order", C.c_size_t), ("deriv_order", C.c_size_t), ("boundary_policy", _i)]


LOWPASS, HIGHPASS, BANDPASS, BANDSTOP = range(4)
BUTTERWORTH, BESSEL, CHEBYSHEV1, CHEBYSHEV2 = range(4)

_lib = None


def lib():
    """Load libgr4hip.so (once).  torch is imported first so that its bundled HIP runtime (same SONAME
    libamdhip64.so.7) is the one instance both share -- device pointers and streams are then interchangeable."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the HIP kernel library is required; there is no CPU fallback)")
        import torch  # noqa: F401  (must precede the CDLL load, see docstring)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here == header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if L.gr4hip_abi_version() != 1:
            raise ImportError("libgr4hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc: int, where: str) -> int:
    if rc < 0 and rc not in (DONE, INSUFFICIENT_INPUT, INSUFFICIENT_OUTPUT):
        raise Gr4HipError(rc, where, lib().gr4hip_last_error().decode(errors="replace"))
    return rc


def device_count() -> int:
    n = C.c_int(0)
    check(lib().gr4hip_device_count(C.byref(n)), "device_count")
    return n.value


def developer_switch(name: str, value: int = 1) -> None:
    """kernel A/B switches of the library (include/gr4hip.h: gr4hip_developer_switch); the tests use it where they compare two kernels"""
    check(lib().gr4hip_developer_switch(name.encode(), int(value)), "developer_switch")
