"""Host-side (Python) mirror of the reference's block interface for the hot path, on top of include/gr4hip.h.

Names, settings and error behaviour follow the reference blocks (citations relative to /root/reference):
  fir_filter / iir_filter / BasicFilter / BasicDecimatingFilter / Decimator  blocks/filter/.../time_domain_filter.hpp
  FFT                                                                         blocks/fourier/.../fft.hpp
  math_const / math_nary (AddConst..Divide)                                   blocks/math/.../Math.hpp
  Rotator                                                                     blocks/math/.../Rotator.hpp
  FrequencyEstimatorTimeDomain / FrequencyEstimatorFrequencyDomain            blocks/filter/.../FrequencyEstimator.hpp
  IQDemodulator                                                               blocks/filter/.../FrequencyEstimator.hpp
  PowerMetrics / PowerFactor / SystemUnbalance                                blocks/electrical/.../PowerEstimators.hpp
  Chain                                                                       the runtime fusion of fir_filter -> FFT -> mag2
                                                                              (Merge<> analogue, core/.../BlockMerging.hpp:136-320)
Blocks consume and produce torch tensors that live on the GPU (`process_bulk(x) -> y`); torch only provides the
device memory and the current HIP stream.  Every block is device-only: without libgr4hip.so or without a GPU the
constructor / call raises (Gr4HipError / ImportError) -- there is no CPU fallback in this package.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import capi
from .capi import check, lib

_TORCH_DTYPE = {
    capi.U8: torch.uint8, capi.U16: torch.uint16, capi.U32: torch.uint32, capi.U64: torch.uint64,
    capi.I8: torch.int8, capi.I16: torch.int16, capi.I32: torch.int32, capi.I64: torch.int64,
    capi.F32: torch.float32, capi.F64: torch.float64, capi.C32: torch.complex64, capi.C64: torch.complex128,
}
_DTYPE_ID = {v: k for k, v in _TORCH_DTYPE.items()}
_NP_DTYPE = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64,
             np.float32, np.float64, np.complex64, np.complex128]
_OPS = {"Add": capi.ADD, "Subtract": capi.SUB, "Multiply": capi.MUL, "Divide": capi.DIV,
        "+": capi.ADD, "-": capi.SUB, "*": capi.MUL, "/": capi.DIV}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(x: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, "input must be a CUDA/HIP torch tensor (device-only path)")
    return x.resolve_conj().contiguous()  # materialise lazy conj views: the kernels read raw memory


def _out(out: Optional[torch.Tensor], numel: int, dtype, x: torch.Tensor, what: str, shape=None) -> torch.Tensor:
    """the tensor a kernel writes: allocated here, or the caller's -- which must be a contiguous device tensor of the result's dtype with room for it (the kernels
    write raw memory: an undersized or host tensor would be an out-of-bounds device write)"""
    if out is None:
        return torch.empty(shape if shape is not None else numel, dtype=dtype, device=x.device)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != x.device or not out.is_contiguous() or out.dtype != dtype or out.numel() < numel:
        raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"out must be a contiguous tensor on the input's device, dtype {dtype}, at least {numel} elements")
    return out


def _window_id(window) -> int:
    if isinstance(window, str):
        names = [w.lower() for w in capi.WINDOWS]
        if window.lower() not in names:
            raise ValueError(f"unknown window '{window}'")
        return names.index(window.lower())
    return int(window)


class _Handle:
    _destroy = None

    def __init__(self):
        self._h = C.c_void_p()

    def close(self):
        if getattr(self, "_h", None) and self._h.value and self._destroy:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class fir_filter(_Handle):
    """gr::filter::fir_filter<T> (time_domain_filter.hpp:22-48): settings `b`; T in {float32, complex64} and the second registered type float64
    (double taps, the plain FP64 kernel of csrc/f64.hip)."""
    _destroy = "gr4hip_fir_destroy"

    def __init__(self, b: Sequence[float], dtype=torch.float32, decimate: int = 1):
        super().__init__()
        self.dtype = dtype
        self.decimate = int(decimate)
        self._f64 = dtype == torch.float64
        if self._f64:
            self._destroy = "gr4hip_fir64_destroy"
            self.b = np.ascontiguousarray(b, np.float64)
            check(lib().gr4hip_fir64_create(C.byref(self._h), self.b.ctypes.data, len(self.b), self.decimate), "fir_filter<float64>")
            return
        self.b = np.ascontiguousarray(b, np.float32)
        check(lib().gr4hip_fir_create(C.byref(self._h), _DTYPE_ID[dtype], self.b.ctypes.data, len(self.b), self.decimate), "fir_filter")

    def settings_changed(self, b: Sequence[float]):  # settingsChanged (:38-42)
        if self._f64:
            self.b = np.ascontiguousarray(b, np.float64)
            check(lib().gr4hip_fir64_set_taps(self._h, self.b.ctypes.data, len(self.b)), "fir_filter.set_taps")
            return
        self.b = np.ascontiguousarray(b, np.float32)
        check(lib().gr4hip_fir_set_taps(self._h, self.b.ctypes.data, len(self.b)), "fir_filter.set_taps")

    def reset(self):
        check((lib().gr4hip_fir64_reset if self._f64 else lib().gr4hip_fir_reset)(self._h), "fir_filter.reset")

    def set_prologue(self, prog: Optional["Merged"]):
        """per-sample blocks in FRONT of the filter, executed in its launch (gr4hip_fir_set_prologue): gains fold into the taps, anything else is a load hook"""
        check(lib().gr4hip_fir_set_prologue(self._h, prog._h if prog is not None else None), "fir_filter.set_prologue")

    def set_epilogue(self, prog: Optional["Merged"]):
        """per-sample blocks BEHIND the filter, executed in its launch (gr4hip_fir_set_epilogue)"""
        check(lib().gr4hip_fir_set_epilogue(self._h, prog._h if prog is not None else None), "fir_filter.set_epilogue")

    def set_algo(self, algo: int):
        """capi.FIR_AUTO / capi.FIR_TIME_DOMAIN (direct form also for long complex spans: error relative to the output) / capi.FIR_EXACT_F32 (IEEE float32
        multiply-add only: the reference's Inf / NaN behaviour) -- include/gr4hip.h"""
        check(lib().gr4hip_fir_set_algo(self._h, int(algo)), "fir_filter.set_algo")

    def set_guard_mode(self, mode: int):
        """capi.GUARD_STRICT (default) / GUARD_DEFERRED / GUARD_OFF: the dynamic-range guard of the frequency-domain kernels, and (OFF) of the f16 direct
        form's per-segment verdict -- gr4hip_fir_set_guard_mode, include/gr4hip.h"""
        check(lib().gr4hip_fir_set_guard_mode(self._h, int(mode)), "fir_filter.set_guard_mode")

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "fir_filter")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "fir_filter", f"expected {self.dtype}, got {x.dtype}")
        n_out = x.numel() // self.decimate
        out = _out(out, n_out, self.dtype, x, "fir_filter.process")
        fn = lib().gr4hip_fir64_process if self._f64 else lib().gr4hip_fir_process
        check(fn(self._h, x.data_ptr(), x.numel(), out.data_ptr(), None, _stream()), "fir_filter.process")
        return out


class fir_interpolator(_Handle):
    """Interpolating FIR (north_star "decimating / interpolating FIR"; the reference only has the rate declaration Resampling<1, L>,
    annotated.hpp:121-128): zero-stuff by `interpolate`, fir_filter's sum at the output rate, gain `interpolate`,
    evaluated as a polyphase bank.  settings `b`, `interpolate`; T in {float32, complex64}; n_out = n_in * interpolate."""
    _destroy = "gr4hip_fir_interp_destroy"

    def __init__(self, b: Sequence[float], interpolate: int, dtype=torch.float32):
        super().__init__()
        self.b = np.ascontiguousarray(b, np.float32)
        self.dtype = dtype
        self.interpolate = int(interpolate)
        check(lib().gr4hip_fir_interp_create(C.byref(self._h), _DTYPE_ID[dtype], self.b.ctypes.data, len(self.b), self.interpolate), "fir_interpolator")

    def settings_changed(self, b: Sequence[float]):
        self.b = np.ascontiguousarray(b, np.float32)
        check(lib().gr4hip_fir_interp_set_taps(self._h, self.b.ctypes.data, len(self.b)), "fir_interpolator.set_taps")

    def reset(self):
        check(lib().gr4hip_fir_interp_reset(self._h), "fir_interpolator.reset")

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "fir_interpolator")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "fir_interpolator", f"expected {self.dtype}, got {x.dtype}")
        out = _out(out, x.numel() * self.interpolate, self.dtype, x, "fir_interpolator.process")
        check(lib().gr4hip_fir_interp_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), None, _stream()), "fir_interpolator.process")
        return out


class rational_resampler(_Handle):
    """Rational resampler, rate `interpolate` / `decimate` (RATIONAL_RESAMPLER.md; the reference has only the rate machinery Resampling<in, out>): zero-stuff by
    L, fir_filter's sum with gain L, keep every M-th sample -- evaluated as L polyphase branches that compute only the kept outputs.  settings `b` (real taps),
    `interpolate`, `decimate`; T in {float32, complex64}; n_in a multiple of `decimate`, n_out = n_in / decimate * interpolate."""
    _destroy = "gr4hip_resamp_destroy"

    def __init__(self, b: Sequence[float], interpolate: int, decimate: int, dtype=torch.float32):
        super().__init__()
        self.b = np.ascontiguousarray(b, np.float32)
        self.dtype = dtype
        self.interpolate, self.decimate = int(interpolate), int(decimate)
        if dtype not in (torch.float32, torch.complex64):
            raise capi.Gr4HipError(capi.UNSUPPORTED, "rational_resampler", f"float32 or complex64 streams, got {dtype}")
        check(lib().gr4hip_resamp_create(C.byref(self._h), _DTYPE_ID[dtype], self.b.ctypes.data, len(self.b), self.interpolate, self.decimate), "rational_resampler")

    def settings_changed(self, b: Sequence[float]):
        """new taps at the same rate; the history is kept unless it must grow"""
        self.b = np.ascontiguousarray(b, np.float32)
        check(lib().gr4hip_resamp_set_taps(self._h, self.b.ctypes.data, len(self.b)), "rational_resampler.set_taps")

    def reset(self):
        check(lib().gr4hip_resamp_reset(self._h), "rational_resampler.reset")

    @staticmethod
    def tile() -> int:
        """output cycles (of `interpolate` samples) per workgroup"""
        return int(lib().gr4hip_resamp_tile())

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "rational_resampler")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "rational_resampler", f"expected {self.dtype}, got {x.dtype}")
        out = _out(out, x.numel() // self.decimate * self.interpolate, self.dtype, x, "rational_resampler.process")
        check(lib().gr4hip_resamp_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), None, _stream()), "rational_resampler.process")
        return out


def design_resampler_taps(interpolate: int, decimate: int, half_len: int = 8, window: str = "Hamming", beta: float = 1.6) -> np.ndarray:
    """the low-pass in front of a rate change by interpolate / decimate: 2 half_len max(L, M) + 1 windowed-sinc taps, cut-off 0.4 / max(L, M) of the L-times rate,
    DC gain 1, float32 (gr4hip_resamp_design: host code, no device)"""
    n = C.c_size_t(0)
    check(lib().gr4hip_resamp_design(None, 0, C.byref(n), int(interpolate), int(decimate), int(half_len), _window_id(window), float(beta)), "design_resampler_taps")
    h = np.empty(n.value, np.float32)
    check(lib().gr4hip_resamp_design(h.ctypes.data, h.size, C.byref(n), int(interpolate), int(decimate), int(half_len), _window_id(window), float(beta)), "design_resampler_taps")
    return h


class complex_fir_filter(_Handle):
    """Complex taps x complex data FIR, direct and decimating (SURVEY.md Appendix A's "complex-tap variant"; the reference's fir_filter takes floating-point
    T only, so the definition is the project's: COMPLEX_FIR.md).  settings `b` (complex), `decimate`; complex64 in, complex64 out, n_out = n_in / decimate."""
    _destroy = "gr4hip_cfir_destroy"

    def __init__(self, b: Sequence[complex], decimate: int = 1):
        super().__init__()
        self.dtype = torch.complex64
        self.decimate = int(decimate)
        self.b = np.ascontiguousarray(b, np.complex64)
        check(lib().gr4hip_cfir_create(C.byref(self._h), self.b.ctypes.data, len(self.b), self.decimate), "complex_fir_filter")

    def settings_changed(self, b: Sequence[complex]):
        self.b = np.ascontiguousarray(b, np.complex64)
        check(lib().gr4hip_cfir_set_taps(self._h, self.b.ctypes.data, len(self.b)), "complex_fir_filter.set_taps")

    def reset(self):
        check(lib().gr4hip_cfir_reset(self._h), "complex_fir_filter.reset")

    def set_guard_mode(self, mode: int):
        """capi.GUARD_STRICT (default) or capi.GUARD_OFF (no marking, no second evaluation) -- gr4hip_cfir_set_guard_mode"""
        check(lib().gr4hip_cfir_set_guard_mode(self._h, int(mode)), "complex_fir_filter.set_guard_mode")

    @staticmethod
    def segment() -> int:
        """complex outputs per guard segment"""
        return int(lib().gr4hip_cfir_segment())

    @staticmethod
    def tile() -> int:
        """complex outputs per tile group of the matrix-pipe kernel"""
        return int(lib().gr4hip_cfir_tile())

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "complex_fir_filter")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "complex_fir_filter", f"expected {self.dtype}, got {x.dtype}")
        out = _out(out, x.numel() // self.decimate, self.dtype, x, "complex_fir_filter.process")
        check(lib().gr4hip_cfir_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), None, _stream()), "complex_fir_filter.process")
        return out


class iir_filter(_Handle):
    """gr::filter::iir_filter<float, form> (time_domain_filter.hpp:62-122) or a cascade of sections
    (gr::filter::Filter<float>, FilterTool.hpp:223-247).  b, a: [nsections][n] or 1-D for a single section."""
    _destroy = "gr4hip_iir_destroy"

    def __init__(self, b, a, form: int = capi.DF_II, dtype=torch.float32):
        super().__init__()
        self.dtype = dtype
        self._f64 = dtype == torch.float64  # iir_filter<double, form> (time_domain_filter.hpp:57-60): csrc/f64.hip
        npt = np.float64 if self._f64 else np.float32
        b = np.atleast_2d(np.asarray(b, npt))
        a = np.atleast_2d(np.asarray(a, npt))
        if b.shape[0] != a.shape[0]:
            raise ValueError("b and a need the same number of sections")
        self.b, self.a, self.form = np.ascontiguousarray(b), np.ascontiguousarray(a), form
        if self._f64:
            self._destroy = "gr4hip_iir64_destroy"
            check(lib().gr4hip_iir64_create(C.byref(self._h), form, b.shape[0], self.b.ctypes.data, b.shape[1], self.a.ctypes.data, a.shape[1]), "iir_filter<float64>")
            return
        check(lib().gr4hip_iir_create(C.byref(self._h), form, b.shape[0], self.b.ctypes.data, b.shape[1], self.a.ctypes.data, a.shape[1]), "iir_filter")

    def reset(self):
        check((lib().gr4hip_iir64_reset if self._f64 else lib().gr4hip_iir_reset)(self._h), "iir_filter.reset")

    def set_algo(self, algo: int):
        """capi.IIR_AUTO (default: the parallel-in-time kernels unless the create-time self-test finds that float32 cannot carry this cascade's state through them),
        capi.IIR_PARALLEL or capi.IIR_SEQUENTIAL_F32 (the reference's arithmetic in the requested form, one lane, sample by sample) -- include/gr4hip.h"""
        if self._f64:
            raise capi.Gr4HipError(capi.UNSUPPORTED, "iir_filter", "the float64 cascade has one evaluation")
        check(lib().gr4hip_iir_set_algo(self._h, int(algo)), "iir_filter.set_algo")

    @property
    def algo_in_use(self):
        """(evaluation in use, create-time error of the parallel kernels, of the sequential float32 form) -- errors as max |error| / output rms, < 0: not measured"""
        a, ep, es = C.c_int(0), C.c_float(0), C.c_float(0)
        check(lib().gr4hip_iir_get_algo(self._h, C.byref(a), C.byref(ep), C.byref(es)), "iir_filter.get_algo")
        return a.value, ep.value, es.value

    def status(self):
        """synchronise the current stream and raise if an earlier launch of this handle reported a look-back time-out (include/gr4hip.h)"""
        if not self._f64:
            check(lib().gr4hip_iir_status(self._h, _stream()), "iir_filter.status")

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "iir_filter")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "iir_filter", f"expected {self.dtype}, got {x.dtype}")
        out = _out(out, x.numel(), x.dtype, x, "iir_filter.process")
        fn = lib().gr4hip_iir64_process if self._f64 else lib().gr4hip_iir_process
        check(fn(self._h, x.data_ptr(), x.numel(), out.data_ptr(), _stream()), "iir_filter.process")
        return out


def fir_iir_process(fir: "fir_filter", iir: "iir_filter", x: torch.Tensor, out: Optional[torch.Tensor] = None, mode: int = 0) -> torch.Tensor:
    """BasicDecimatingFilter (FIR) -> IIR cascade in one call (gr4hip_fir_iir_process, BASELINE configs[2]).  mode capi.FIR_IIR_ONE_LAUNCH: the cascade as the
    frequency-domain decimator's store epilogue where both qualify -- one launch, no decimated stream in HBM; FIR_IIR_TWO_LAUNCHES; FIR_IIR_AUTO (0): the faster one
    as measured (two launches).  Both handles keep their own state"""
    x = _dev(x, "fir_iir_process")
    if x.dtype != torch.float32 or fir.dtype != torch.float32 or iir.dtype != torch.float32:
        raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "fir_iir_process", "float32 stream, filter and cascade")
    n_out = x.numel() // fir.decimate
    out = _out(out, n_out, torch.float32, x, "fir_iir_process")
    check(lib().gr4hip_fir_iir_process(fir._h, iir._h, x.data_ptr(), x.numel(), out.data_ptr(), None, int(mode), _stream()), "fir_iir_process")
    return out


def design_fir(filter_response: int, order: int, f_low: float, f_high: float, sample_rate: float, window="Kaiser", gain=1.0,
               attenuation_db=40.0, beta=1.6) -> np.ndarray:
    """fir::designFilter<float> (FilterTool.hpp:1006-1071) through the library's host-side restatement."""
    p = capi.FilterParams()
    lib().gr4hip_filter_params_default(C.byref(p))
    p.order, p.f_low, p.f_high, p.fs, p.gain, p.attenuation_db, p.beta = order, f_low, f_high, sample_rate, gain, attenuation_db, beta
    n = C.c_size_t(0)
    check(lib().gr4hip_fir_design(filter_response, C.byref(p), _window_id(window), None, 0, C.byref(n)), "fir_design")
    taps = np.empty(n.value, np.float32)
    check(lib().gr4hip_fir_design(filter_response, C.byref(p), _window_id(window), taps.ctypes.data, len(taps), C.byref(n)), "fir_design")
    return taps


def design_iir(filter_response: int, order: int, f_low: float, f_high: float, sample_rate: float, design: int = capi.BUTTERWORTH,
               gain=1.0, ripple_db=0.1, attenuation_db=40.0):
    """iir::designFilter<float> (FilterTool.hpp:848-917): biquad sections (b[ns][3], a[ns][3])."""
    p = capi.FilterParams()
    lib().gr4hip_filter_params_default(C.byref(p))
    p.order, p.f_low, p.f_high, p.fs, p.gain, p.ripple_db, p.attenuation_db = order, f_low, f_high, sample_rate, gain, ripple_db, attenuation_db
    b = np.zeros((32, 3), np.float32)
    a = np.zeros((32, 3), np.float32)
    ns = C.c_size_t(0)
    check(lib().gr4hip_iir_design(filter_response, C.byref(p), design, b.ctypes.data, a.ctypes.data, 32, C.byref(ns)), "iir_design")
    return b[:ns.value].copy(), a[:ns.value].copy()


class BasicFilter:
    """gr::filter::BasicFilterProto<float, Args...> (time_domain_filter.hpp:129-205), defaults :148-157."""

    def __init__(self, filter_type="IIR", filter_response=capi.LOWPASS, filter_order=3, f_low=0.1, f_high=0.2, sample_rate=1.0,
                 decimate=1, iir_design_method=capi.BUTTERWORTH, fir_design_method="Kaiser"):
        self.filter_type, self.filter_response, self.filter_order = filter_type, filter_response, filter_order
        self.f_low, self.f_high, self.sample_rate, self.decimate = f_low, f_high, sample_rate, int(decimate)
        self.iir_design_method, self.fir_design_method = iir_design_method, fir_design_method
        self.input_chunk_size = 1
        self._fir = self._iir = None
        self.design_filter()

    def design_filter(self):  # designFilter() :163-182
        self.input_chunk_size = self.decimate
        if self.filter_type == "FIR":
            self.taps = design_fir(self.filter_response, self.filter_order, self.f_low, self.f_high, self.sample_rate, self.fir_design_method)
            self._fir, self._iir = fir_filter(self.taps, torch.float32, self.decimate), None
        elif self.filter_type == "IIR":
            self.sections = design_iir(self.filter_response, self.filter_order, self.f_low, self.f_high, self.sample_rate, self.iir_design_method)
            self._iir, self._fir = iir_filter(*self.sections), None
        else:
            raise ValueError("filter_type must be 'FIR' or 'IIR'")

    def process_bulk(self, x: torch.Tensor) -> torch.Tensor:  # :184-204
        if self._fir is not None:
            return self._fir.process_bulk(x)
        y = self._iir.process_bulk(x)
        return Decimator(self.decimate).process_bulk(y) if self.decimate > 1 else y


BasicDecimatingFilter = BasicFilter  # BasicFilterProto<T, Resampling<1,1,false>> (:210-211): same class, decimate > 1


class Decimator:
    """gr::filter::Decimator<T> (time_domain_filter.hpp:215-245): keep every decim-th sample."""

    def __init__(self, decim: int = 1):
        self.decim = int(decim)
        self.input_chunk_size = self.decim

    def process_bulk(self, x: torch.Tensor) -> torch.Tensor:
        x = _dev(x, "Decimator")
        n_out = (x.numel() + self.decim - 1) // self.decim
        out = torch.empty(n_out, dtype=x.dtype, device=x.device)
        check(lib().gr4hip_decimate(_DTYPE_ID[x.dtype], x.data_ptr(), x.numel(), self.decim, out.data_ptr(), None, _stream()), "Decimator")
        return out


class FFT(_Handle):
    """gr::blocks::fft::FFT<T> (blocks/fourier/.../fft.hpp:31-251): settings fftSize, window, outputInDb, outputInDeg,
    unwrapPhase.  process_bulk returns a dict per call with the DataSet signals for all frames:
    magnitude / phase / re / im tensors [frames, n] plus `ranges` [frames, 4, 2] (fft.hpp:173-250)."""
    _destroy = "gr4hip_fft_destroy"

    def __init__(self, fftSize: int = 1024, window="Hann", outputInDb=False, outputInDeg=False, unwrapPhase=False, dtype=torch.complex64,
                 sample_rate: float = 1.0):
        super().__init__()
        self.fftSize, self.window, self.dtype, self.sample_rate = int(fftSize), window, dtype, sample_rate
        self.outputInDb, self.outputInDeg, self.unwrapPhase = outputInDb, outputInDeg, unwrapPhase
        flags = (capi.FFT_OUTPUT_IN_DB if outputInDb else 0) | (capi.FFT_OUTPUT_IN_DEG if outputInDeg else 0) | (capi.FFT_UNWRAP_PHASE if unwrapPhase else 0)
        self._f64 = dtype == torch.float64  # FFT<double> (fourier/fft.hpp:29): real double frames, outputs in double (csrc/f64.hip)
        self.input_chunk_size = self.fftSize  # fft.hpp:131-134
        self.n_out = self.fftSize if dtype == torch.complex64 else self.fftSize // 2
        if self._f64:
            self._destroy = "gr4hip_fft64_destroy"
            check(lib().gr4hip_fft64_create(C.byref(self._h), self.fftSize, _window_id(window), flags), "FFT<float64>")
            return
        check(lib().gr4hip_fft_create(C.byref(self._h), _DTYPE_ID[dtype], self.fftSize, _window_id(window), flags), "FFT")

    def _frames(self, x):
        x = _dev(x, "FFT")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "FFT", f"expected {self.dtype}, got {x.dtype}")
        return x, x.numel() // self.fftSize

    def process_bulk(self, x: torch.Tensor, ranges: bool = True) -> dict:
        x, frames = self._frames(x)
        if self._f64:
            mk64 = lambda: torch.empty((frames, self.n_out), dtype=torch.float64, device=x.device)
            out = {"magnitude": mk64(), "phase": mk64(), "re": mk64(), "im": mk64()}
            check(lib().gr4hip_fft64_process(self._h, x.data_ptr(), frames, out["magnitude"].data_ptr(), out["phase"].data_ptr(), out["re"].data_ptr(), out["im"].data_ptr(),
                                             _stream()), "FFT.process")
            if ranges:  # fft.hpp:229-232: min / max of the four signals per frame (host-side glue for the float64 corner)
                out["ranges"] = torch.stack([torch.stack([out[k].amin(dim=1), out[k].amax(dim=1)], dim=1) for k in ("magnitude", "phase", "re", "im")], dim=1)
            out["frequency"] = np.arange(self.n_out) * (self.sample_rate / self.fftSize)  # frequency axis (fft.hpp:187-193), as for float32 real input
            return out
        mk = lambda: torch.empty((frames, self.n_out), dtype=torch.float32, device=x.device)
        out = {"magnitude": mk(), "phase": mk(), "re": mk(), "im": mk()}
        rg = torch.empty((frames, 4, 2), dtype=torch.float32, device=x.device) if ranges else None
        check(lib().gr4hip_fft_process(self._h, x.data_ptr(), frames, out["magnitude"].data_ptr(), out["phase"].data_ptr(), out["re"].data_ptr(),
                                       out["im"].data_ptr(), rg.data_ptr() if ranges else None, _stream()), "FFT.process")
        if ranges:
            out["ranges"] = rg
        n = self.n_out
        fw = self.sample_rate / self.fftSize  # frequency axis (fft.hpp:187-193)
        out["frequency"] = (np.arange(n) * fw - (n // 2) * fw) if self.dtype == torch.complex64 else np.arange(n) * fw
        return out

    def spectrum(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x, frames = self._frames(x)
        out = _out(out, frames * self.fftSize, torch.complex64, x, "FFT.spectrum", (frames, self.fftSize))
        check(lib().gr4hip_fft_spectrum(self._h, x.data_ptr(), frames, out.data_ptr(), _stream()), "FFT.spectrum")
        return out

    def set_epilogue(self, prog: Optional["Merged"]):
        """float blocks BEHIND the power spectrum (normalisation, an offset) in the transform's launch: applied to every |X|^2 of mag2() (gr4hip_fft_set_epilogue)"""
        check(lib().gr4hip_fft_set_epilogue(self._h, prog._h if prog is not None else None), "FFT.set_epilogue")

    def mag2(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x, frames = self._frames(x)
        out = _out(out, frames * self.fftSize, torch.float32, x, "FFT.mag2", (frames, self.fftSize))
        check(lib().gr4hip_fft_mag2(self._h, x.data_ptr(), frames, out.data_ptr(), _stream()), "FFT.mag2")
        return out

    def power_integrated(self, x: torch.Tensor, integrator: "SpectrumIntegrator", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mag2() followed by integrator.process_bulk(), bit for bit, in the transform's launch where it has a sink (gr4hip_fft_mag2_integrate)"""
        x, frames = self._frames(x)
        return integrator._run(lib().gr4hip_fft_mag2_integrate, self._h, x, frames, out, "FFT.power_integrated")


class STFT(_Handle):
    """The FFT block with the reference's `stride` setting (Block.hpp:711), stated for a stream (OVERLAPPED_FFT.md): frame m covers the samples
    [m stride, m stride + fftSize) and leaves once its last sample has arrived -- stride < fftSize overlaps frames (spectrograms, Welch averaging), stride > fftSize
    skips samples, 0 means fftSize.  The last fftSize - 1 samples are carried across calls, so the values do not depend on how a stream is cut; every frame's outputs
    are those of FFT(fftSize, window, ...) on that frame."""
    _destroy = "gr4hip_stft_destroy"

    def __init__(self, fftSize: int = 1024, stride: int = 0, window="Hann", outputInDb=False, outputInDeg=False, unwrapPhase=False, dtype=torch.complex64,
                 sample_rate: float = 1.0):
        super().__init__()
        if dtype not in (torch.complex64, torch.float32):
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "STFT", f"complex64 or float32 frames (got {dtype})")
        self.fftSize, self.stride, self.window, self.dtype, self.sample_rate = int(fftSize), int(stride) or int(fftSize), window, dtype, sample_rate
        self.outputInDb, self.outputInDeg, self.unwrapPhase = outputInDb, outputInDeg, unwrapPhase
        flags = (capi.FFT_OUTPUT_IN_DB if outputInDb else 0) | (capi.FFT_OUTPUT_IN_DEG if outputInDeg else 0) | (capi.FFT_UNWRAP_PHASE if unwrapPhase else 0)
        self.n_out = self.fftSize if dtype == torch.complex64 else self.fftSize // 2
        self._frames_out = 0  # frames emitted since create / reset: the index of the next one
        check(lib().gr4hip_stft_create(C.byref(self._h), _DTYPE_ID[dtype], self.fftSize, self.stride, _window_id(window), flags), "STFT")

    def reset(self):
        """the next sample starts a new stream"""
        check(lib().gr4hip_stft_reset(self._h), "STFT.reset")
        self._frames_out = 0

    def pending(self, n: int) -> int:
        """frames the next call of n samples emits (host only)"""
        k = C.c_size_t(0)
        check(lib().gr4hip_stft_pending(self._h, int(n), C.byref(k)), "STFT.pending")
        return int(k.value)

    def _in(self, x):
        x = _dev(x, "STFT").reshape(-1)
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "STFT", f"expected {self.dtype}, got {x.dtype}")
        return x, self.pending(x.numel())

    def _done(self, got, k, what="STFT"):
        if got.value != k:
            raise capi.Gr4HipError(capi.RUNTIME_ERROR, what, f"the call emitted {got.value} frames, pending() said {k}")
        self._frames_out += k

    def process_bulk(self, x: torch.Tensor, ranges: bool = True) -> dict:
        """FFT.process_bulk's dict for the frames this call completes, plus `time`: their start times"""
        x, k = self._in(x)
        rows = max(k, 1)  # (a call too short for a frame still names its outputs: the library refuses a call whose outputs are all null)
        mk = lambda: torch.empty((rows, self.n_out), dtype=torch.float32, device=x.device)
        full = {"magnitude": mk(), "phase": mk(), "re": mk(), "im": mk()}
        rg = torch.empty((rows, 4, 2), dtype=torch.float32, device=x.device) if ranges else None
        got = C.c_size_t(0)
        first = self._frames_out
        check(lib().gr4hip_stft_process(self._h, x.data_ptr(), x.numel(), full["magnitude"].data_ptr(), full["phase"].data_ptr(), full["re"].data_ptr(),
                                        full["im"].data_ptr(), rg.data_ptr() if ranges else None, C.byref(got), _stream()), "STFT.process")
        self._done(got, k, "STFT.process")
        out = {key: v[:k] for key, v in full.items()}
        if ranges:
            out["ranges"] = rg[:k]
        n = self.n_out
        fw = self.sample_rate / self.fftSize
        out["frequency"] = (np.arange(n) * fw - (n // 2) * fw) if self.dtype == torch.complex64 else np.arange(n) * fw
        out["time"] = (first + np.arange(k)) * (self.stride / self.sample_rate)
        return out

    def _one(self, entry, x, out, dtype, what):
        x, k = self._in(x)
        out = _out(out, max(k, 1) * self.fftSize, dtype, x, what, (max(k, 1), self.fftSize))  # (never a null output: see process_bulk)
        got = C.c_size_t(0)
        check(entry(self._h, x.data_ptr(), x.numel(), out.data_ptr(), C.byref(got), _stream()), what)
        self._done(got, k, what)
        return out.reshape(-1)[:k * self.fftSize].view(k, self.fftSize)

    def spectrum(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """complex64 [frames, fftSize], natural bin order"""
        return self._one(lib().gr4hip_stft_spectrum, x, out, torch.complex64, "STFT.spectrum")

    def mag2(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """|X|^2, float32 [frames, fftSize]"""
        return self._one(lib().gr4hip_stft_mag2, x, out, torch.float32, "STFT.mag2")

    def power_integrated(self, x: torch.Tensor, integrator: "SpectrumIntegrator", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Welch: mag2() followed by integrator.process_bulk(), bit for bit, without the frames' |X|^2 in the caller's memory (gr4hip_stft_mag2_integrate)"""
        x, k = self._in(x)
        n = integrator.pending(k)
        out = _out(out, n * self.fftSize, torch.float32, x, "STFT.power_integrated", (n, self.fftSize))
        got = C.c_size_t(0)
        check(lib().gr4hip_stft_mag2_integrate(self._h, integrator._h, x.data_ptr(), x.numel(), out.data_ptr() if n else None, C.byref(got), _stream()),
              "STFT.power_integrated")
        if got.value != n:
            raise capi.Gr4HipError(capi.RUNTIME_ERROR, "STFT.power_integrated", f"the call completed {got.value} spectra, pending() said {n}")
        self._frames_out += k
        return out.reshape(-1)[:n * self.fftSize].view(n, self.fftSize)


def design_pfb(n_channels: int, taps_per_channel: int, window="Hamming", beta: float = 1.6) -> np.ndarray:
    """the bank's windowed-sinc prototype h[j] = w[j] sinc((j - (P N - 1) / 2) / N), float32 [P N] (gr4hip_pfb_design: host code, no device)"""
    h = np.empty(int(n_channels) * int(taps_per_channel), np.float32)
    check(lib().gr4hip_pfb_design(h.ctypes.data, int(n_channels), int(taps_per_channel), _window_id(window), float(beta)), "design_pfb")
    return h


class PolyphaseFilterBank(_Handle):
    """Critically sampled polyphase analysis bank in front of the FFT block's transform (PFB spectrometer / channelizer; the project's own definition, PFB.md):
    frame m = FFT_N(sum_k h[k N + i] x[(m - P + 1 + k) N + i]).  complex64 in, N samples per frame in and out, the last (P - 1) N samples carried across calls.
    `taps` = P N float values (None: design_pfb with `window`)."""
    _destroy = "gr4hip_pfb_destroy"

    def __init__(self, n_channels: int, taps_per_channel: int, taps=None, window="Hamming"):
        super().__init__()
        self.n_channels, self.taps_per_channel, self.dtype = int(n_channels), int(taps_per_channel), torch.complex64
        self.taps = None
        if taps is not None:
            self.taps = np.ascontiguousarray(taps, np.float32)
            if self.taps.size != self.n_channels * self.taps_per_channel:
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PolyphaseFilterBank", f"{self.taps.size} taps, the bank has {self.taps_per_channel} x {self.n_channels}")
        elif _window_id(window) != _window_id("Hamming"):  # (Hamming is the library's own default design)
            self.taps = design_pfb(self.n_channels, self.taps_per_channel, window)
        check(lib().gr4hip_pfb_create(C.byref(self._h), capi.C32, self.n_channels, self.taps_per_channel, self.taps.ctypes.data if self.taps is not None else None, 0),
              "PolyphaseFilterBank")

    def set_taps(self, taps):
        """new prototype from the next call on; the history is kept"""
        self.taps = np.ascontiguousarray(taps, np.float32)
        check(lib().gr4hip_pfb_set_taps(self._h, self.taps.ctypes.data, self.taps.size), "PolyphaseFilterBank.set_taps")

    def reset(self):
        check(lib().gr4hip_pfb_reset(self._h), "PolyphaseFilterBank.reset")

    def _run(self, x, out, dtype, power: bool):
        x = _dev(x, "PolyphaseFilterBank")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PolyphaseFilterBank", f"expected {self.dtype}, got {x.dtype}")
        if x.numel() % self.n_channels:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PolyphaseFilterBank", f"{x.numel()} samples are not whole frames of {self.n_channels}")
        frames = x.numel() // self.n_channels
        out = _out(out, frames * self.n_channels, dtype, x, "PolyphaseFilterBank", (frames, self.n_channels))
        check(lib().gr4hip_pfb_process(self._h, x.data_ptr(), frames, None if power else out.data_ptr(), out.data_ptr() if power else None, _stream()),
              "PolyphaseFilterBank.process")
        return out

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the channelizer: complex64 [frames, N], bin c of frame m"""
        return self._run(x, out, torch.complex64, False)

    def power(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the spectrometer: |X|^2, float32 [frames, N]"""
        return self._run(x, out, torch.float32, True)

    def power_integrated(self, x: torch.Tensor, integrator: "SpectrumIntegrator", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """power() followed by integrator.process_bulk(), bit for bit, in the transform's launch where it has a sink (gr4hip_pfb_power_integrate)"""
        x = _dev(x, "PolyphaseFilterBank")
        if x.dtype != self.dtype or x.numel() % self.n_channels:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PolyphaseFilterBank", f"expected whole frames of {self.n_channels} {self.dtype} samples")
        return integrator._run(lib().gr4hip_pfb_power_integrate, self._h, x, x.numel() // self.n_channels, out, "PolyphaseFilterBank.power_integrated")


class InverseFFT(_Handle):
    """The unnormalised inverse of the FFT block's transform (algorithm::FFT's Direction::Backward, algorithm/.../fourier/fft.hpp:260-314; INVERSE_FFT.md):
    frames of fftSize complex64 bins in natural order -> [frames, fftSize] complex64, or float32 (the packed complex-to-real form: bins 0 .. N/2 are used, the
    rest is ignored).  scale=True multiplies by 1 / fftSize; `window` is a synthesis window multiplied onto the samples."""
    _destroy = "gr4hip_ifft_destroy"

    def __init__(self, fftSize: int = 1024, dtype=torch.complex64, window="None", scale: bool = False):
        super().__init__()
        if dtype not in (torch.complex64, torch.float32):
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "InverseFFT", f"output dtype must be complex64 or float32, got {dtype}")
        self.fftSize, self.dtype, self.window, self.scale = int(fftSize), dtype, window, bool(scale)
        self.input_chunk_size = self.fftSize
        check(lib().gr4hip_ifft_create(C.byref(self._h), _DTYPE_ID[dtype], self.fftSize, _window_id(window), capi.IFFT_SCALE if self.scale else 0), "InverseFFT")

    def process_bulk(self, spectra: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(spectra, "InverseFFT")
        if x.dtype != torch.complex64:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "InverseFFT", f"expected {torch.complex64}, got {x.dtype}")
        if x.numel() % self.fftSize:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "InverseFFT", f"{x.numel()} bins are not whole frames of {self.fftSize}")
        frames = x.numel() // self.fftSize
        out = _out(out, frames * self.fftSize, self.dtype, x, "InverseFFT", (frames, self.fftSize))
        check(lib().gr4hip_ifft_process(self._h, x.data_ptr(), frames, out.data_ptr(), _stream()), "InverseFFT.process")
        return out


class PolyphaseSynthesisBank(_Handle):
    """Critically sampled polyphase synthesis bank behind the inverse transform (the project's own definition, INVERSE_FFT.md): v_m = IFFT_N(Y_m),
    y[m N + i] = sum_k g[k N + i] v_{m - k}[i].  complex64 in and out, N values per frame in, N samples out, the last P - 1 transformed frames carried across
    calls.  `taps` = P N float values (None: design_pfb with `window`).  With the analysis bank's prototype it is that bank's adjoint, not its inverse."""
    _destroy = "gr4hip_pfb_synth_destroy"

    def __init__(self, n_channels: int, taps_per_channel: int, taps=None, window="Hamming", scale: bool = False):
        super().__init__()
        self.n_channels, self.taps_per_channel, self.dtype, self.scale = int(n_channels), int(taps_per_channel), torch.complex64, bool(scale)
        self.taps = None
        if taps is not None:
            self.taps = np.ascontiguousarray(taps, np.float32)
            if self.taps.size != self.n_channels * self.taps_per_channel:
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PolyphaseSynthesisBank", f"{self.taps.size} taps, the bank has {self.taps_per_channel} x {self.n_channels}")
        elif _window_id(window) != _window_id("Hamming"):  # (Hamming is the library's own default design)
            self.taps = design_pfb(self.n_channels, self.taps_per_channel, window)
        check(lib().gr4hip_pfb_synth_create(C.byref(self._h), self.n_channels, self.taps_per_channel, self.taps.ctypes.data if self.taps is not None else None,
                                            capi.IFFT_SCALE if self.scale else 0), "PolyphaseSynthesisBank")

    def set_taps(self, taps):
        """new prototype from the next call on; the history is kept"""
        self.taps = np.ascontiguousarray(taps, np.float32)
        check(lib().gr4hip_pfb_synth_set_taps(self._h, self.taps.ctypes.data, self.taps.size), "PolyphaseSynthesisBank.set_taps")

    def reset(self):
        check(lib().gr4hip_pfb_synth_reset(self._h), "PolyphaseSynthesisBank.reset")

    def process_bulk(self, spectra: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(spectra, "PolyphaseSynthesisBank")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PolyphaseSynthesisBank", f"expected {self.dtype}, got {x.dtype}")
        if x.numel() % self.n_channels:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PolyphaseSynthesisBank", f"{x.numel()} values are not whole frames of {self.n_channels}")
        frames = x.numel() // self.n_channels
        out = _out(out, frames * self.n_channels, torch.complex64, x, "PolyphaseSynthesisBank", (frames, self.n_channels))
        check(lib().gr4hip_pfb_synth_process(self._h, x.data_ptr(), frames, out.data_ptr(), _stream()), "PolyphaseSynthesisBank.process")
        return out


class _Integrating(_Handle):
    """what the handles that carry a partial integration across calls share: gr4hip_<_prefix>_reset / _set_length / _pending, reported as <_name>.<call>"""
    _prefix = _name = None

    def _call(self, call, *args):
        check(getattr(lib(), f"gr4hip_{self._prefix}_{call}")(self._h, *args), f"{self._name}.{call}")

    def reset(self):
        """drops the partial integration (from the next call on)"""
        self._call("reset")

    def set_length(self, n_integrate: int):
        """another integration length; the partial integration is dropped"""
        self._call("set_length", int(n_integrate))
        self.n_integrate = int(n_integrate)

    def pending(self, n_frames: int) -> int:
        """results (spectra, matrices) the next call of n_frames frames (per stream) completes (host only)"""
        n = C.c_size_t(0)
        self._call("pending", int(n_frames), C.byref(n))
        return int(n.value)


class SpectrumIntegrator(_Integrating):
    """Sum (mean=True: mean) of n_integrate consecutive power spectra of n_bins values, one spectrum out per n_integrate frames in (the project's own definition,
    SPECTRUM_INTEGRATOR.md: float32 leaves of 32 frames, folded in float64, one fixed order).  The partial integration is carried across calls; a call returns the
    spectra it completes, float32 [pending(frames), n_bins]."""
    _destroy, _prefix, _name = "gr4hip_specint_destroy", "specint", "SpectrumIntegrator"

    def __init__(self, n_bins: int, n_integrate: int, mean: bool = False):
        super().__init__()
        self.n_bins, self.n_integrate, self.mean = int(n_bins), int(n_integrate), bool(mean)
        check(lib().gr4hip_specint_create(C.byref(self._h), self.n_bins, self.n_integrate, capi.SPECINT_MEAN if self.mean else 0), "SpectrumIntegrator")

    def _run(self, entry, first, x, frames, out, what):
        n = self.pending(frames)
        out = _out(out, n * self.n_bins, torch.float32, x, what, (n, self.n_bins))
        got = C.c_size_t(0)
        args = (first,) if first is not None else ()
        check(entry(*args, self._h, x.data_ptr(), frames, out.data_ptr() if n else None, C.byref(got), _stream()), what)
        assert got.value == n
        return out.reshape(-1)[:n * self.n_bins].view(n, self.n_bins)

    def process_bulk(self, frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(frames, "SpectrumIntegrator")
        if x.dtype != torch.float32 or x.numel() % self.n_bins:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SpectrumIntegrator", f"expected whole float32 frames of {self.n_bins} values")
        return self._run(lib().gr4hip_specint_process, None, x, x.numel() // self.n_bins, out, "SpectrumIntegrator.process_bulk")


class CrossSpectrum(_Integrating):
    """The averaged cross-spectral matrix of n_streams (2 .. 32) streams of complex spectra of n_bins values, V_ij[c] = sum_m X_i[m][c] conj(X_j[m][c]) over
    n_integrate frames (mean=True: divided by n_integrate) -- the project's own definition, CROSS_SPECTRUM.md: float32 fma chains over leaves of 64 frames, folded
    in float64, one fixed order.  Baselines are the lower triangle j <= i, packed p = i (i + 1) / 2 + j.  The partial integration is carried across calls; a call
    returns the matrices it completes, complex64 [pending(frames), P, n_bins]."""
    _destroy, _prefix, _name = "gr4hip_xcorr_destroy", "xcorr", "CrossSpectrum"

    def __init__(self, n_streams: int, n_bins: int, n_integrate: int, mean: bool = False):
        super().__init__()
        self.n_streams, self.n_bins, self.n_integrate, self.mean = int(n_streams), int(n_bins), int(n_integrate), bool(mean)
        self.n_baselines = self.n_streams * (self.n_streams + 1) // 2
        check(lib().gr4hip_xcorr_create(C.byref(self._h), self.n_streams, self.n_bins, self.n_integrate, capi.XCORR_MEAN if self.mean else 0), "CrossSpectrum")

    def baseline(self, i: int, j: int) -> int:
        """the row of the pair (i, j), j <= i, in an emitted matrix"""
        if not 0 <= j <= i < self.n_streams:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "CrossSpectrum.baseline", f"expected 0 <= j <= i < {self.n_streams}")
        return i * (i + 1) // 2 + j

    def process_bulk(self, spectra, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """spectra: a sequence of n_streams complex64 tensors of whole frames (the same tensor may appear twice), or one [n_streams, frames, n_bins] tensor"""
        what = "CrossSpectrum.process_bulk"
        xs = [_dev(x, what) for x in (spectra.unbind(0) if isinstance(spectra, torch.Tensor) else spectra)]
        if len(xs) != self.n_streams or any(x.dtype != torch.complex64 or x.numel() != xs[0].numel() or x.device != xs[0].device for x in xs) or xs[0].numel() % self.n_bins:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"expected {self.n_streams} complex64 streams of equally many whole frames of {self.n_bins} values")
        frames = xs[0].numel() // self.n_bins
        n = self.pending(frames)
        shape = (n, self.n_baselines, self.n_bins)
        out = _out(out, n * self.n_baselines * self.n_bins, torch.complex64, xs[0], what, shape)
        ptrs = (C.c_void_p * self.n_streams)(*[x.data_ptr() for x in xs])
        got = C.c_size_t(0)
        check(lib().gr4hip_xcorr_process(self._h, ptrs, frames, out.data_ptr() if n else None, C.byref(got), _stream()), what)
        assert got.value == n
        return out.reshape(-1)[:n * self.n_baselines * self.n_bins].view(shape)

    def coherence(self, vis: torch.Tensor, i: int, j: int):
        """(msc, h1) of the pair (i, j), any order, from emitted matrices vis [..., P, n_bins]: the magnitude-squared coherence |V_ij|^2 / (V_ii V_jj), float32
        [..., n_bins], and the H1 transfer-function estimate V_ij / V_jj, complex64 [..., n_bins] -- both from float64 arithmetic rounded once"""
        what = "CrossSpectrum.coherence"
        v = _dev(vis, what)
        if v.dtype != torch.complex64 or v.dim() < 2 or tuple(v.shape[-2:]) != (self.n_baselines, self.n_bins):
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"expected complex64 [..., {self.n_baselines}, {self.n_bins}]")
        lead = tuple(v.shape[:-2])
        n = v.numel() // (self.n_baselines * self.n_bins)
        msc = torch.empty(lead + (self.n_bins,), dtype=torch.float32, device=v.device)
        h1 = torch.empty(lead + (self.n_bins,), dtype=torch.complex64, device=v.device)
        if n:
            check(lib().gr4hip_xcorr_coherence(v.data_ptr(), self.n_streams, self.n_bins, n, int(i), int(j), msc.data_ptr(), h1.data_ptr(), _stream()), what)
        return msc, h1


class Beamformer(_Handle):
    """The per-bin weighted sum of n_streams (1 .. 32) streams of complex spectra of n_bins values into n_beams (1 .. 32) beams, Y_b[f][c] = sum_s W[b][s][c]
    X_s[f][c] -- the project's own definition, BEAMFORMER.md: per beam, frame and bin one float32 fma chain over the streams in ascending order.  The handle
    holds the weights and nothing else; the state of an integration lives in the SpectrumIntegrator passed to power_integrated."""
    _destroy = "gr4hip_beamform_destroy"

    def __init__(self, n_streams: int, n_beams: int, n_bins: int):
        super().__init__()
        self.n_streams, self.n_beams, self.n_bins = int(n_streams), int(n_beams), int(n_bins)
        self._weights = None
        check(lib().gr4hip_beamform_create(C.byref(self._h), self.n_streams, self.n_beams, self.n_bins), "Beamformer")

    @staticmethod
    def delay_weights(delays_s, bin_freqs_hz, normalise: bool = True) -> np.ndarray:
        """delay-and-sum weights exp(-2 pi j f tau) (normalise: / n_streams) for delays_s [n_beams][n_streams] in seconds and the bins' frequencies [n_bins] in
        Hz: complex64 [n_beams, n_streams, n_bins], computed in float64 and rounded once"""
        tau = np.asarray(delays_s, np.float64)
        f = np.asarray(bin_freqs_hz, np.float64)
        if tau.ndim != 2 or f.ndim != 1:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Beamformer.delay_weights", "expected delays [n_beams][n_streams] and frequencies [n_bins]")
        w = np.exp(-2j * np.pi * f[None, None, :] * tau[:, :, None])
        if normalise:
            w = w / tau.shape[1]
        return w.astype(np.complex64)

    def set_weights(self, w):
        """complex64 [n_beams, n_streams, n_bins], or [n_beams, n_streams]: the same weight in every bin (expanded on the host); a device tensor is taken as it
        is.  Stream-ordered: the weights hold for every call enqueued after this one."""
        what = "Beamformer.set_weights"
        full = (self.n_beams, self.n_streams, self.n_bins)
        if isinstance(w, torch.Tensor) and w.is_cuda:
            d = w.resolve_conj()
            if d.dtype != torch.complex64 or tuple(d.shape) not in (full, full[:2]):
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"expected complex64 {full} or {full[:2]}")
            d = (d[:, :, None].expand(full) if d.dim() == 2 else d).contiguous()
        else:
            h = np.asarray(w.cpu().numpy() if isinstance(w, torch.Tensor) else w)
            if tuple(h.shape) not in (full, full[:2]):
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"expected complex64 {full} or {full[:2]}")
            h = np.array(np.broadcast_to(h[:, :, None] if h.ndim == 2 else h, full), np.complex64)  # (a copy: torch wants writable memory)
            d = torch.from_numpy(h).cuda()
        check(lib().gr4hip_beamform_set_weights(self._h, d.data_ptr(), _stream()), what)
        self._weights = d  # (kept until the next set_weights: the copy is stream-ordered)

    def _inputs(self, spectra, what):
        xs = [_dev(x, what) for x in (spectra.unbind(0) if isinstance(spectra, torch.Tensor) else spectra)]
        if len(xs) != self.n_streams or any(x.dtype != torch.complex64 or x.numel() != xs[0].numel() or x.device != xs[0].device for x in xs) or xs[0].numel() % self.n_bins:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"expected {self.n_streams} complex64 streams of equally many whole frames of {self.n_bins} values")
        return xs, xs[0].numel() // self.n_bins, (C.c_void_p * self.n_streams)(*[x.data_ptr() for x in xs])

    def process_bulk(self, spectra, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """spectra: a sequence of n_streams complex64 tensors of whole frames (the same tensor may appear twice), or one [n_streams, frames, n_bins] tensor ->
        the voltage beams, complex64 [n_beams, frames, n_bins]"""
        what = "Beamformer.process_bulk"
        xs, frames, ptrs = self._inputs(spectra, what)
        shape = (self.n_beams, frames, self.n_bins)
        out = _out(out, self.n_beams * frames * self.n_bins, torch.complex64, xs[0], what, shape)
        outs = (C.c_void_p * self.n_beams)(*[out.data_ptr() + b * frames * self.n_bins * 8 for b in range(self.n_beams)])
        check(lib().gr4hip_beamform_process(self._h, ptrs, frames, outs, self.n_bins, _stream()), what)
        return out.reshape(-1)[:self.n_beams * frames * self.n_bins].view(shape)

    def power_integrated(self, spectra, integrator: "SpectrumIntegrator", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """|Y_b|^2 followed by integrator.process_bulk() on frames [b][c], bit for bit, without the per-frame power in HBM (gr4hip_beamform_power_integrate):
        float32 [integrator.pending(frames), n_beams, n_bins]; the integrator has n_beams * n_bins bins"""
        what = "Beamformer.power_integrated"
        xs, frames, ptrs = self._inputs(spectra, what)
        n = integrator.pending(frames)
        shape = (n, self.n_beams, self.n_bins)
        out = _out(out, n * self.n_beams * self.n_bins, torch.float32, xs[0], what, shape)
        got = C.c_size_t(0)
        check(lib().gr4hip_beamform_power_integrate(self._h, integrator._h, ptrs, frames, out.data_ptr() if n else None, C.byref(got), _stream()), what)
        assert got.value == n
        return out.reshape(-1)[:n * self.n_beams * self.n_bins].view(shape)


class AdaptiveWeights(_Handle):
    """Adaptive (MVDR / Capon) beamformer weights from the matrices CrossSpectrum emits: per matrix and bin one n_streams x n_streams (2 .. 32) Hermitian
    positive-definite solve in float64 on the device, for n_beams (1 .. 32) steering vectors -- the project's own definition, ADAPTIVE_WEIGHTS.md:
    w = R'^-1 a / (a^H R'^-1 a) through a Cholesky factorisation of R' = R + loading * trace(R) / n_streams * I; the output is conj(w), laid out as
    Beamformer.set_weights reads it, so that sum_s W_s a_s = 1.  A bin whose matrix is not positive definite is NaN and counted (stats())."""
    _destroy = "gr4hip_mvdr_destroy"

    def __init__(self, n_streams: int, n_beams: int, n_bins: int, loading: float = 0.0):
        super().__init__()
        self.n_streams, self.n_beams, self.n_bins = int(n_streams), int(n_beams), int(n_bins)
        self.n_baselines = self.n_streams * (self.n_streams + 1) // 2
        self._steering = None
        check(lib().gr4hip_mvdr_create(C.byref(self._h), self.n_streams, self.n_beams, self.n_bins), "AdaptiveWeights")
        self.set_loading(loading)

    @staticmethod
    def steering_from_delays(delays_s, bin_freqs_hz) -> np.ndarray:
        """steering vectors exp(+2 pi j f tau) for delays_s [n_beams][n_streams] in seconds and the bins' frequencies [n_bins] in Hz: complex64
        [n_beams, n_streams, n_bins], computed in float64 and rounded once.  This equals conj(Beamformer.delay_weights(tau, f, normalise=False))."""
        tau = np.asarray(delays_s, np.float64)
        f = np.asarray(bin_freqs_hz, np.float64)
        if tau.ndim != 2 or f.ndim != 1:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "AdaptiveWeights.steering_from_delays", "expected delays [n_beams][n_streams] and frequencies [n_bins]")
        return np.exp(2j * np.pi * f[None, None, :] * tau[:, :, None]).astype(np.complex64)

    def set_steering(self, a):
        """complex64 [n_beams, n_streams, n_bins], or [n_beams, n_streams]: the same vector in every bin (expanded on the host); a device tensor is taken as it
        is.  Stream-ordered: the vectors hold for every call enqueued after this one."""
        what = "AdaptiveWeights.set_steering"
        full = (self.n_beams, self.n_streams, self.n_bins)
        if isinstance(a, torch.Tensor) and a.is_cuda:
            d = a.resolve_conj()
            if d.dtype != torch.complex64 or tuple(d.shape) not in (full, full[:2]):
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"expected complex64 {full} or {full[:2]}")
            d = (d[:, :, None].expand(full) if d.dim() == 2 else d).contiguous()
        else:
            h = np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
            if tuple(h.shape) not in (full, full[:2]):
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"expected complex64 {full} or {full[:2]}")
            h = np.array(np.broadcast_to(h[:, :, None] if h.ndim == 2 else h, full), np.complex64)  # (a copy: torch wants writable memory)
            d = torch.from_numpy(h).cuda()
        check(lib().gr4hip_mvdr_set_steering(self._h, d.data_ptr(), _stream()), what)
        self._steering = d  # (kept until the next set_steering: the copy is stream-ordered)

    def set_loading(self, loading: float):
        """relative diagonal loading >= 0: lambda = loading * trace(R) / n_streams is added to the diagonal.  Holds for every call enqueued after this one."""
        check(lib().gr4hip_mvdr_set_loading(self._h, float(loading)), "AdaptiveWeights.set_loading")
        self.loading = float(loading)

    def process_bulk(self, vis: torch.Tensor, out: Optional[torch.Tensor] = None, power: bool = False):
        """vis: complex64 [n_spectra, P, n_bins] (or [P, n_bins]) as CrossSpectrum.process_bulk returns it -> the weights, complex64
        [n_spectra, n_beams, n_streams, n_bins]; row q goes straight into Beamformer.set_weights.  power=True: also the Capon power estimates 1 / (a^H R'^-1 a),
        float32 [n_spectra, n_beams, n_bins], as a second value."""
        what = "AdaptiveWeights.process_bulk"
        v = _dev(vis, what)
        per = self.n_baselines * self.n_bins
        if v.dtype != torch.complex64 or v.numel() % per:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, what, f"expected complex64 matrices of {self.n_baselines} baselines of {self.n_bins} bins")
        n = v.numel() // per
        shape = (n, self.n_beams, self.n_streams, self.n_bins)
        numel = n * self.n_beams * self.n_streams * self.n_bins
        out = _out(out, numel, torch.complex64, v, what, shape)
        p = torch.empty((n, self.n_beams, self.n_bins), dtype=torch.float32, device=v.device) if power else None
        check(lib().gr4hip_mvdr_process(self._h, v.data_ptr(), n, out.data_ptr(), p.data_ptr() if power else None, _stream()), what)
        w = out.reshape(-1)[:numel].view(shape)
        return (w, p) if power else w

    def stats(self):
        """(bins solved, bins failed) over every (matrix, bin) processed since the block was made; waits for the block's last call"""
        solved, failed = C.c_ulonglong(0), C.c_ulonglong(0)
        check(lib().gr4hip_mvdr_stats(self._h, C.byref(solved), C.byref(failed)), "AdaptiveWeights.stats")
        return solved.value, failed.value


class Chain(_Handle):
    """complex<float> fir_filter -> FFT frames -> |X|^2, one fused device pipeline (BASELINE.json configs[1])."""
    _destroy = "gr4hip_chain_destroy"

    def __init__(self, b: Sequence[float], fftSize: int = 8192, window="None", algo: int = capi.CHAIN_AUTO):
        super().__init__()
        self.b = np.ascontiguousarray(b, np.float32)
        self.fftSize = int(fftSize)
        check(lib().gr4hip_chain_create(C.byref(self._h), self.b.ctypes.data, len(self.b), self.fftSize, _window_id(window), algo), "Chain")
        a = C.c_int(0)
        check(lib().gr4hip_chain_get_algo(self._h, C.byref(a)), "Chain.algo")
        self.algo = a.value

    def set_max_workgroups(self, n: int):
        """cap the persistent grid of the fused kernels (0 = every CU); leaves CUs to kernels on other streams, e.g. an RCCL fan-in"""
        check(lib().gr4hip_chain_set_max_workgroups(self._h, int(n)), "Chain.set_max_workgroups")

    def reset(self):
        check(lib().gr4hip_chain_reset(self._h), "Chain.reset")

    def last_power_ratio(self):
        """(output / input power of the last measured fused launch or -1, chain now in the time domain?) -- the dynamic-range guard of CHAIN_AUTO (include/gr4hip.h)"""
        r, td = C.c_float(0), C.c_int(0)
        check(lib().gr4hip_chain_last_power_ratio(self._h, C.byref(r), C.byref(td), _stream()), "Chain.last_power_ratio")
        return r.value, bool(td.value)

    def last_guard_fractions(self):
        """(fraction of the last measured launch's frames the fused kernel marked or -1, fraction of all frames since create / reset that ended in float64)"""
        m, f = C.c_float(0), C.c_float(0)
        check(lib().gr4hip_chain_last_guard_fractions(self._h, C.byref(m), C.byref(f), _stream()), "Chain.last_guard_fractions")
        return m.value, f.value

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "Chain")
        if x.dtype != torch.complex64:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Chain", "input must be complex64")
        frames = x.numel() // self.fftSize
        out = _out(out, frames * self.fftSize, torch.float32, x, "Chain.process", (frames, self.fftSize))
        nf = C.c_size_t(0)
        check(lib().gr4hip_chain_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), C.byref(nf), _stream()), "Chain.process")
        return out

    def set_guard_mode(self, mode: int):
        """capi.GUARD_STRICT (default: the frames a launch marks are evaluated again in the time domain by a launch enqueued behind it; asynchronous),
        GUARD_DEFERRED (no second evaluation: the call that measures the drop is published from the fused kernel, the switch lags one call) or GUARD_OFF (include/gr4hip.h)"""
        check(lib().gr4hip_chain_set_guard_mode(self._h, int(mode)), "Chain.set_guard_mode")


def chain_process_multi(chains: Sequence[Chain], xs: Sequence[torch.Tensor], outs: Optional[Sequence[torch.Tensor]] = None,
                        sum_out: Optional[torch.Tensor] = None, want_outs: bool = True):
    """n chains fed the same number of samples in ONE call (gr4hip_chain_process_multi): the parallel SDR channels of a flowgraph that share
    this device.  Returns (outs or None, sum_out or None).  want_outs=False with sum_out given: only the combiner output sum_i |FFT(fir(x_i))|^2
    (math::Add over the channels) is produced -- one launch with the fold in registers when all chains have the same taps."""
    n = len(chains)
    assert n >= 1 and len(xs) == n
    xs = [_dev(x, "chain_process_multi") for x in xs]
    N = chains[0].fftSize
    frames = xs[0].numel() // N
    for x in xs:
        if x.dtype != torch.complex64 or x.numel() != xs[0].numel():
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "chain_process_multi", "inputs must be complex64 spans of one length")
    if want_outs and outs is None:
        outs = [torch.empty((frames, N), dtype=torch.float32, device=xs[0].device) for _ in range(n)]
    if not want_outs:
        outs = None
        if sum_out is None:
            sum_out = torch.empty((frames, N), dtype=torch.float32, device=xs[0].device)
    hs = (C.c_void_p * n)(*[c._h for c in chains])
    ins = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    os_ = (C.c_void_p * n)(*[o.data_ptr() for o in outs]) if outs is not None else None
    nf = C.c_size_t(0)
    check(lib().gr4hip_chain_process_multi(hs, n, ins, xs[0].numel(), os_, sum_out.data_ptr() if sum_out is not None else None, C.byref(nf), _stream()),
          "chain_process_multi")
    return outs, sum_out


class FirBatched(_Handle):
    """nchannels independent fir_filter<float> instances with per-channel taps b[c][k] on channel-major samples x[c][n]
    (BASELINE.json configs[3]); evaluated as a block-Toeplitz contraction on the f32 MFMA units."""
    _destroy = "gr4hip_fir_batched_destroy"

    def __init__(self, b):
        super().__init__()
        self.b = np.ascontiguousarray(b, np.float32)
        if self.b.ndim != 2:
            raise ValueError("taps must be [nchannels][ntaps]")
        check(lib().gr4hip_fir_batched_create(C.byref(self._h), self.b.shape[0], self.b.ctypes.data, self.b.shape[1]), "FirBatched")

    def reset(self):
        check(lib().gr4hip_fir_batched_reset(self._h), "FirBatched.reset")

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x: [nchannels][n]; rows may lie apart (a view with unit inner stride is read in place, row stride = x.stride(0)).  out (optional): [nchannels][>= n] on the
        same terms; the library wants it 16-byte aligned with a row stride that is a multiple of 4."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "FirBatched", "input must be a CUDA/HIP torch tensor (device-only path)")
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != self.b.shape[0]:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "FirBatched", "input must be float32 [nchannels][n]")
        nch, n = x.shape
        if n > 0 and not (x.stride(1) == 1 and (nch == 1 or x.stride(0) >= n)):  # rows that overlap, run backwards or are not unit-stride: a copy
            x = x.contiguous()
        if out is None:
            out = torch.empty((nch, (n + 3) // 4 * 4), dtype=torch.float32, device=x.device)
        elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != x.device or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != nch
              or out.shape[1] < n or (n > 0 and not (out.stride(1) == 1 and (nch == 1 or out.stride(0) >= n)))):
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "FirBatched", f"out must be a float32 tensor on the input's device, [{nch}][>= {n}] with unit inner stride and rows that do not overlap")
        in_stride, out_stride = (x.stride(0), out.stride(0)) if nch > 1 else ((n + 3) // 4 * 4,) * 2  # (one row: no stride is ever applied, and torch reports any for a dimension of size 1)
        check(lib().gr4hip_fir_batched_process(self._h, x.data_ptr(), in_stride, n, out.data_ptr(), out_stride, _stream()), "FirBatched.process")
        return out[:, :n]


def _uncertain_id(t: torch.Tensor, who: str) -> int:
    """gr::UncertainValue<float | double> streams are float tensors of shape [n, 2]: rows of {value, uncertainty} (meta/.../UncertainValue.hpp:34-40)"""
    if t.dim() != 2 or t.shape[1] != 2 or t.dtype not in (torch.float32, torch.float64):
        raise capi.Gr4HipError(capi.INVALID_ARGUMENT, who, "UncertainValue streams are float32 / float64 tensors of shape [n, 2]")
    return capi.UF32 if t.dtype == torch.float32 else capi.UF64


def math_const(op, x: torch.Tensor, value, uncertain: bool = False) -> torch.Tensor:
    """MathOpImpl<T,op>::processOne (Math.hpp:38-56): AddConst / SubtractConst / MultiplyConst / DivideConst.
    uncertain: T = UncertainValue<float | double> -- x of shape [n, 2], value = (value, uncertainty)."""
    x = _dev(x, "math_const")
    if uncertain:
        did = _uncertain_id(x, "math_const")
        v = np.asarray(value, np.float32 if did == capi.UF32 else np.float64).reshape(2)
        n = x.shape[0]
    else:
        did = _DTYPE_ID[x.dtype]
        v = np.array([value]).astype(_NP_DTYPE[did])
        n = x.numel()
    out = torch.empty_like(x)
    check(lib().gr4hip_math_const(_OPS.get(op, op), did, x.data_ptr(), out.data_ptr(), n, v.ctypes.data, _stream()), "math_const")
    return out


def math_nary(op, inputs: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None, uncertain: bool = False) -> torch.Tensor:
    """MathOpMultiPortImpl<T,op>::processBulk (Math.hpp:100-107): Add / Subtract / Multiply / Divide over n_inputs.
    `out` (optional): a contiguous device tensor of the inputs' dtype and length that receives the result.
    uncertain: T = UncertainValue<float | double>, every stream of shape [n, 2]."""
    ins = [_dev(t, "math_nary") for t in inputs]
    if not 1 <= len(ins) <= 32:
        raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "math_nary", "n_inputs must be in [1, 32] (Math.hpp:90)")
    if any(t.dtype != ins[0].dtype or t.numel() != ins[0].numel() for t in ins):
        raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "math_nary", "all inputs need the same dtype and length")
    ptrs = (C.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    if out is None:
        out = torch.empty_like(ins[0])
    elif not out.is_cuda or not out.is_contiguous() or out.dtype != ins[0].dtype or out.numel() != ins[0].numel():
        raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "math_nary", "out must be a contiguous device tensor of the inputs' dtype and length")
    did = _uncertain_id(ins[0], "math_nary") if uncertain else _DTYPE_ID[ins[0].dtype]
    check(lib().gr4hip_math_nary(_OPS.get(op, op), did, ptrs, len(ins), out.data_ptr(), ins[0].shape[0] if uncertain else out.numel(), _stream()), "math_nary")
    return out


class Merged(_Handle):
    """A run of per-sample blocks as ONE launch: the run-time counterpart of Merge<A, "out", B, "in"> (core/.../BlockMerging.hpp:126-240) for chains of
    MathOpImpl<T, op> (Math.hpp:38-56) and Rotator<complex<float>> (Rotator.hpp:51-61; closed-form phase).  `ops`: a sequence of
    ("Add" | "Subtract" | "Multiply" | "Divide", value) and ("Rotator", phase_increment[, initial_phase]) in stream order.  2 sizeof(T) bytes of HBM traffic per
    sample whatever the length; integer types bit-exact, float ops single IEEE operations in program order (include/gr4hip.h, gr4hip_ewise_*).
    The same object is what fir_filter.set_prologue / set_epilogue take."""
    _destroy = "gr4hip_ewise_destroy"

    def __init__(self, dtype, ops=()):
        super().__init__()
        self.dtype = dtype
        self._did = _DTYPE_ID[dtype]
        check(lib().gr4hip_ewise_create(C.byref(self._h), self._did), "Merged")
        self.ops = []
        for op in ops:
            self.append(*op)

    def append(self, op, *args):
        if op == "Rotator":
            inc = float(np.float32(args[0]))
            ph0 = float(np.float32(args[1])) if len(args) > 1 else 0.0
            check(lib().gr4hip_ewise_append_rotator(self._h, inc, ph0), "Merged.append_rotator")
        else:
            v = np.array([args[0]]).astype(_NP_DTYPE[self._did])
            check(lib().gr4hip_ewise_append_const(self._h, _OPS[op], v.ctypes.data), "Merged.append_const")
        self.ops.append((op,) + tuple(args))
        return self

    def reset(self):
        check(lib().gr4hip_ewise_reset(self._h), "Merged.reset")

    @property
    def position(self) -> int:
        v = C.c_uint64(0)
        check(lib().gr4hip_ewise_position(self._h, C.byref(v)), "Merged.position")
        return v.value

    def decimate(self, x: torch.Tensor, decim: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decimator<T> with this program's blocks behind it in ONE launch: out[m] = program(x[m * decim]) (gr4hip_ewise_decimate)"""
        x = _dev(x, "Merged.decimate")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Merged", f"expected {self.dtype}, got {x.dtype}")
        n_out = -(-x.numel() // int(decim))
        out = _out(out, n_out, self.dtype, x, "Merged.decimate")
        check(lib().gr4hip_ewise_decimate(self._h, x.data_ptr(), x.numel(), int(decim), out.data_ptr(), None, _stream()), "Merged.decimate")
        return out

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "Merged")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Merged", f"expected {self.dtype}, got {x.dtype}")
        out = _out(out, x.numel(), x.dtype, x, "Merged.process")
        check(lib().gr4hip_ewise_process(self._h, x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "Merged.process")
        return out


class Rotator(_Handle):
    """gr::blocks::math::Rotator<complex<float>> (Rotator.hpp:16-63): XOR settings frequency_shift / phase_increment.
    algo: "closed_form" (default: float64 phase of sample i = carried + (i+1) inc, HBM-bound) or "recurrence" (the reference's float
    accumulator bit for bit, sequential); the carried phase is the same float member either way (include/gr4hip.h)."""
    _destroy = "gr4hip_rotator_destroy"

    def __init__(self, phase_increment: Optional[float] = None, frequency_shift: Optional[float] = None, sample_rate: float = 1.0,
                 initial_phase: float = 0.0, algo: str = "closed_form", dtype=torch.complex64):
        super().__init__()
        if phase_increment is not None and frequency_shift is not None:  # Rotator.hpp:45-46 throws
            raise ValueError("cannot set both 'frequency_shift' and 'phase_increment' in new setting (XOR)")
        self.dtype = dtype
        self._f64 = dtype == torch.complex128  # Rotator<complex<double>> (Rotator.hpp:15): closed form in float64 (csrc/f64.hip)
        if self._f64:
            self._destroy = "gr4hip_rotator64_destroy"
            self.sample_rate = float(sample_rate)
            if frequency_shift is not None:
                self.frequency_shift = float(frequency_shift)
                self.phase_increment = 2.0 * np.pi * self.frequency_shift / self.sample_rate
            else:
                self.phase_increment = float(phase_increment or 0.0)
                self.frequency_shift = self.phase_increment / (2.0 * np.pi) * self.sample_rate
            self.initial_phase, self.algo = float(initial_phase), "closed_form"
            check(lib().gr4hip_rotator64_create(C.byref(self._h), self.phase_increment, self.initial_phase), "Rotator<complex128>")
            return
        self.sample_rate = np.float32(sample_rate)
        if frequency_shift is not None:  # :41-42 (float arithmetic)
            self.frequency_shift = np.float32(frequency_shift)
            self.phase_increment = np.float32(2) * np.float32(np.float32(np.pi) * self.frequency_shift / self.sample_rate)
        else:
            self.phase_increment = np.float32(phase_increment or 0.0)
            self.frequency_shift = np.float32(self.phase_increment / (np.float32(2) * np.float32(np.pi))) * self.sample_rate
        self.initial_phase = np.float32(initial_phase)
        check(lib().gr4hip_rotator_create(C.byref(self._h), float(self.phase_increment), float(self.initial_phase)), "Rotator")
        self.set_algo(algo)

    def set_algo(self, algo: str):
        ids = {"closed_form": capi.ROTATOR_CLOSED_FORM, "recurrence": capi.ROTATOR_RECURRENCE}
        if algo not in ids:
            raise ValueError(f"unknown rotator algo '{algo}'")
        if self._f64:
            if algo != "closed_form":
                raise capi.Gr4HipError(capi.UNSUPPORTED, "Rotator", "the float64 rotator has the closed form only")
            return
        check(lib().gr4hip_rotator_set_algo(self._h, ids[algo]), "Rotator.set_algo")
        self.algo = algo

    def settings_changed(self, initial_phase: float = 0.0):
        """settingsChanged (Rotator.hpp:40-49): _accumulated_phase = initial_phase.  Host-side note; the device word (recurrence) is stored on the next call's stream."""
        if self._f64:
            check(lib().gr4hip_rotator64_reset(self._h, float(initial_phase)), "Rotator.reset")
        else:
            check(lib().gr4hip_rotator_reset(self._h, float(np.float32(initial_phase))), "Rotator.reset")
        self.initial_phase = initial_phase

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "Rotator")
        if x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Rotator", f"expected {self.dtype}, got {x.dtype}")
        out = _out(out, x.numel(), x.dtype, x, "Rotator.process")
        fn = lib().gr4hip_rotator64_process if self._f64 else lib().gr4hip_rotator_process
        check(fn(self._h, x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "Rotator.process")
        return out

    @property
    def accumulated_phase(self) -> float:
        if self._f64:
            d = C.c_double(0)
            check(lib().gr4hip_rotator64_phase(self._h, C.byref(d)), "Rotator.phase")
            return d.value
        v = C.c_float(0)
        check(lib().gr4hip_rotator_phase(self._h, C.byref(v), _stream()), "Rotator.phase")
        return v.value


class _FrequencyEstimator(_Handle):
    """gr::filter::FrequencyEstimator{TimeDomain,FrequencyDomain}<float> (FrequencyEstimator.hpp:30-351) with the reference's setting names plus `chunk`
    (inputs per output: 1 = processOne; decimating=True gives the decimating form's chunk, 10 / N).  process_bulk takes a multiple of `chunk` samples and returns
    one estimate per chunk; every fallback of the reference repeats the previous output (include/gr4hip.h "frequency estimators").  A new block starts from
    f_expected; reset() goes back to it, set_params() keeps the last estimate."""
    _destroy = "gr4hip_freqest_destroy"
    _method = None
    _names = ("sample_rate", "f_min", "f_expected", "f_max", "epsilon")

    def __init__(self, chunk: Optional[int] = None, decimating: bool = False, **settings):
        super().__init__()
        self._decimating = bool(decimating) and chunk is None
        self._p = self._params(capi.FreqEstParams(), settings, chunk, init=True)
        check(lib().gr4hip_freqest_create(C.byref(self._h), self._method, C.byref(self._p)), type(self).__name__)

    def _params(self, p, settings, chunk, init=False):
        if init:
            check(lib().gr4hip_freqest_params_default(self._method, C.byref(p)), type(self).__name__)
        for k, v in settings.items():
            if k not in self._names + (self._extra,):
                raise TypeError(f"{type(self).__name__}: unknown setting '{k}'")
            setattr(p, k, v)
        if chunk is not None:
            p.chunk = int(chunk)
        elif self._decimating:
            p.chunk = self._decimating_chunk(p)
        return p

    def _decimating_chunk(self, p) -> int:
        raise NotImplementedError

    def geometry(self):
        """(W, i_min, i_max): the samples each estimate is taken over and, for the frequency domain, the clamped search range [i_min, i_max)"""
        w, a, b = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(lib().gr4hip_freqest_geometry(self._method, C.byref(self._p), C.byref(w), C.byref(a), C.byref(b)), type(self).__name__)
        return w.value, a.value, b.value

    @property
    def chunk(self) -> int:
        return int(self._p.chunk)

    def __getattr__(self, name):
        if name in type(self)._names + (type(self)._extra,):
            return getattr(self.__dict__["_p"], name)
        raise AttributeError(name)

    def set_params(self, chunk: Optional[int] = None, **settings):
        """settingsChanged: the histories are emptied, the last estimate is kept"""
        p = self._params(capi.FreqEstParams.from_buffer_copy(self._p), settings, chunk)
        check(lib().gr4hip_freqest_set_params(self._h, C.byref(p)), f"{type(self).__name__}.set_params")
        self._p = p

    def reset(self):
        """reset(): the histories are emptied, the last estimate becomes f_expected"""
        check(lib().gr4hip_freqest_reset(self._h), f"{type(self).__name__}.reset")

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, type(self).__name__)
        if x.dtype != torch.float32:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, type(self).__name__, f"expected torch.float32, got {x.dtype}")
        n_out = x.numel() // self.chunk
        out = _out(out, n_out, torch.float32, x, f"{type(self).__name__}.process")
        check(lib().gr4hip_freqest_process(self._h, x.data_ptr(), x.numel(), out.data_ptr(), None, _stream()), f"{type(self).__name__}.process")
        return out[:n_out]


class FrequencyEstimatorTimeDomain(_FrequencyEstimator):
    """FrequencyEstimatorTimeDomain<float> (FrequencyEstimator.hpp:30-176); decimating=True: FrequencyEstimatorTimeDomainDecimating (Resampling<10U>, :179)"""
    _method = capi.FREQEST_TIME_DOMAIN
    _extra = "n_periods"

    def _decimating_chunk(self, p) -> int:
        return 10


class FrequencyEstimatorFrequencyDomain(_FrequencyEstimator):
    """FrequencyEstimatorFrequencyDomain<float> (FrequencyEstimator.hpp:186-351); decimating=True: the decimating form, chunk = N (initialiseFFT, :231-242)"""
    _method = capi.FREQEST_FREQUENCY_DOMAIN
    _extra = "min_fft_size"

    def _decimating_chunk(self, p) -> int:
        w = C.c_size_t(0)
        check(lib().gr4hip_freqest_geometry(self._method, C.byref(p), C.byref(w), None, None), type(self).__name__)
        return int(w.value)


class IQDemodulator(_Handle):
    """gr::filter::IQDemodulator<T> (FrequencyEstimator.hpp:356-653), T in {float32, float64}: a lock-in amplifier with the reference's setting names plus
    `chunk` (input_chunk_size, the registered Resampling<1024U, 1U, false>).  process_bulk(ref, resp) takes a multiple of `chunk` samples of each input and
    returns (amplitude, phase, frequency), one value per chunk (include/gr4hip.h "IQ demodulator").  set_params re-initialises the filters iff it names
    sample_rate, f_high_pass, f_low_pass or derivative_method (settingsChanged, :454-466); reset() always does."""
    _destroy = "gr4hip_iqdemod_destroy"
    _names = ("sample_rate", "f_high_pass", "f_low_pass", "phase_unit", "invert_phase", "derivative_method", "epsilon")
    _filter_keys = ("sample_rate", "f_high_pass", "f_low_pass", "derivative_method")

    def __init__(self, dtype=torch.float32, chunk: int = 1024, **settings):
        super().__init__()
        if dtype not in (torch.float32, torch.float64):
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "IQDemodulator", f"dtype {dtype}: float32 or float64")
        self.dtype = dtype
        p = capi.IQDemodParams()
        check(lib().gr4hip_iqdemod_params_default(C.byref(p)), "IQDemodulator")
        self._p = self._params(p, settings, chunk)
        check(lib().gr4hip_iqdemod_create(C.byref(self._h), _DTYPE_ID[dtype], C.byref(self._p)), "IQDemodulator")

    def _params(self, p, settings, chunk):
        for k, v in settings.items():
            if k not in self._names:
                raise TypeError(f"IQDemodulator: unknown setting '{k}'")
            if k == "phase_unit" and isinstance(v, str):
                v = {"radians": 0, "degrees": 1}[v.lower()]
            setattr(p, k, int(v) if k in ("phase_unit", "invert_phase", "derivative_method") else v)
        if chunk is not None:
            p.chunk = int(chunk)
        return p

    @property
    def chunk(self) -> int:
        return int(self._p.chunk)

    def __getattr__(self, name):
        if name in type(self)._names:
            return getattr(self.__dict__["_p"], name)
        raise AttributeError(name)

    def set_params(self, chunk: Optional[int] = None, **settings):
        """settingsChanged: a filter key in `settings` re-initialises the filters, the other settings (and chunk) keep their state"""
        p = self._params(capi.IQDemodParams.from_buffer_copy(self._p), settings, chunk)
        reinit = any(k in self._filter_keys for k in settings)
        check(lib().gr4hip_iqdemod_set_params(self._h, C.byref(p), int(reinit)), "IQDemodulator.set_params")
        self._p = p

    def reset(self):
        """reset(): the filters are re-initialised"""
        check(lib().gr4hip_iqdemod_reset(self._h), "IQDemodulator.reset")

    def process_bulk(self, ref: torch.Tensor, resp: torch.Tensor, amplitude: Optional[torch.Tensor] = None, phase: Optional[torch.Tensor] = None,
                     frequency: Optional[torch.Tensor] = None):
        ref, resp = _dev(ref, "IQDemodulator"), _dev(resp, "IQDemodulator")
        if ref.dtype != self.dtype or resp.dtype != self.dtype or ref.numel() != resp.numel() or ref.device != resp.device:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "IQDemodulator", f"ref and resp must be {self.dtype} tensors of one length on one device")
        n = ref.numel()
        n_out = n // self.chunk
        outs = [_out(o, n_out, self.dtype, ref, "IQDemodulator.process") for o in (amplitude, phase, frequency)]
        check(lib().gr4hip_iqdemod_process(self._h, ref.data_ptr(), resp.data_ptr(), n, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None,
                                           _stream()), "IQDemodulator.process")
        return tuple(o[:n_out] for o in outs)


class PowerMetrics(_Handle):
    """gr::electrical::PowerMetrics<float32, nPhases> (PowerEstimators.hpp:21-131) with the reference's setting names.  process_bulk(u, i) takes two
    [n_phases, n] float32 tensors, n a multiple of `decimate` (a 1-D tensor is one phase; rows may be strided views, read in place), and returns
    (P, Q, S, U_rms, I_rms), each [n_phases, n / decimate] (include/gr4hip.h "Power metrics").  set_params always re-initialises the filters
    (settingsChanged, :95), reset() zeroes their states."""
    _destroy = "gr4hip_powermetrics_destroy"
    _names = ("sample_rate", "high_pass", "low_pass", "decimate")

    def __init__(self, n_phases: int = 1, **settings):
        super().__init__()
        p = capi.PowerMetricsParams()
        check(lib().gr4hip_powermetrics_params_default(C.byref(p)), "PowerMetrics")
        p.n_phases = int(n_phases)
        self._p = self._params(p, settings)
        check(lib().gr4hip_powermetrics_create(C.byref(self._h), C.byref(self._p)), "PowerMetrics")

    @staticmethod
    def segment() -> int:
        """samples per workgroup segment: where the kernels hand their carries over"""
        return int(lib().gr4hip_powermetrics_segment())

    def _params(self, p, settings):
        for k, v in settings.items():
            if k not in self._names:
                raise TypeError(f"PowerMetrics: unknown setting '{k}'")
            setattr(p, k, int(v) if k == "decimate" else v)
        return p

    @property
    def n_phases(self) -> int:
        return int(self._p.n_phases)

    def __getattr__(self, name):
        if name in type(self)._names:
            return getattr(self.__dict__["_p"], name)
        raise AttributeError(name)

    def set_params(self, **settings):
        """settingsChanged: every filter is rebuilt, whatever the update names"""
        p = self._params(capi.PowerMetricsParams.from_buffer_copy(self._p), settings)
        check(lib().gr4hip_powermetrics_set_params(self._h, C.byref(p)), "PowerMetrics.set_params")
        self._p = p

    def reset(self):
        check(lib().gr4hip_powermetrics_reset(self._h), "PowerMetrics.reset")

    def _rows(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PowerMetrics", "input must be a CUDA/HIP torch tensor (device-only path)")
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] != self.n_phases:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PowerMetrics", f"inputs must be float32 tensors of shape [{self.n_phases}, n]")
        if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
            x = x.contiguous()  # only rows of unit stride, a row stride apart, are read in place
        return x

    def process_bulk(self, u: torch.Tensor, i: torch.Tensor, outputs=("P", "Q", "S", "U_rms", "I_rms")):
        """`outputs`: the ones to compute; the others come back as None (their pointers are NULL in the call)"""
        u, i = self._rows(u), self._rows(i)
        if u.shape != i.shape or u.device != i.device:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "PowerMetrics", "u and i must have one shape on one device")
        n = u.shape[1]
        stride = u.stride(0) if self.n_phases > 1 else max(n, 1)
        if self.n_phases > 1 and i.stride(0) != stride:
            i = i.contiguous()
            if i.stride(0) != stride:
                u = u.contiguous()
                stride = n
        n_out = n // int(self._p.decimate)
        outs = [torch.empty((self.n_phases, n_out), dtype=torch.float32, device=u.device) if k in outputs else None for k in ("P", "Q", "S", "U_rms", "I_rms")]
        ptr = [o.data_ptr() if o is not None else None for o in outs]
        check(lib().gr4hip_powermetrics_process(self._h, u.data_ptr(), i.data_ptr(), stride, n, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], max(n_out, 1), None,
                                                _stream()), "PowerMetrics.process")
        return tuple(outs)


class _ElectricalRows:
    """the row handling PowerFactor and SystemUnbalance share: [n_phases, n] device tensors of the block's dtype, rows of unit stride a common row stride apart are
    read in place (the layout of PowerMetrics' outputs), anything else is made contiguous first"""
    _what = ""
    _min_phases = 1

    def __init__(self, n_phases: int = 3, dtype=torch.float32):
        if dtype not in (torch.float32, torch.float64) or not self._min_phases <= int(n_phases) <= 16:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, self._what, f"dtype float32 or float64, n_phases in [{self._min_phases}, 16]")
        self.n_phases = int(n_phases)
        self.dtype = dtype

    @staticmethod
    def tile() -> int:
        """items per workgroup of the kernels: where the aligned body hands over to the element-wise tail"""
        return int(lib().gr4hip_electrical_tile())

    def _rows(self, xs):
        rows = []
        for x in xs:
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, self._what, "input must be a CUDA/HIP torch tensor (device-only path)")
            if x.dim() == 1:
                x = x.unsqueeze(0)
            if x.dim() != 2 or x.dtype != self.dtype or x.shape[0] != self.n_phases:
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, self._what, f"inputs must be {self.dtype} tensors of shape [{self.n_phases}, n]")
            if rows and (x.shape != rows[0].shape or x.device != rows[0].device):
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, self._what, "the inputs must have one shape on one device")
            if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
                x = x.contiguous()
            rows.append(x)
        n = rows[0].shape[1]
        stride = rows[0].stride(0) if self.n_phases > 1 else max(n, 1)
        if self.n_phases > 1 and any(x.stride(0) != stride for x in rows):
            rows, stride = [x.contiguous() for x in rows], max(n, 1)
        return rows, n, stride


class PowerFactor(_ElectricalRows):
    """gr::electrical::PowerFactor<T, nPhases> (PowerEstimators.hpp:144-182), T float32 or float64.  process(P, S) takes two [n_phases, n] tensors (a 1-D tensor is
    one phase; rows may be strided views such as PowerMetrics' outputs, read in place) and returns (power_factor, phase), each [n_phases, n]
    (include/gr4hip.h "Power factor and system unbalance", POWER_QUALITY.md)."""
    _what = "PowerFactor"
    _outputs = ("power_factor", "phase")

    def process(self, P: torch.Tensor, S: torch.Tensor, outputs=_outputs):
        """`outputs`: the ones to compute; the others come back as None (their pointers are NULL in the call)"""
        (P, S), n, stride = self._rows((P, S))
        outs = [torch.empty((self.n_phases, n), dtype=self.dtype, device=P.device) if k in outputs else None for k in self._outputs]
        ptr = [o.data_ptr() if o is not None else None for o in outs]
        check(lib().gr4hip_powerfactor_process(_DTYPE_ID[self.dtype], self.n_phases, P.data_ptr(), S.data_ptr(), stride, ptr[0], ptr[1], max(n, 1), n, _stream()),
              "PowerFactor.process")
        return tuple(outs)

    process_bulk = process


class SystemUnbalance(_ElectricalRows):
    """gr::electrical::SystemUnbalance<T, nPhases> (PowerEstimators.hpp:193-257), T float32 or float64, nPhases >= 2.  process(U_rms, I_rms, P) takes three
    [n_phases, n] tensors (rows may be strided views, read in place) and returns (P_total, U_unbalance, I_unbalance), each [n]."""
    _what = "SystemUnbalance"
    _min_phases = 2
    _outputs = ("P_total", "U_unbalance", "I_unbalance")

    def process(self, U_rms: torch.Tensor, I_rms: torch.Tensor, P: torch.Tensor, outputs=_outputs):
        """`outputs`: the ones to compute; the others come back as None (their pointers are NULL in the call)"""
        (U, I, P), n, stride = self._rows((U_rms, I_rms, P))
        outs = [torch.empty(n, dtype=self.dtype, device=U.device) if k in outputs else None for k in self._outputs]
        ptr = [o.data_ptr() if o is not None else None for o in outs]
        check(lib().gr4hip_unbalance_process(_DTYPE_ID[self.dtype], self.n_phases, U.data_ptr(), I.data_ptr(), P.data_ptr(), stride, ptr[0], ptr[1], ptr[2], n,
                                             _stream()), "SystemUnbalance.process")
        return tuple(outs)

    process_bulk = process


class SchmittEdges(NamedTuple):
    """the edges of one SchmittTrigger.process_bulk call, in order of `sample`: `count` edges were detected, the tensors hold the first min(count, capacity)"""
    count: int
    sample: torch.Tensor       # int64: index within the call's input at which processOne returned the edge
    kind: torch.Tensor         # int32: 1 RISING, 2 FALLING (gr::trigger::EdgeDetection)
    edge_idx: torch.Tensor     # int32: lastEdgeIdx
    edge_offset: torch.Tensor  # float32: value(lastEdgeOffset)
    n_fit: torch.Tensor        # int32: the regression's n (0 for NO, 2 for BASIC)
    flags: torch.Tensor        # int32: kind_flags without the kind (capi.SCHMITT_DEGENERATE)


class SchmittTrigger(_Handle):
    """gr::trigger::SchmittTrigger<T, Method, 32> (algorithm/.../SchmittTrigger.hpp:39-357), the detector of gr::blocks::basic::SchmittTrigger
    (blocks/basic/.../Trigger.hpp:45), for T in {int16, int32, float32, float64}: processOne applied to every sample once, in order, whatever the chunking into
    calls (include/gr4hip.h "Schmitt trigger").  `method`: "NO_INTERPOLATION", "BASIC_LINEAR_INTERPOLATION", "LINEAR_INTERPOLATION" or the enum's number;
    "POLYNOMIAL_INTERPOLATION" raises (UNSUPPORTED).  set_params resets the detector (settingsChanged, Trigger.hpp:76-80)."""
    _destroy = "gr4hip_schmitt_destroy"
    METHODS = ("NO_INTERPOLATION", "BASIC_LINEAR_INTERPOLATION", "LINEAR_INTERPOLATION", "POLYNOMIAL_INTERPOLATION")
    _dtypes = {torch.int16: capi.I16, torch.int32: capi.I32, torch.float32: capi.F32, torch.float64: capi.F64}

    def __init__(self, offset: float = 0.0, threshold: float = 1.0, method="NO_INTERPOLATION", dtype=torch.float32):
        super().__init__()
        if dtype not in self._dtypes:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SchmittTrigger", f"dtype {dtype} (int16, int32, float32, float64)")
        self.dtype = dtype
        self._p = self._params(offset, threshold, method)
        check(lib().gr4hip_schmitt_create(C.byref(self._h), C.byref(self._p)), "SchmittTrigger")

    @staticmethod
    def segment() -> int:
        """samples per workgroup segment: where the kernels hand their carries over"""
        return int(lib().gr4hip_schmitt_segment())

    @staticmethod
    def walk_tile() -> int:
        """segments per workgroup of the carry walk: a longer call has its carries from several workgroups"""
        return int(lib().gr4hip_schmitt_walk_tile())

    def _params(self, offset, threshold, method):
        if isinstance(method, str):
            if method not in self.METHODS:
                raise ValueError(f"SchmittTrigger: unknown method '{method}'")
            method = self.METHODS.index(method)
        return capi.SchmittParams(float(offset), float(threshold), int(method), self._dtypes[self.dtype])

    offset = property(lambda self: self._p.offset)
    threshold = property(lambda self: self._p.threshold)
    method = property(lambda self: self.METHODS[self._p.method])

    def set_params(self, offset=None, threshold=None, method=None):
        p = self._params(self._p.offset if offset is None else offset, self._p.threshold if threshold is None else threshold,
                         self._p.method if method is None else method)
        check(lib().gr4hip_schmitt_set_params(self._h, C.byref(p)), "SchmittTrigger.set_params")
        self._p = p

    def reset(self):
        check(lib().gr4hip_schmitt_reset(self._h), "SchmittTrigger.reset")

    def process_bulk(self, x: torch.Tensor, capacity: Optional[int] = None) -> SchmittEdges:
        """the edges of x (1-D, the handle's dtype); at most `capacity` (default len(x)) are returned, `count` says how many there were.  Reads the count back,
        so it waits for the call's stream."""
        x = _dev(x, "SchmittTrigger")
        if x.dim() != 1 or x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SchmittTrigger", f"input must be a 1-D {self.dtype} tensor")
        n = x.numel()
        cap = n if capacity is None else int(capacity)
        if cap < 0:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SchmittTrigger", f"capacity {cap}")
        buf = torch.empty((max(cap, 1), capi.SCHMITT_EDGE_BYTES // 4), dtype=torch.int32, device=x.device)
        cnt = torch.empty(1, dtype=torch.int64, device=x.device)
        check(lib().gr4hip_schmitt_process(self._h, x.data_ptr(), n, buf.data_ptr(), cap, cnt.data_ptr(), _stream()), "SchmittTrigger.process")
        count = int(cnt.item())
        e = buf[:min(count, cap)]
        kf = e[:, 4]
        return SchmittEdges(count, e[:, 0:2].contiguous().view(torch.int64).reshape(-1), kf & capi.SCHMITT_KIND_MASK, e[:, 2].clone(),
                            e[:, 3].contiguous().view(torch.float32), e[:, 5].clone(), kf & ~capi.SCHMITT_KIND_MASK)


class SvdDenoiser(_Handle):
    """gr::filter::SvdDenoiser<T> (blocks/filter/.../SvdDenoiser.hpp:14-91) for T in {float32, float64, complex64, complex128} with the reference's setting
    names and defaults (the two thresholds default to eps of T's real type): Hankel-SVD low-rank denoising, processOne applied to every sample once, in order,
    whatever the chunking into calls (include/gr4hip.h "SVD denoiser", SVD_DENOISER.md).  set_params resets, as setParameters does (SvdFilter.hpp:221-229)."""
    _destroy = "gr4hip_svddenoise_destroy"
    _names = ("window_size", "hankel_rows", "max_rank", "relative_threshold", "absolute_threshold", "energy_fraction", "hop_fraction")
    _ints = ("window_size", "hankel_rows", "max_rank")
    _dtypes = {torch.float32: capi.F32, torch.float64: capi.F64, torch.complex64: capi.C32, torch.complex128: capi.C64}

    def __init__(self, dtype=torch.float32, **settings):
        super().__init__()
        if dtype not in self._dtypes:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SvdDenoiser", f"dtype {dtype} (float32, float64, complex64, complex128)")
        self.dtype = dtype
        p = capi.SvdDenoiseParams()
        check(lib().gr4hip_svddenoise_params_default(C.byref(p), self._dtypes[dtype]), "SvdDenoiser")
        self._p = self._params(p, settings)
        check(lib().gr4hip_svddenoise_create(C.byref(self._h), C.byref(self._p)), "SvdDenoiser")

    @staticmethod
    def windows_per_group() -> int:
        """windows per workgroup of the kernel"""
        return int(lib().gr4hip_svddenoise_windows_per_group())

    def _params(self, p, settings):
        for k, v in settings.items():
            if k not in self._names:
                raise TypeError(f"SvdDenoiser: unknown setting '{k}'")
            setattr(p, k, int(v) if k in self._ints else float(v))
        return p

    def __getattr__(self, name):
        if name in type(self)._names:
            return getattr(self.__dict__["_p"], name)
        raise AttributeError(name)

    def set_params(self, **settings):
        p = self._params(capi.SvdDenoiseParams.from_buffer_copy(self._p), settings)
        check(lib().gr4hip_svddenoise_set_params(self._h, C.byref(p)), "SvdDenoiser.set_params")
        self._p = p

    def reset(self):
        check(lib().gr4hip_svddenoise_reset(self._h), "SvdDenoiser.reset")

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "SvdDenoiser")
        if x.dim() != 1 or x.dtype != self.dtype:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SvdDenoiser", f"input must be a 1-D {self.dtype} tensor")
        n = x.numel()
        y = _out(out, n, self.dtype, x, "SvdDenoiser.process")
        check(lib().gr4hip_svddenoise_process(self._h, x.data_ptr(), n, y.data_ptr(), _stream()), "SvdDenoiser.process")
        return y[:n]

    def stats(self):
        """(windows started since the handle was made, windows among them that gave NaN: a non-finite sample, or sweeps that did not converge); waits for the
        stream of the handle's last call"""
        w, nc = C.c_ulonglong(0), C.c_ulonglong(0)
        check(lib().gr4hip_svddenoise_stats(self._h, C.byref(w), C.byref(nc)), "SvdDenoiser.stats")
        return int(w.value), int(nc.value)

    def sweeps(self) -> int:
        """Jacobi sweeps of all windows since the handle was made; waits as stats() does"""
        s = C.c_ulonglong(0)
        check(lib().gr4hip_svddenoise_sweeps(self._h, C.byref(s)), "SvdDenoiser.sweeps")
        return int(s.value)


_SAVGOL_DTYPES = {torch.float32: capi.F32, torch.float64: capi.F64}


def _savgol_dtype(dtype, who: str) -> int:
    if dtype not in _SAVGOL_DTYPES:
        raise capi.Gr4HipError(capi.INVALID_ARGUMENT, who, f"dtype {dtype} (float32, float64)")
    return _SAVGOL_DTYPES[dtype]


def design_savitzky_golay(dtype=torch.float32, window_size: int = 11, poly_order: int = 4, deriv_order: int = 0, delta: float = 1.0, alignment: str = "Centred"):
    """computeCoefficients<T> (algorithm/filter/SavitzkyGolay.hpp:93-151) through gr4hip_savgol_design (host code, no device): (coefficients as a numpy array of
    T, capi.SavgolInfo).  coeffs[k] belongs to the offset k - D; "Causal", or anything else = Centred."""
    did = _savgol_dtype(dtype, "design_savitzky_golay")
    c = np.empty(max(int(window_size), 1), _NP_DTYPE[did])
    info = capi.SavgolInfo()
    check(lib().gr4hip_savgol_design(did, int(window_size), int(poly_order), int(deriv_order), float(delta),
                                     capi.SAVGOL_CAUSAL if alignment == "Causal" else capi.SAVGOL_CENTRED, c.ctypes.data, C.byref(info)), "design_savitzky_golay")
    return c, info


class SavitzkyGolayFilter:
    """gr::filter::SavitzkyGolayFilter<T> (blocks/filter/.../SavitzkyGolayFilter.hpp:17-81) for T in {float32, float64}: the streaming filter
    y[n] = sum_k c[k] x[n - (W - 1) + k] over a history of zeros (SavitzkyGolay.hpp:226-233, BoundaryPolicy::Default), which is fir_filter with b[k] = c[W - 1 - k]:
    the library's design on its FIR handles (IEEE float32 kernels for float, the FP64 kernel for double).  set_params designs again and clears the history, as
    setParameters does (:253-260); delta = 1 / T(sample_rate) when sample_rate > 0, else 1 (:49-52)."""
    _names = ("window_size", "poly_order", "deriv_order", "sample_rate", "alignment")

    def __init__(self, dtype=torch.float32, window_size: int = 11, poly_order: int = 4, deriv_order: int = 0, sample_rate: float = 1.0, alignment: str = "Centred"):
        self._np = _NP_DTYPE[_savgol_dtype(dtype, "SavitzkyGolayFilter")]
        self.dtype = dtype
        self._s = dict(window_size=int(window_size), poly_order=int(poly_order), deriv_order=int(deriv_order), sample_rate=float(sample_rate), alignment=str(alignment))
        self._fir = None
        self._design()

    def _design(self):
        s = self._s
        rate = self._np(np.float32(s["sample_rate"]))  # the setting is a float (:40), cast to T (:49)
        delta = self._np(1) / rate if rate > 0 else self._np(1)
        self.coeffs, self.info = design_savitzky_golay(self.dtype, s["window_size"], s["poly_order"], s["deriv_order"], float(delta), s["alignment"])
        b = self.coeffs[::-1].copy()
        if self._fir is None:
            self._fir = fir_filter(b, self.dtype)
            if self.dtype == torch.float32:
                self._fir.set_algo(capi.FIR_EXACT_F32)
        else:
            self._fir.settings_changed(b)
            self._fir.reset()  # set_taps keeps the FIR history; the reference's setParameters clears it

    def __getattr__(self, name):
        if name in type(self)._names:
            return self.__dict__["_s"][name]
        raise AttributeError(name)

    def set_params(self, **settings):
        for k in settings:
            if k not in self._names:
                raise TypeError(f"SavitzkyGolayFilter: unknown setting '{k}'")
        old = dict(self._s)
        self._s.update({k: (str(v) if k == "alignment" else float(v) if k == "sample_rate" else int(v)) for k, v in settings.items()})
        try:
            self._design()
        except Exception:
            self._s = old
            raise

    def reset(self):
        self._fir.reset()

    def close(self):
        self._fir.close()

    def process_bulk(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._fir.process_bulk(x, out)


class SavitzkyGolayDataSetFilter(_Handle):
    """gr::filter::SavitzkyGolayDataSetFilter<T> (blocks/filter/.../SavitzkyGolayFilter.hpp:87-164) for T in {float32, float64}: zero-phase (forward-backward)
    Savitzky-Golay filtering, both passes in one launch (include/gr4hip.h "Savitzky-Golay", SAVITZKY_GOLAY.md).  process(x[batch, n]) filters every row on its own;
    the block itself filters the whole flat signal_values as one row.  boundary_policy: "Replicate", or anything else = Reflect (:126-128)."""
    _destroy = "gr4hip_savgol_zp_destroy"
    _names = ("window_size", "poly_order", "deriv_order", "boundary_policy")

    def __init__(self, dtype=torch.float32, window_size: int = 11, poly_order: int = 4, deriv_order: int = 0, boundary_policy: str = "Reflect"):
        super().__init__()
        self._did = _savgol_dtype(dtype, "SavitzkyGolayDataSetFilter")
        self.dtype = dtype
        self._s = dict(window_size=int(window_size), poly_order=int(poly_order), deriv_order=int(deriv_order), boundary_policy=str(boundary_policy))
        p = self._params(self._s)
        check(lib().gr4hip_savgol_zp_create(C.byref(self._h), C.byref(p)), "SavitzkyGolayDataSetFilter")

    @staticmethod
    def tile() -> int:
        """outputs per workgroup of the kernel: a row of at most this many samples is one workgroup's"""
        return int(lib().gr4hip_savgol_zp_tile())

    def _params(self, s):
        return capi.SavgolZpParams(self._did, s["window_size"], s["poly_order"], s["deriv_order"],
                                   capi.SAVGOL_REPLICATE if s["boundary_policy"] == "Replicate" else capi.SAVGOL_REFLECT)

    def __getattr__(self, name):
        if name in type(self)._names:
            return self.__dict__["_s"][name]
        raise AttributeError(name)

    def set_params(self, **settings):
        for k in settings:
            if k not in self._names:
                raise TypeError(f"SavitzkyGolayDataSetFilter: unknown setting '{k}'")
        s = dict(self._s)
        s.update({k: (str(v) if k == "boundary_policy" else int(v)) for k, v in settings.items()})
        p = self._params(s)
        check(lib().gr4hip_savgol_zp_set_params(self._h, C.byref(p)), "SavitzkyGolayDataSetFilter.set_params")
        self._s = s

    def coefficients(self):
        """(the W coefficients in T the kernel filters with, capi.SavgolInfo)"""
        info = capi.SavgolInfo()
        c = np.empty(max(self._s["window_size"], 1), _NP_DTYPE[self._did])
        check(lib().gr4hip_savgol_zp_coeffs(self._h, c.ctypes.data, C.byref(info)), "SavitzkyGolayDataSetFilter.coefficients")
        return c, info

    def process(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x: [n] or [batch, n], rows a stride apart (a column slice of a wider tensor is taken as it is, without a copy)"""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SavitzkyGolayDataSetFilter", "input must be a CUDA/HIP torch tensor (device-only path)")
        if x.dtype != self.dtype or x.dim() not in (1, 2):
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SavitzkyGolayDataSetFilter", f"input must be a 1-D or 2-D {self.dtype} tensor")
        x2 = x if x.dim() == 2 else x.unsqueeze(0)
        if x2.numel() and (x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1])):
            x2 = x2.contiguous()
        batch, n = x2.shape
        if out is None:
            y = torch.empty_like(x2) if x2.is_contiguous() else torch.empty_strided(x2.shape, x2.stride(), dtype=x2.dtype, device=x2.device)
        else:
            y = out if out.dim() == 2 else out.unsqueeze(0)
            if (not y.is_cuda or y.device != x2.device or y.dtype != self.dtype or y.shape != x2.shape or (n and y.stride(1) != 1)
                    or (batch > 1 and y.stride(0) != x2.stride(0))):
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SavitzkyGolayDataSetFilter.process", "out must be a device tensor of the input's dtype, shape and row stride")
        stride = x2.stride(0) if batch > 1 else max(n, 1)
        check(lib().gr4hip_savgol_zp_process(self._h, x2.data_ptr(), y.data_ptr(), n, batch, stride, _stream()), "SavitzkyGolayDataSetFilter.process")
        return y if x.dim() == 2 else y[0]


class SignalGenerator(_Handle):
    """gr::basic::SignalGenerator<T> (blocks/basic/.../SignalGenerator.hpp:25-87) as a device source for T in {float32, float64, complex64, int16}: sample n is what
    the n-th generateSample() of the reference's core returns, whatever the cutting into calls (include/gr4hip.h "Signal generator", SIGNAL_GENERATOR.md).
    `signal_type`: one of capi.SIGGEN_TYPES or its number.  configure is settingsChanged (noise re-seeded, phasor restarted, time keeps running); reset also
    zeroes the time."""
    _destroy = "gr4hip_siggen_destroy"
    _names = ("signal_type", "sample_rate", "frequency", "amplitude", "offset", "phase", "seed")
    _dtypes = {torch.float32: capi.F32, torch.float64: capi.F64, torch.complex64: capi.C32, torch.int16: capi.I16}

    def __init__(self, signal_type="Sin", dtype=torch.float32, sample_rate=1000., frequency=1., amplitude=1., offset=0., phase=0., seed=0):
        super().__init__()
        if dtype not in self._dtypes:
            raise capi.Gr4HipError(capi.UNSUPPORTED, "SignalGenerator", f"dtype {dtype} (float32, float64, complex64, int16)")
        self.dtype = dtype
        self._p = self._params(capi.SigGenParams(self._dtypes[dtype], 1, 1000., 1., 1., 0., 0., 0),
                               dict(signal_type=signal_type, sample_rate=sample_rate, frequency=frequency, amplitude=amplitude, offset=offset, phase=phase, seed=seed))
        check(lib().gr4hip_siggen_create(C.byref(self._h), C.byref(self._p)), "SignalGenerator")

    @staticmethod
    def run() -> int:
        """consecutive samples one lane generates"""
        return int(lib().gr4hip_siggen_run())

    @staticmethod
    def tile() -> int:
        """samples of one workgroup: where the generator's start states change hands"""
        return int(lib().gr4hip_siggen_tile())

    def _params(self, p, settings):
        for k, v in settings.items():
            if k not in self._names:
                raise TypeError(f"SignalGenerator: unknown setting '{k}'")
            if k == "signal_type":
                if isinstance(v, str):
                    if v not in capi.SIGGEN_TYPES:
                        raise ValueError(f"SignalGenerator: unknown signal type '{v}'")
                    v = capi.SIGGEN_TYPES.index(v)
                p.signal_type = int(v)
            elif k == "seed":
                p.seed = int(v) & 0xFFFFFFFFFFFFFFFF
            else:
                setattr(p, k, float(v))
        return p

    def __getattr__(self, name):
        if name in type(self)._names:
            v = getattr(self.__dict__["_p"], name)
            return capi.SIGGEN_TYPES[v] if name == "signal_type" else v
        raise AttributeError(name)

    def configure(self, **settings):
        p = self._params(capi.SigGenParams.from_buffer_copy(self._p), settings)
        check(lib().gr4hip_siggen_configure(self._h, C.byref(p)), "SignalGenerator.configure")
        self._p = p

    def reset(self):
        check(lib().gr4hip_siggen_reset(self._h), "SignalGenerator.reset")

    def generate_into(self, out: torch.Tensor) -> torch.Tensor:
        """the next out.numel() samples into `out` (a contiguous 1-D device tensor of the handle's dtype), on the current stream; returns without waiting"""
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dim() != 1 or out.dtype != self.dtype or not out.is_contiguous():
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "SignalGenerator", f"out must be a contiguous 1-D {self.dtype} device tensor")
        check(lib().gr4hip_siggen_process(self._h, out.data_ptr(), out.numel(), _stream()), "SignalGenerator.generate")
        return out

    def generate(self, n: int, device="cuda") -> torch.Tensor:
        return self.generate_into(torch.empty(int(n), dtype=self.dtype, device=device))


class Converter(_Handle):
    """The type-converter blocks of blocks/basic/.../ConverterBlocks.hpp:13-277 on the device (include/gr4hip.h "Type converters", CONVERTERS.md): one launch per
    call, every pointer with the alignment of its element type only.  `process_bulk` takes one tensor per input port and returns a tensor, or a tuple for the
    two-output kinds.  set_prologue / set_epilogue take a Merged program of the input / output dtype: a run of per-sample neighbours rides in this launch."""
    _destroy = "gr4hip_convert_destroy"

    def __init__(self, kind, in_dtype, out_dtype=None, scale=1.0):
        super().__init__()
        self.kind = capi.CONVERT_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        if in_dtype not in _DTYPE_ID:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Converter", f"dtype {in_dtype}")
        self._p = capi.ConvertParams()
        check(lib().gr4hip_convert_params_default(C.byref(self._p), self.kind, _DTYPE_ID[in_dtype]), "Converter")
        if out_dtype is not None:
            if out_dtype not in _DTYPE_ID:
                raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Converter", f"dtype {out_dtype}")
            self._p.out_dtype = _DTYPE_ID[out_dtype]
        self._p.scale = float(scale)
        check(lib().gr4hip_convert_create(C.byref(self._h), C.byref(self._p)), "Converter")
        self.in_dtype, self.out_dtype = in_dtype, _TORCH_DTYPE[self._p.out_dtype]
        n_in, n_out, ic, oc = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(lib().gr4hip_convert_ports(self._h, C.byref(n_in), C.byref(n_out), C.byref(ic), C.byref(oc)), "Converter.ports")
        self.n_inputs, self.n_outputs, self.in_chunk, self.out_chunk = n_in.value, n_out.value, ic.value, oc.value

    def tile(self) -> int:
        """items one workgroup of the aligned body converts"""
        return int(lib().gr4hip_convert_tile(C.byref(self._p)))

    @property
    def scale(self) -> float:
        return self._p.scale

    def set_scale(self, scale):
        check(lib().gr4hip_convert_set_scale(self._h, float(scale)), "Converter.set_scale")
        self._p.scale = float(scale)

    def reset(self):
        check(lib().gr4hip_convert_reset(self._h), "Converter.reset")

    def set_prologue(self, prog: Optional["Merged"]):
        check(lib().gr4hip_convert_set_prologue(self._h, prog._h if prog is not None else None), "Converter.set_prologue")

    def set_epilogue(self, prog: Optional["Merged"]):
        check(lib().gr4hip_convert_set_epilogue(self._h, prog._h if prog is not None else None), "Converter.set_epilogue")

    def process_bulk(self, *inputs: torch.Tensor, out=None, connected: Optional[Sequence[bool]] = None):
        """`out`: a tensor (or one per output port) to write into; `connected`: False for an output port left unconnected (its entry of the result is None)"""
        if len(inputs) != self.n_inputs:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Converter", f"{self.n_inputs} input port(s), got {len(inputs)}")
        ins = [_dev(x, "Converter") for x in inputs]
        if any(x.dtype != self.in_dtype or x.numel() != ins[0].numel() for x in ins):
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Converter", f"every input must be {self.in_dtype} and of one length")
        n_in = ins[0].numel()
        if n_in % self.in_chunk:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Converter", f"the input comes in chunks of {self.in_chunk} (got {n_in})")
        n_out = n_in // self.in_chunk * self.out_chunk
        connected = [True] * self.n_outputs if connected is None else list(connected)
        given = [None] * self.n_outputs if out is None else [out] if isinstance(out, torch.Tensor) else list(out)
        if len(connected) != self.n_outputs or len(given) != self.n_outputs:
            raise capi.Gr4HipError(capi.INVALID_ARGUMENT, "Converter", f"{self.n_outputs} output port(s)")
        outs = [_out(given[q], n_out, self.out_dtype, ins[0], "Converter") if connected[q] else None for q in range(self.n_outputs)]
        pin = (C.c_void_p * self.n_inputs)(*[x.data_ptr() for x in ins])
        pout = (C.c_void_p * self.n_outputs)(*[o.data_ptr() if o is not None else None for o in outs])
        written = C.c_size_t(0)
        check(lib().gr4hip_convert_process(self._h, pin, pout, n_in, C.byref(written), _stream()), "Converter.process")
        assert written.value == n_out
        return outs[0] if self.n_outputs == 1 else tuple(outs)


class Convert(Converter):
    """Convert<T, R> (ConverterBlocks.hpp:15-33): static_cast<R>(input)"""

    def __init__(self, in_dtype, out_dtype):
        super().__init__("Convert", in_dtype, out_dtype)


class ScalingConvert(Converter):
    """ScalingConvert<T, R> (:37-59): static_cast<R>(input * scale), scale of type T"""

    def __init__(self, in_dtype, out_dtype, scale=1.0):
        super().__init__("ScalingConvert", in_dtype, out_dtype, scale)


class _OneType(Converter):
    def __init__(self, dtype):
        super().__init__(type(self).__name__, dtype)


class _TwoTypes(Converter):
    def __init__(self, in_dtype, out_dtype):
        super().__init__(type(self).__name__, in_dtype, out_dtype)


class Abs(_OneType):
    """Abs<T> (:63-81)"""


class Real(_OneType):
    """Real<T> (:100-111)"""


class Imag(_OneType):
    """Imag<T> (:85-96)"""


class Arg(_OneType):
    """Arg<T> (:115-126)"""


class RadiansToDegree(_OneType):
    """RadiansToDegree<T> (:130-143)"""


class DegreeToRadians(_OneType):
    """DegreeToRadians<T> (:147-160)"""


class ToRealImag(_OneType):
    """ToRealImag<T> (:164-178): process_bulk returns (real, imag)"""


class RealImagToComplex(_OneType):
    """RealImagToComplex<T> (:182-195): process_bulk(real, imag)"""


class ToMagPhase(_OneType):
    """ToMagPhase<T> (:199-213): process_bulk returns (mag, phase)"""


class MagPhaseToComplex(_OneType):
    """MagPhaseToComplex<T> (:217-231): process_bulk(mag, phase)"""


class ComplexToInterleaved(_TwoTypes):
    """ComplexToInterleaved<T, R> (:235-254): two output elements per input sample"""


class InterleavedToComplex(_TwoTypes):
    """InterleavedToComplex<T, R> (:258-277): one output sample per two input elements"""


def synth_c32(n: int, seed: int = 42, tone_frel: float = 0.1, tone_amp: float = 1.0, noise_amp: float = 1.0, device="cuda") -> torch.Tensor:
    out = torch.empty(n, dtype=torch.complex64, device=device)
    check(lib().gr4hip_synth_c32(out.data_ptr(), n, seed, tone_frel, tone_amp, noise_amp, _stream()), "synth_c32")
    return out


def synth_draws(n_draws: int, seed: int, group: int) -> torch.Tensor:
    """raw 64-bit draws of the generator behind 8-sample group `group` of a synth stream (int64 tensor holding the uint64 bit patterns)"""
    out = torch.empty(n_draws, dtype=torch.int64, device="cuda")
    check(lib().gr4hip_synth_draws(out.data_ptr(), n_draws, seed & (2 ** 64 - 1), group, _stream()), "synth_draws")
    return out


def synth_f32(n: int, seed: int = 42, tone_frel: float = 0.1, tone_amp: float = 1.0, noise_amp: float = 1.0, device="cuda") -> torch.Tensor:
    out = torch.empty(n, dtype=torch.float32, device=device)
    check(lib().gr4hip_synth_f32(out.data_ptr(), n, seed, tone_frel, tone_amp, noise_amp, _stream()), "synth_f32")
    return out
