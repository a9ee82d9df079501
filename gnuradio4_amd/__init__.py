"""gnuradio4_amd -- MI355X-native execution of the GNU Radio 4 filter / fourier / math hot path.

Host-side mirror (Python) of the reference's block interface for that path, on top of the C-ABI kernel library
libgr4hip.so (include/gr4hip.h).  torch is used only for device memory, streams and torch.distributed.
"""
from . import capi  # noqa: F401
from .blocks import (Abs, Arg, ComplexToInterleaved, Convert, Converter, DegreeToRadians, Imag, InterleavedToComplex, MagPhaseToComplex, RadiansToDegree, Real,  # noqa: F401
                     RealImagToComplex, ScalingConvert, ToMagPhase, ToRealImag)
from .blocks import (FFT, AdaptiveWeights, BasicDecimatingFilter, BasicFilter, Beamformer, Chain, CrossSpectrum, Decimator, FirBatched, FrequencyEstimatorFrequencyDomain, FrequencyEstimatorTimeDomain, IQDemodulator, InverseFFT,
                     Merged, PolyphaseFilterBank, PolyphaseSynthesisBank, PowerFactor, PowerMetrics, Rotator, SavitzkyGolayDataSetFilter, SavitzkyGolayFilter, SchmittEdges, SchmittTrigger, SignalGenerator, STFT, SpectrumIntegrator, SvdDenoiser, SystemUnbalance, complex_fir_filter, design_pfb, design_resampler_taps, design_savitzky_golay, fir_filter, fir_interpolator, iir_filter, rational_resampler,  # noqa: F401
                     math_const, math_nary, synth_c32, synth_draws, synth_f32)

__all__ = ["capi", "fir_filter", "fir_interpolator", "rational_resampler", "design_resampler_taps", "complex_fir_filter", "iir_filter", "BasicFilter", "BasicDecimatingFilter", "Decimator", "FirBatched", "FFT", "InverseFFT", "STFT", "PolyphaseFilterBank", "PolyphaseSynthesisBank", "design_pfb", "SpectrumIntegrator", "CrossSpectrum", "Beamformer", "AdaptiveWeights", "Chain", "Merged", "Rotator",
           "FrequencyEstimatorTimeDomain", "FrequencyEstimatorFrequencyDomain", "IQDemodulator", "PowerMetrics", "PowerFactor", "SystemUnbalance", "SchmittTrigger", "SchmittEdges", "SvdDenoiser", "SignalGenerator", "SavitzkyGolayFilter", "SavitzkyGolayDataSetFilter", "design_savitzky_golay",
           "Converter", "Convert", "ScalingConvert", "Abs", "Real", "Imag", "Arg", "RadiansToDegree", "DegreeToRadians", "ToRealImag", "RealImagToComplex", "ToMagPhase",
           "MagPhaseToComplex", "ComplexToInterleaved", "InterleavedToComplex",
           "math_const", "math_nary", "synth_c32", "synth_draws", "synth_f32"]
