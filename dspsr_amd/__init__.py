"""dspsr_amd: MI355X-native coherent-dedispersion + detection + fold engine (DSPSR hot path).

Importing the package loads libdspsr_amd.so (hand-written HIP for gfx950); it raises if the
library has not been built -- there is no CPU fallback."""
from ._lib import (lib, LIB_PATH, RAW_GENERIC, RAW_CASPSR, RAW_UWB16, RAW_MEERKAT, RAW_MEERKAT_SWAP, RAW_GUPPI, raw_at, guppi_at, is_guppi, GuppiLayout, COHERENCE, STOKES, INTENSITY, PPQQ,  # noqa: F401
                   TWOBIT_OFFSET_BINARY, TWOBIT_SIGN_MAGNITUDE, TWOBIT_TWOS_COMPLEMENT,
                   FUSED_AUTO, FUSED_ALWAYS, FUSED_NEVER)
from .engine import (BandpassEngine, bandpass_check_input, bandpass_check_shape, Communicator, Context, ConvolutionEngine, CyclicFoldEngine, cyclic_binplan, cyclic_lags_to_spectra, Dedispersion, DetectionEngine, DspsrAmdError, FilterbankEngine, FITSDigitizer, FoldEngine, PhaseLockedFilterbankEngine, plfb_check_shape, plfb_check_windows, Rescale, SampleDelay, SpectralKurtosisEngine, add_fpt, copy_data_fpt, dedispersion_sample_delays, detect_raw, fourth_moment, fscrunch_fpt, pscrunch_tfp, sigproc_digitize, sigproc_digitize_fpt, sk_limits, tscrunch_fpt, unpack_fpt, unpack_heaps_fpt, unpack_guppi_fpt, unpack_sigproc_fpt, twobit_block_bytes, twobit_check, twobit_unpack,  # noqa: F401
                     eight_bit_scale, fold_binplan, fold_binplan_runs, optimal_fft_length, tfp_filterbank)

__all__ = ["BandpassEngine", "bandpass_check_input", "bandpass_check_shape", "Communicator", "Context", "ConvolutionEngine", "CyclicFoldEngine", "cyclic_binplan", "cyclic_lags_to_spectra", "Dedispersion", "DetectionEngine", "DspsrAmdError", "FilterbankEngine", "FITSDigitizer", "FoldEngine", "PhaseLockedFilterbankEngine", "plfb_check_shape", "plfb_check_windows", "Rescale", "SampleDelay", "SpectralKurtosisEngine", "add_fpt", "copy_data_fpt", "dedispersion_sample_delays", "detect_raw", "fourth_moment", "fscrunch_fpt", "pscrunch_tfp", "sigproc_digitize", "sigproc_digitize_fpt", "sk_limits", "tscrunch_fpt", "unpack_fpt", "unpack_heaps_fpt", "unpack_guppi_fpt", "unpack_sigproc_fpt", "raw_at", "guppi_at", "is_guppi", "GuppiLayout", "twobit_block_bytes", "twobit_check", "twobit_unpack",
           "eight_bit_scale", "fold_binplan", "fold_binplan_runs", "optimal_fft_length", "tfp_filterbank", "lib", "LIB_PATH", "build_id"]


def build_id() -> str:
    """sha256 (12 hex digits) of the sources the loaded library was built from (csrc/Makefile: BUILD_ID)."""
    return lib.dspsr_amd_build_id().decode()
