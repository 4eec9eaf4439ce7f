"""ctypes binding of libdspsr_amd.so (the C-ABI declared in include/dspsr_amd.h).

The library is the product: there is NO fallback.  If it is missing or a symbol is absent the
import fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSPSR_AMD_LIB: alternative build of the same library (kernel experiments); there is still no fallback
LIB_PATH = os.environ.get("DSPSR_AMD_LIB") or os.path.join(_HERE, "libdspsr_amd.so")

OK, EINVAL, EHIP, ENOMEM, ESTATE = 0, -1, -2, -3, -4
H2D, D2H, D2D = 1, 2, 3
RAW_GENERIC, RAW_CASPSR, RAW_UWB16 = 0, 1, 2
RAW_MEERKAT, RAW_MEERKAT_SWAP = 3, 4      # heaps of 256 samples per (pol, chan) run; _SWAP: odd and even samples exchanged (MKBFRo)
RAW_TWOBIT = 5                            # two-bit real samples, whole excision windows (FilterbankEngine.set_twobit; not a C-ABI layout)
RAW_GUPPI = 6                             # GUPPI / PUPPI raw blocks, channel-major runs (FilterbankEngine.set_guppi; not a C-ABI layout)
HEAP_NSAMP = 256
HEAP_MACHINES = {"MKBF": RAW_MEERKAT, "MKBFRo": RAW_MEERKAT_SWAP}   # INSTRUMENT -> layout (kat/MeerKATUnpacker.C: sample_swap 2 for MKBFRo)
TWOBIT_OFFSET_BINARY, TWOBIT_SIGN_MAGNITUDE, TWOBIT_TWOS_COMPLEMENT = 0, 1, 2      # DSPSR_AMD_TWOBIT_*: TwoBitTable's code map
TWOBIT_MACHINES = {"CPSR2": TWOBIT_OFFSET_BINARY}   # INSTRUMENT -> table type (cpsr2/CPSR2TwoBitCorrection.C: matches, OffsetBinary)
COHERENCE, STOKES, INTENSITY, PPQQ = 0, 1, 2, 3
FUSED_AUTO, FUSED_ALWAYS, FUSED_NEVER = 0, 1, 2
REDUCE_SUM, REDUCE_GATHER = 0, 1
UNIQUE_ID_BYTES = 128


def raw_at(layout: int, first_sample: int) -> int:
    """DSPSR_AMD_RAW_AT: the layout word of a block of heaps whose first sample lies at `first_sample` of its first heap."""
    if layout not in (RAW_MEERKAT, RAW_MEERKAT_SWAP):
        raise ValueError("raw_at: layout %d is not a heap layout (RAW_MEERKAT, RAW_MEERKAT_SWAP)" % layout)
    if not 0 <= first_sample < HEAP_NSAMP:
        raise ValueError("raw_at: first_sample %d is not inside a heap of %d samples" % (first_sample, HEAP_NSAMP))
    return layout | (first_sample << 8)


def is_heaps(layout: int) -> bool:
    """The layout word names one of the heap layouts (with or without a first sample)."""
    return layout >= 0 and (layout & 0xff) in (RAW_MEERKAT, RAW_MEERKAT_SWAP)


def twobit_at(first_sample: int) -> int:
    """The layout word of a two-bit block whose first sample lies at `first_sample` of its first excision window (as raw_at for heaps;
    RAW_TWOBIT is a form of the Python engine alone: FilterbankEngine unpacks it and calls the float entry points)."""
    if first_sample < 0:
        raise ValueError("twobit_at: first_sample %d is negative" % first_sample)
    return RAW_TWOBIT | (first_sample << 8)


def is_twobit(layout: int) -> bool:
    return layout >= 0 and (layout & 0xff) == RAW_TWOBIT


def guppi_at(first_sample: int) -> int:
    """The layout word of a block of GUPPI raw blocks whose first sample lies at `first_sample` of the runs of its first block (as
    raw_at for heaps; RAW_GUPPI is a form of the Python engine alone: FilterbankEngine unpacks it and calls the float entry points)."""
    if first_sample < 0:
        raise ValueError("guppi_at: first_sample %d is negative" % first_sample)
    return RAW_GUPPI | (first_sample << 8)


def is_guppi(layout: int) -> bool:
    return layout >= 0 and (layout & 0xff) == RAW_GUPPI


def guppi_block_bytes(first_sample: int, nsamp: int, nchan: int, npol: int, block_nsamp: int, chan_stride: int, block_stride: int) -> int:
    """Bytes from the data section of the block that holds the first sample to the last kept sample of the last block's last run."""
    nblk = -(-(first_sample + nsamp) // block_nsamp)
    return (nblk - 1) * block_stride + (nchan - 1) * chan_stride + block_nsamp * 2 * npol if nsamp > 0 else 0


def heap_block_bytes(first_sample: int, nsamp: int, nchan: int, npol: int) -> int:
    """Bytes of the whole heaps that hold `nsamp` samples from `first_sample` of the first heap on."""
    return -(-(first_sample + nsamp) // HEAP_NSAMP) * npol * nchan * HEAP_NSAMP * 2


def raw_block_bytes(layout: int, nsamp: int, nchan: int, npol: int, ndim: int, first_sample: int = 0, geometry=None) -> int:
    """Bytes of an 8-bit block of `nsamp` samples in `layout` (a layout without its first sample).  Heaps: the whole heaps from
    `first_sample` of the first one on; GUPPI raw blocks of `geometry` = (block_nsamp, chan_stride, block_stride): from the data
    section that holds `first_sample` to the last kept sample of the last run."""
    if layout in (RAW_MEERKAT, RAW_MEERKAT_SWAP):
        return heap_block_bytes(first_sample, nsamp, nchan, npol)
    if layout == RAW_GUPPI:
        return guppi_block_bytes(first_sample, nsamp, nchan, npol, *geometry)
    if layout == RAW_CASPSR:
        # 4 samples of pol0 then 4 of pol1: the block must hold WHOLE 8-byte groups (its last samples' pol1 bytes lie up to 4 bytes
        # behind their pol0 bytes; CASPSRUnpacker.C:132-187 unpacks group by group)
        return ((nsamp + 3) // 4) * 8
    return nsamp * nchan * npol * ndim


class FilterbankConfig(C.Structure):
    _fields_ = [("nchan_subband", C.c_uint32), ("freq_res", C.c_uint32), ("nfilt_pos", C.c_uint32),
                ("nfilt_neg", C.c_uint32), ("input_nchan", C.c_uint32), ("npol", C.c_uint32),
                ("real_input", C.c_uint32), ("max_parts", C.c_uint32), ("force_four_pass", C.c_uint32),
                ("fused_fold", C.c_uint32), ("split_in_inverse", C.c_uint32)]


class GuppiLayout(C.Structure):
    _fields_ = [("nchan", C.c_uint32), ("npol", C.c_uint32), ("block_nsamp", C.c_uint32), ("first", C.c_uint32),
                ("chan_stride", C.c_uint64), ("block_stride", C.c_uint64)]


class TfpConfig(C.Structure):
    _fields_ = [("nchan", C.c_uint32), ("npol", C.c_uint32), ("pscrunch", C.c_uint32), ("tscrunch", C.c_uint32)]


class DedispersionConfig(C.Structure):
    _fields_ = [("centre_frequency", C.c_double), ("bandwidth", C.c_double), ("dispersion_measure", C.c_double),
                ("input_nchan", C.c_uint32), ("nchan", C.c_uint32), ("ndim", C.c_uint32),
                ("dual_sideband", C.c_int32), ("dc_centred", C.c_uint32), ("swap", C.c_uint32),
                ("freq_res", C.c_uint32), ("ndat_max", C.c_uint32), ("fractional_delay", C.c_uint32)]


class DedispersionInfo(C.Structure):
    _fields_ = [("impulse_pos", C.c_uint32), ("impulse_neg", C.c_uint32), ("minimum_ndat", C.c_uint32),
                ("ndat", C.c_uint32)]


_vp, _u32, _u64, _i, _f, _d, _sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float, C.c_double, C.c_size_t
_pp = C.POINTER(C.c_void_p)

# every symbol include/dspsr_amd.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "dspsr_amd_ctx_create": (_i, [_i, _vp, _pp]),
    "dspsr_amd_ctx_destroy": (None, [_vp]),
    "dspsr_amd_last_error": (C.c_char_p, [_vp]),
    "dspsr_amd_stream_sync": (_i, [_vp]),
    "dspsr_amd_version": (C.c_char_p, []),
    "dspsr_amd_build_id": (C.c_char_p, []),
    "dspsr_amd_malloc": (_i, [_vp, _sz, _pp]),
    "dspsr_amd_free": (_i, [_vp, _vp]),
    "dspsr_amd_zero": (_i, [_vp, _vp, _sz]),
    "dspsr_amd_copy": (_i, [_vp, _vp, _vp, _sz, _i]),
    "dspsr_amd_copy_fpt": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _u32, _u64]),
    "dspsr_amd_add_fpt": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _u32, _u64]),
    "dspsr_amd_filterbank_create": (_i, [_vp, C.POINTER(FilterbankConfig), _pp]),
    "dspsr_amd_filterbank_destroy": (None, [_vp]),
    "dspsr_amd_filterbank_set_kernel": (_i, [_vp, _vp, _u64]),
    "dspsr_amd_filterbank_set_response_matrix": (_i, [_vp, _vp, _u64]),
    "dspsr_amd_filterbank_response_ndim": (_i, [_vp]),
    "dspsr_amd_filterbank_sizes": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u32)]),
    "dspsr_amd_filterbank_perform": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _u64, _u64, _u64]),
    "dspsr_amd_filterbank_perform_raw": (_i, [_vp, _vp, _i, _f, _vp, _u64, _u64, _u64, _u64]),
    "dspsr_amd_filterbank_perform_detect": (_i, [_vp, _vp, _u64, _u64, _u64, _vp, _i, _f, _i, _u32, _vp, _u64, _u64,
                                                 _u64]),
    "dspsr_amd_filterbank_fold_is_fused": (_i, [_vp]),
    "dspsr_amd_filterbank_fold_is_fused_state": (_i, [_vp, _i]),
    "dspsr_amd_filterbank_npass": (_i, [_vp, _i]),
    "dspsr_amd_filterbank_presplit": (_i, [_vp]),
    "dspsr_amd_filterbank_takes_heaps": (_i, [_vp]),
    "dspsr_amd_filterbank_perform_fold": (_i, [_vp, _vp, _u64, _u64, _u64, _vp, _i, _f, _i, _vp, _u64]),
    "dspsr_amd_filterbank_perform_search": (_i, [_vp, _vp, _u64, _u64, _u64, _vp, _i, _f, _i, _u32, _vp, _u64, _u64, _vp,
                                                 C.POINTER(_u32), _u64, C.POINTER(_u64)]),
    "dspsr_amd_filterbank_search_is_fused": (_i, [_vp]),
    "dspsr_amd_filterbank_search_is_fused_state": (_i, [_vp, _i, _u32]),
    "dspsr_amd_tscrunch_fpt": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _u32, _u32, _u64, _u32, _vp, C.POINTER(_u32),
                                    C.POINTER(_u64)]),
    "dspsr_amd_fscrunch_fpt": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _u32, _u64, _u32]),
    "dspsr_amd_sample_delay_create": (_i, [_vp, _u32, _u32, _vp, _i, _pp]),
    "dspsr_amd_sample_delay_destroy": (None, [_vp]),
    "dspsr_amd_sample_delay_zero_delay": (C.c_int64, [_vp]),
    "dspsr_amd_sample_delay_total_delay": (_u64, [_vp]),
    "dspsr_amd_sample_delay_transform": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _u64, C.POINTER(_u64)]),
    "dspsr_amd_dedispersion_sample_delays": (_i, [_d, _d, _d, _u32, _d, _i, _u32, _i, _vp]),
    "dspsr_amd_pscrunch_tfp": (_i, [_vp, _vp, _vp, _u64, _u32, _u32]),
    "dspsr_amd_rescale_create": (_i, [_vp, _u32, _u32, _u64, _i, _pp]),
    "dspsr_amd_rescale_destroy": (None, [_vp]),
    "dspsr_amd_rescale_transform": (_i, [_vp, _vp, _vp, _u64]),
    "dspsr_amd_rescale_get": (_i, [_vp, _vp, _vp]),
    "dspsr_amd_rescale_pscrunch_digitize": (_i, [_vp, _vp, _u64, _i, _f, _i, _i, _vp]),
    "dspsr_amd_sigproc_digitize": (_i, [_vp, _vp, _u64, _u32, _u32, _i, _i, _d, _f, _i, _i, _vp]),
    "dspsr_amd_rescale_transform_fpt": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _u64]),
    "dspsr_amd_sigproc_digitize_fpt": (_i, [_vp, _vp, _u64, _u64, _u64, _u32, _u32, _i, _i, _d, _f, _i, _i, _vp]),
    "dspsr_amd_rescale_digitize_fpt": (_i, [_vp, _vp, _u64, _u64, _u64, _i, _f, _i, _i, _vp]),
    "dspsr_amd_fits_digitizer_create": (_i, [_vp, _u32, _u32, _i, _u32, _u32, _i, _i, _i, _pp]),
    "dspsr_amd_fits_digitizer_destroy": (None, [_vp]),
    "dspsr_amd_fits_digitizer_pack": (_i, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "dspsr_amd_detect_polarimetry": (_i, [_vp, _i, _u32, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _u64]),
    "dspsr_amd_detect_square_law": (_i, [_vp, _i, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _u32, _u64]),
    "dspsr_amd_unpack_fpt": (_i, [_vp, _vp, _f, _u32, _u32, _u32, _u64, _vp, _u64, _u64]),
    "dspsr_amd_unpack_heaps_fpt": (_i, [_vp, _vp, _i, _f, _u32, _u32, _u64, _vp, _u64, _u64]),
    "dspsr_amd_unpack_guppi_fpt": (_i, [_vp, _vp, C.POINTER(GuppiLayout), _u64, _vp, _u64, _u64]),
    "dspsr_amd_unpack_sigproc_fpt": (_i, [_vp, _vp, _u32, _u32, _u32, _u64, _vp, _u64, _u64]),
    "dspsr_amd_twobit_check": (_i, [_u64, _i, _u32, _u32, _u32, _u64, _u32, _u32, _u64, _u64, C.c_char_p, _sz]),
    "dspsr_amd_twobit_unpack": (_i, [_vp, _vp, _i, _u32, _u32, _u32, _u64, _u32, _u32, _vp, _vp, _u64, _vp, _vp]),
    "dspsr_amd_detect_raw": (_i, [_vp, _vp, _f, _u32, _u32, _u64, _i, _u32, _vp, _u64, _u64, _vp, C.POINTER(_u32), C.POINTER(_u64)]),
    "dspsr_amd_tfp_filterbank": (_i, [_vp, C.POINTER(TfpConfig), _vp, _i, _f, _vp, _u64]),
    "dspsr_amd_fold_create": (_i, [_vp, _pp]),
    "dspsr_amd_fold_destroy": (None, [_vp]),
    "dspsr_amd_fold_set_shape": (_i, [_vp, _u32, _u32, _u32, _u32]),
    "dspsr_amd_fold_bind_profile": (_i, [_vp, _vp, _u64, _u32, _u32, _u32, _u32]),
    "dspsr_amd_fold_set_nbin": (_i, [_vp, _u32]),
    "dspsr_amd_fold_set_ndat": (_i, [_vp, _u64, _u64]),
    "dspsr_amd_fold_set_bin": (_i, [_vp, _u64, _d, _d]),
    "dspsr_amd_fold_set_bins": (_i, [_vp, _d, _d, _u64, _u64, _vp, C.POINTER(_u64)]),
    "dspsr_amd_fold_set_bins_weighted": (_i, [_vp, _d, _d, _u64, _u64, _vp, _u64, _u64, _u64, _vp, C.POINTER(_u64)]),
    "dspsr_amd_fold_fold": (_i, [_vp, _vp, _u64, _u64]),
    "dspsr_amd_fold_fold_many": (_i, [C.POINTER(_vp), _u32, _vp, _u64, _u64, C.POINTER(_u32)]),
    "dspsr_amd_fold_fold_zeroed": (_i, [_vp, _vp, _u64, _u64, _vp]),
    "dspsr_amd_fold_profiles_dev": (_vp, [_vp]),
    "dspsr_amd_fold_get_ndat_folded": (_u64, [_vp]),
    "dspsr_amd_fold_zero": (_i, [_vp]),
    "dspsr_amd_fold_synch": (_i, [_vp, _vp]),
    "dspsr_amd_fourth_moment": (_i, [_vp, _vp, _u64, _vp, _u64, _u32, _u64]),
    "dspsr_amd_fold_fold_moments": (_i, [_vp, _vp, _u64]),
    "dspsr_amd_cyclic_fold_create": (_i, [_vp, _pp]),
    "dspsr_amd_cyclic_fold_destroy": (None, [_vp]),
    "dspsr_amd_cyclic_fold_set_shape": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32]),
    "dspsr_amd_cyclic_fold_set_ndat": (_i, [_vp, _u64, _u64]),
    "dspsr_amd_cyclic_fold_set_bin": (_i, [_vp, _u64, _d, _d]),
    "dspsr_amd_cyclic_fold_set_bins": (_i, [_vp, _d, _d, _u64, _u64, _vp, C.POINTER(_u64)]),
    "dspsr_amd_cyclic_fold_fold": (_i, [_vp, _vp, _u64, _u64]),
    "dspsr_amd_cyclic_fold_zero": (_i, [_vp]),
    "dspsr_amd_cyclic_fold_lagdata_dev": (_vp, [_vp]),
    "dspsr_amd_cyclic_fold_synch_lags": (_i, [_vp, _vp]),
    "dspsr_amd_plfb_check_shape": (_i, [_u32, _u32, _u32, _u32, _u32, _u32, C.c_char_p, _sz]),
    "dspsr_amd_plfb_check_windows": (_i, [_u32, _u32, _u32, _u32, _u32, _u64, _u64, _u64, _u64, _u64, _vp, _vp, C.c_char_p, _sz]),
    "dspsr_amd_plfb_create": (_i, [_vp, _pp]),
    "dspsr_amd_plfb_destroy": (None, [_vp]),
    "dspsr_amd_plfb_set_shape": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32]),
    "dspsr_amd_plfb_accumulate": (_i, [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _vp]),
    "dspsr_amd_plfb_zero": (_i, [_vp]),
    "dspsr_amd_plfb_profile_dev": (_vp, [_vp]),
    "dspsr_amd_plfb_synch": (_i, [_vp, _vp]),
    "dspsr_amd_bandpass_check_shape": (_i, [_u32, _u32, _u32, _u32, _u32, C.c_char_p, _sz]),
    "dspsr_amd_bandpass_check_input": (_i, [_u32, _u32, _u32, _u32, _i, _u64, _u64, _u64, _u64, C.POINTER(_u32), C.POINTER(_u32),
                                            C.POINTER(_u32), C.c_char_p, _sz]),
    "dspsr_amd_bandpass_create": (_i, [_vp, _pp]),
    "dspsr_amd_bandpass_destroy": (None, [_vp]),
    "dspsr_amd_bandpass_set_shape": (_i, [_vp, _u32, _u32, _u32, _u32, _u32]),
    "dspsr_amd_bandpass_accumulate": (_i, [_vp, _vp, _u64, _u64, _u64]),
    "dspsr_amd_bandpass_accumulate_raw": (_i, [_vp, _vp, _i, _f, _u64]),
    "dspsr_amd_bandpass_zero": (_i, [_vp]),
    "dspsr_amd_bandpass_pass_dev": (_vp, [_vp]),
    "dspsr_amd_bandpass_synch": (_i, [_vp, _vp, C.POINTER(_d)]),
    "dspsr_amd_sk_limits": (_i, [_u32, _u32, C.POINTER(_f), C.POINTER(_f)]),
    "dspsr_amd_sk_create": (_i, [_vp, _pp]),
    "dspsr_amd_sk_destroy": (None, [_vp]),
    "dspsr_amd_sk_set_shape": (_i, [_vp, _u32, _u32, _u32]),
    "dspsr_amd_sk_set_options": (_i, [_vp, _u32, _u32, _u32, _i, _i, _i]),
    "dspsr_amd_sk_compute": (_i, [_vp, _vp, _u64, _u64, _u64]),
    "dspsr_amd_sk_reset_mask": (_i, [_vp]),
    "dspsr_amd_sk_detect_tscr": (_i, [_vp, _f, _f]),
    "dspsr_amd_sk_detect_skfb": (_i, [_vp, _f, _f]),
    "dspsr_amd_sk_detect_fscr": (_i, [_vp]),
    "dspsr_amd_sk_count_zapped": (_i, [_vp]),
    "dspsr_amd_sk_mask": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64]),
    "dspsr_amd_sk_transform": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _u64]),
    "dspsr_amd_sk_npart": (_u64, [_vp]),
    "dspsr_amd_sk_estimates_dev": (_vp, [_vp]),
    "dspsr_amd_sk_estimates_tscr_dev": (_vp, [_vp]),
    "dspsr_amd_sk_zapmask_dev": (_vp, [_vp]),
    "dspsr_amd_sk_get_statistics": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "dspsr_amd_sk_reset_count": (_i, [_vp]),
    "dspsr_amd_comm_set_library": (_i, [C.c_char_p]),
    "dspsr_amd_comm_unique_id": (_i, [_vp]),
    "dspsr_amd_comm_create": (_i, [_vp, _i, _i, _vp, _pp]),
    "dspsr_amd_comm_destroy": (None, [_vp]),
    "dspsr_amd_comm_rank": (_i, [_vp]),
    "dspsr_amd_comm_size": (_i, [_vp]),
    "dspsr_amd_reduce_profiles_start": (_i, [_vp, _i, _i, _vp, _u64, _u64, _u64, _vp, _u32, _d, _u64, _i]),
    "dspsr_amd_reduce_profiles_result": (_vp, [_vp, C.POINTER(_u64)]),
    "dspsr_amd_reduce_profiles_finish": (_i, [_vp, _vp, _vp, C.POINTER(_d), C.POINTER(_u64), C.POINTER(_i)]),
    "dspsr_amd_dedispersion_prepare": (_i, [C.POINTER(DedispersionConfig), C.POINTER(DedispersionInfo), C.c_char_p,
                                            _sz]),
    "dspsr_amd_dedispersion_build": (_i, [C.POINTER(DedispersionConfig), _u32, _vp]),
    "dspsr_amd_optimal_fft_length": (_u64, [_u64, _u64]),
    "dspsr_amd_eight_bit_scale": (_d, [_d]),
    "dspsr_amd_fold_binplan": (_i, [_d, _d, _u32, _u64, _vp, _vp]),
    "dspsr_amd_fold_binplan_runs": (_i, [_d, _d, _u32, _u64, _vp, _vp, _vp, _u64, _vp, _vp]),
    "dspsr_amd_cyclic_binplan": (_i, [_d, _d, _u32, _u64, _vp, _vp, _vp]),
    "dspsr_amd_cyclic_lags_to_spectra": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _vp]),
    "dspsr_amd_rfi_mask_calculate": (_i, [_vp, _vp, _u32, _u32, _i, _vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "dspsr_amd_rfi_mask_calculate_log": (_i, [_vp, _vp, _u32, _u32, _i, _vp, C.POINTER(_u32), C.POINTER(_u32), _vp, _u32]),
    "dspsr_amd_rfi_mask_expand": (_i, [_vp, _u32, _u64, _vp]),
    "dspsr_amd_response_multiply": (_i, [_vp, _vp, _u64]),
}


def load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "dspsr_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process.  torch ships its own libamdhip64.so.7 / libhsa-runtime64 and the Python host side
    # shares streams and device memory with it, so torch's copy must be the one the dynamic linker binds: import torch
    # BEFORE the library (loading libdspsr_amd.so first binds /opt/rocm's runtime, and the context then finds no device
    # once torch has initialised its own).  A C/C++ host such as DSPSR has no torch in the process and links /opt/rocm.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


lib = load()
