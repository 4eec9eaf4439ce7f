"""Host-side mirror of the reference's Engine plug-in interfaces, over the C-ABI.

Names, argument meaning and error behaviour follow the reference classes:
  dsp::Filterbank::Engine  (Signal/General/dsp/FilterbankEngine.h:15-44): setup / perform / finish
  dsp::Detection::Engine   (Signal/General/dsp/Detection.h:98-106): polarimetry / square_law
  dsp::Fold::Engine        (Signal/Pulsar/dsp/Fold.h:249-312): set_nbin / set_ndat / set_bin / fold / synch / zero
  dsp::Dedispersion        (Signal/General/Dedispersion.C): prepare / build / match (host side)
Errors the reference throws as `Error` surface as DspsrAmdError with the same message text.

torch is used only to own device memory and streams; every computation goes through
libdspsr_amd.so (hand-written HIP).  TimeSeries are torch tensors in FPT order:
  voltages   float32 [nchan][npol][ndat*ndim]
  detected   float32 [nchan][npol_out][ndat*ndim_out]
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import lib


class DspsrAmdError(RuntimeError):
    """Counterpart of the reference's `Error` exception."""


def _check(ctx_handle, code, where):
    if code != 0:
        msg = lib.dspsr_amd_last_error(ctx_handle).decode() if ctx_handle else ""
        raise DspsrAmdError("%s failed (%d): %s" % (where, code, msg))


def _host_check(fn, *args):
    """One of the C-ABI's device-free check functions: its refusal, with the library's text, as DspsrAmdError."""
    msg = C.create_string_buffer(400)
    if fn(*args, msg, len(msg)) != _lib.OK:
        raise DspsrAmdError(msg.value.decode())


class _Owned:
    """An object the C-ABI makes with <_abi>_create(ctx, ..., &handle) and ends with <_abi>_destroy(handle); dead once its context
    is closed (a context closed first has already taken its device objects with it)."""

    _abi = None

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.handle = None

    def _create(self, *args):
        h = C.c_void_p()
        name = self._abi + "_create"
        _check(self.ctx.handle, getattr(lib, name)(self.ctx.handle, *args, C.byref(h)), name)
        self.handle = h

    def close(self):
        if self.handle and self.ctx.handle:
            getattr(lib, self._abi + "_destroy")(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One per pipeline thread/GPU, bound to one HIP stream (SingleThread.C:213-290)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        h = C.c_void_p()
        # stream: a hipStream_t handle as int (0 = the default stream torch uses), None = context-owned stream
        sp = C.c_void_p(-1 & (2 ** 64 - 1)) if stream is None else C.c_void_p(int(stream))
        code = lib.dspsr_amd_ctx_create(int(device), sp, C.byref(h))
        if code != 0:
            raise DspsrAmdError("dspsr_amd_ctx_create(device=%d) failed (%d): no usable HIP device" % (device, code))
        self.handle = h
        self.device = device

    def synchronize(self):
        _check(self.handle, lib.dspsr_amd_stream_sync(self.handle), "dspsr_amd_stream_sync")

    def close(self):
        if self.handle:
            lib.dspsr_amd_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fold_binplan_runs(phi: float, phase_per_sample: float, nbin: int, ndat: int, cap: int = 0):
    """The plan of fold_binplan as runs (first sample, bin, samples), found run by run (csrc/host_prep.cpp fold_plan_run); hits[nbin]."""
    cap = cap or max(1, ndat)
    off, rb, rh = np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint64)
    hits = np.zeros(nbin, dtype=np.uint32)
    n = C.c_uint64()
    code = lib.dspsr_amd_fold_binplan_runs(phi, phase_per_sample, nbin, ndat, off.ctypes.data_as(C.c_void_p), rb.ctypes.data_as(C.c_void_p),
                                           rh.ctypes.data_as(C.c_void_p), cap, C.byref(n), hits.ctypes.data_as(C.c_void_p))
    if code != 0:
        raise DspsrAmdError("dspsr_amd_fold_binplan_runs failed (%d)" % code)
    k = min(n.value, cap)
    return off[:k].copy(), rb[:k].copy(), rh[:k].copy(), hits, n.value


# ----------------------------------------------------------------------------------------------
# host-side preparation
# ----------------------------------------------------------------------------------------------

JA98_SPACING_8BIT = 0.02957   # JenetAnderson98::get_optimal_spacing(8) (PSRCHIVE, ext)


def eight_bit_scale(spacing: float = JA98_SPACING_8BIT) -> float:
    return float(np.float32(lib.dspsr_amd_eight_bit_scale(spacing)))


def optimal_fft_length(nbadperfft: int, nfft_max: int = 0) -> int:
    n = lib.dspsr_amd_optimal_fft_length(nbadperfft, nfft_max)
    return -1 if n == 2 ** 64 - 1 else int(n)


class Dedispersion:
    """dsp::Dedispersion: smearing -> impulse_pos/neg, frequency resolution, chirp (host, double->float)."""

    def __init__(self, centre_frequency, bandwidth, dispersion_measure, input_nchan=1, ndim=1,
                 dual_sideband=-1, dc_centred=False, swap=False, fractional_delay=False):
        self.cfg = _lib.DedispersionConfig(centre_frequency, bandwidth, dispersion_measure, input_nchan, input_nchan,
                                           ndim, dual_sideband, int(dc_centred), int(swap), 0, 0, int(fractional_delay))
        self.impulse_pos = self.impulse_neg = self.ndat = self.minimum_ndat = 0
        self.nchan = input_nchan
        self.kernel = None

    def set_frequency_resolution(self, nfft: int):
        self.cfg.freq_res = int(nfft)

    def set_maximum_ndat(self, n: int):
        self.cfg.ndat_max = int(n)

    def match(self, nchan: int):
        """Dedispersion::match(input, channels): prepare + build + Response::match ordering."""
        self.cfg.nchan = int(nchan)
        self.nchan = int(nchan)
        info = _lib.DedispersionInfo()
        err = C.create_string_buffer(256)
        code = lib.dspsr_amd_dedispersion_prepare(C.byref(self.cfg), C.byref(info), err, 256)
        if code != 0:
            raise DspsrAmdError(err.value.decode() or "dspsr_amd_dedispersion_prepare failed (%d)" % code)
        self.impulse_pos, self.impulse_neg = info.impulse_pos, info.impulse_neg
        self.minimum_ndat, self.ndat = info.minimum_ndat, info.ndat
        k = np.empty(self.nchan * self.ndat, dtype=np.complex64)
        code = lib.dspsr_amd_dedispersion_build(C.byref(self.cfg), self.ndat, k.ctypes.data_as(C.c_void_p))
        if code != 0:
            raise DspsrAmdError("dspsr_amd_dedispersion_build failed (%d)" % code)
        self.kernel = k
        return self


def fold_binplan(phi: float, phase_per_sample: float, nbin: int, ndat: int):
    plan = np.empty(ndat, dtype=np.uint32)
    hits = np.zeros(nbin, dtype=np.uint32)
    code = lib.dspsr_amd_fold_binplan(phi, phase_per_sample, nbin, ndat, plan.ctypes.data_as(C.c_void_p),
                                      hits.ctypes.data_as(C.c_void_p))
    if code != 0:
        raise DspsrAmdError("dspsr_amd_fold_binplan failed (%d)" % code)
    return plan, hits


# ----------------------------------------------------------------------------------------------
# engines
# ----------------------------------------------------------------------------------------------

def _strides3(t):
    """(chan_stride, pol_stride) in elements of a [nchan][npol][n] tensor with contiguous last dim."""
    assert t.dim() == 3 and t.stride(2) == 1, "TimeSeries rows must be contiguous"
    return t.stride(0), t.stride(1)


class FilterbankEngine(_Owned):
    """dsp::Filterbank::Engine.  setup() takes what CUDA::FilterbankEngine::setup reads from the
    Filterbank (FilterbankCUDA.cu:73-168)."""

    _abi = "dspsr_amd_filterbank"

    def setup(self, nchan_subband, freq_res, nfilt_pos, nfilt_neg, input_nchan=1, npol=2, real_input=True,
              kernel: np.ndarray | None = None, max_parts: int = 1, force_four_pass: bool | int = False,
              fused_fold: int = _lib.FUSED_AUTO, split_in_inverse: bool = False, response_matrix: np.ndarray | None = None,
              fuse_heaps: bool = True):
        """force_four_pass: False / 0 = passes chosen from the geometry, True / 1 = two-pass inverse everywhere, 2 = never the
        two-pass path of short responses (dspsr_amd_filterbank_config::force_four_pass).
        split_in_inverse: True keeps the Hermitian split of real dual-polarisation input in the inverse pass
        (dspsr_amd_filterbank_config::split_in_inverse); see presplit().
        response_matrix: float32 [nchan_subband * freq_res][8], one Jones matrix per bin as f11, f21, f22, f12 (`dspsr -pac`,
        dspsr_amd_filterbank_set_response_matrix); mutually exclusive with kernel.  When the library refuses it the object
        stays created, without a response: set_kernel() may still be called.
        fuse_heaps: False keeps blocks of MeerKAT heaps (RAW_MEERKAT / RAW_MEERKAT_SWAP) off the one-pass kernel's own loader even
        where the object has one (takes_heaps()): the engine unpacks them and hands float rows over, as it does for every other
        object (tests and comparison runs; the same numbers bit for bit)."""
        if kernel is not None and response_matrix is not None:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine.setup: kernel and response_matrix are mutually exclusive")
        self.close()
        cfg = _lib.FilterbankConfig(nchan_subband, freq_res, nfilt_pos, nfilt_neg, input_nchan, npol,
                                    1 if real_input else 0, max_parts, int(force_four_pass), fused_fold,
                                    1 if split_in_inverse else 0)
        self._create(C.byref(cfg))
        h = self.handle
        self.cfg = cfg
        self.max_parts = max(1, int(max_parts))
        self.fuse_heaps = bool(fuse_heaps)
        self._heap_rows = None      # float rows of an unpacked block of heaps: allocated by the first call that needs them
        self._twobit = None         # set_twobit: how a RAW_TWOBIT block is unpacked
        self._guppi = None          # set_guppi: (block_nsamp, chan_stride, block_stride) of a RAW_GUPPI block
        self._guppi_rows = None
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        lib.dspsr_amd_filterbank_sizes(h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        self.nsamp_fft, self.nsamp_overlap, self.nsamp_step, self.nkeep = a.value, b.value, c.value, d.value
        if response_matrix is not None:
            self.set_response_matrix(response_matrix)
        else:
            self.set_kernel(kernel)
        return self

    def set_kernel(self, kernel: np.ndarray | None):
        """The scalar response (complex64, input_nchan * nchan_subband * freq_res bins), or None for no response; replaces a
        matrix response."""
        if kernel is not None:
            k = np.ascontiguousarray(kernel, dtype=np.complex64)
            _check(self.ctx.handle, lib.dspsr_amd_filterbank_set_kernel(self.handle, k.ctypes.data_as(C.c_void_p), k.size),
                   "dspsr_amd_filterbank_set_kernel")
        else:
            _check(self.ctx.handle, lib.dspsr_amd_filterbank_set_kernel(self.handle, None, 0), "dspsr_amd_filterbank_set_kernel")

    def set_response_matrix(self, response_matrix: np.ndarray):
        """One Jones matrix per bin, float32 [nchan_subband * freq_res][8] in the order f11, f21, f22, f12 (Response.C:614-640);
        replaces a scalar response.  Refused (DspsrAmdError naming the limit) for npol 1, several input channels, freq_res 1 or
        above 8192, nchan_subband 1, odd factors, force_four_pass = 1 and a wrong number of matrices."""
        m = np.ascontiguousarray(response_matrix, dtype=np.float32)
        if m.ndim != 2 or m.shape[1] != 8:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine.set_response_matrix: the response must be float32 [nmatrix][8]")
        _check(self.ctx.handle, lib.dspsr_amd_filterbank_set_response_matrix(self.handle, m.ctypes.data_as(C.c_void_p), m.shape[0]),
               "dspsr_amd_filterbank_set_response_matrix")

    def response_ndim(self) -> int:
        """Response::get_ndim of what the object holds: 0 none, 2 complex (kernel), 8 Jones (response_matrix)."""
        return int(lib.dspsr_amd_filterbank_response_ndim(self.handle))

    def _need(self, what, have, need):
        if have < need:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine: %s holds %d elements per row, %d needed" % (what, have, need))

    def _raw_bytes(self, npart, layout=_lib.RAW_GENERIC):
        """bytes of a call of `npart` parts whose layout word (the call's first sample inside it) is `layout`"""
        c = self.cfg
        return _lib.raw_block_bytes(layout & 0xff if layout >= 0 else layout, npart * self.nsamp_step + self.nsamp_overlap, c.input_nchan, c.npol,
                                    1 if c.real_input else 2, layout >> 8, self._guppi_geometry() if _lib.is_guppi(layout) else None)

    def takes_heaps(self) -> bool:
        """True: the raw entry points read a block of MeerKAT heaps inside their one tile pass (dspsr_amd_filterbank_takes_heaps)."""
        return bool(lib.dspsr_amd_filterbank_takes_heaps(self.handle))

    def _unpacked_heaps(self, raw, layout, scale, npart):
        """A block of heaps this object does not read itself (or fuse_heaps=False), unpacked into float rows owned by the engine:
        (rows [input_nchan][npol][2 * nsamp], in_step), or None when the block goes to the library as it is.  The rows are
        allocated on first use for max_parts parts (a longer call allocates again).  A RAW_TWOBIT block (set_twobit) takes the same
        way through unpack_twobit; its weights stay in self.twobit_weights.  A RAW_GUPPI block (set_guppi) is unpacked by
        unpack_guppi_fpt into rows of its own, allocated the same way; `scale` is IGNORED for it: the format's value is float(int8)
        (GUPPIUnpacker.C:74-80)."""
        if raw is not None and _lib.is_twobit(layout):
            return self.unpack_twobit(raw, layout >> 8, npart)[:2]
        if raw is not None and _lib.is_guppi(layout):
            return self.unpack_guppi(raw, layout >> 8, npart)
        if raw is None or not _lib.is_heaps(layout) or (self.fuse_heaps and self.takes_heaps()):
            return None
        import torch
        c = self.cfg
        if c.real_input:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine: MeerKAT heaps are complex samples; the object was set up for real input")
        parts = max(npart, self.max_parts)
        need = 2 * (parts * self.nsamp_step + self.nsamp_overlap)
        if self._heap_rows is None or self._heap_rows.shape[2] < need or self._heap_rows.device != raw.device:
            self._heap_rows = torch.empty((c.input_nchan, c.npol, need), dtype=torch.float32, device=raw.device)
        if npart:
            self._need("raw block", raw.numel(), self._raw_bytes(npart, layout))
            unpack_heaps_fpt(self.ctx, raw, self._heap_rows, c.input_nchan, c.npol, layout, scale,
                             ndat=npart * self.nsamp_step + self.nsamp_overlap)
        return self._heap_rows, 2 * self.nsamp_step

    def set_guppi(self, block_nsamp, chan_stride, block_stride):
        """The GUPPI form of the raw entry points (layout RAW_GUPPI / guppi_at(first), next to the heap and two-bit forms): the
        geometry of the raw blocks a RAW_GUPPI block is made of -- kept samples per run, bytes from a run to the next one of the
        block, bytes from a block's data section to the next one's (dspsr_amd_guppi_layout).  nchan and npol are the object's
        input_nchan and npol; complex samples.  The `scale` of the raw entry points is ignored for this layout."""
        c = self.cfg
        if c.real_input:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine.set_guppi: GUPPI raw blocks are complex samples; the object was set up for real input")
        block_nsamp, chan_stride, block_stride = int(block_nsamp), int(chan_stride), int(block_stride)
        sb = 2 * c.npol
        if block_nsamp < 1 or chan_stride < block_nsamp * sb or chan_stride % sb or block_stride % sb:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine.set_guppi: block_nsamp=%d chan_stride=%d block_stride=%d contradict npol=%d "
                                "(chan_stride >= block_nsamp * 2 * npol, strides multiples of 2 * npol)" % (block_nsamp, chan_stride, block_stride, c.npol))
        if c.input_nchan > 1 and block_stride < (c.input_nchan - 1) * chan_stride + block_nsamp * sb:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine.set_guppi: block_stride=%d is shorter than the %d runs of input_nchan=%d "
                                "(chan_stride=%d)" % (block_stride, c.input_nchan, c.input_nchan, chan_stride))
        self._guppi = (block_nsamp, chan_stride, block_stride)
        self._guppi_rows = None

    def _guppi_geometry(self):
        if getattr(self, "_guppi", None) is None:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine: a RAW_GUPPI block needs set_guppi() first")
        return self._guppi

    def unpack_guppi(self, raw, first_sample, npart):
        """A RAW_GUPPI block (the data sections from the one that holds the call's first sample on, `first_sample` inside its runs)
        unpacked into float rows owned by the engine: (rows [input_nchan][npol][2 * nsamp], in_step = 2 * nsamp_step) for the float
        entry points.  The rows are allocated on first use for max_parts parts (a longer call allocates again), 16-byte aligned."""
        import torch
        geom = self._guppi_geometry()
        c = self.cfg
        parts = max(npart, self.max_parts)
        need = 2 * (parts * self.nsamp_step + self.nsamp_overlap)
        need += (-need) % 4                         # every row starts on a 16-byte boundary: float4 stores
        if self._guppi_rows is None or self._guppi_rows.shape[2] < need or self._guppi_rows.device != raw.device:
            self._guppi_rows = torch.empty((c.input_nchan, c.npol, need), dtype=torch.float32, device=raw.device)
        if npart:
            unpack_guppi_fpt(self.ctx, raw, self._guppi_rows, _lib.GuppiLayout(c.input_nchan, c.npol, geom[0], first_sample, geom[1], geom[2]),
                             npart * self.nsamp_step + self.nsamp_overlap)
        return self._guppi_rows, 2 * self.nsamp_step

    def set_twobit(self, nsample, nlow_min, nlow_max, levels, table_type=_lib.TWOBIT_OFFSET_BINARY):
        """The two-bit form of the raw entry points (layout RAW_TWOBIT, next to the heap form): how a two-bit block is unpacked --
        the excision window, its limits, the level table float32 [nlow_max - nlow_min + 1][2] (twobit.limits, twobit.levels) and
        the code table.  One input channel of real samples."""
        c = self.cfg
        if not c.real_input or c.input_nchan != 1:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine.set_twobit: two-bit input is one channel of real samples; the object was set "
                                "up for %s input of %d channels" % ("real" if c.real_input else "complex", c.input_nchan))
        twobit_check(0, table_type, c.npol, nsample, 0, 0, nlow_min, nlow_max)
        import torch
        lev = np.ascontiguousarray(levels, dtype=np.float32)
        if lev.shape != (nlow_max - nlow_min + 1, 2):
            raise DspsrAmdError("dspsr_amd.FilterbankEngine.set_twobit: the level table is %s, [%d][2] needed" % (lev.shape, nlow_max - nlow_min + 1))
        self._twobit = (int(nsample), int(nlow_min), int(nlow_max), torch.from_numpy(lev).to("cuda:%d" % self.ctx.device), int(table_type))
        self._twobit_rows = None
        self.twobit_weights = self.twobit_nlow = None      # per digitiser and window of the last block unpacked, before mask_weights

    def unpack_twobit(self, raw, first_sample, npart):
        """A RAW_TWOBIT block (the whole windows from the one that holds the call's first sample, `first_sample` inside it) unpacked
        into float rows owned by the engine: (rows [1][npol][nsamp], in_step, weights) for the float entry points -- weights: device
        int32 [npol][nwindow], 0 / 1 per digitiser (also self.twobit_weights; n_low in self.twobit_nlow).  The rows are allocated
        on first use for max_parts parts (a longer call allocates again), and placed so that the unpacker stores whole float4."""
        import torch
        if getattr(self, "_twobit", None) is None:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine: a RAW_TWOBIT block needs set_twobit() first")
        nsample, nlow_min, nlow_max, levels, table_type = self._twobit
        c = self.cfg
        nsamp = npart * self.nsamp_step + self.nsamp_overlap if npart else 0
        parts = max(npart, self.max_parts)
        need = (parts * self.nsamp_step + self.nsamp_overlap + 3) // 4 * 4 + 4
        if self._twobit_rows is None or self._twobit_rows.shape[1] < need or self._twobit_rows.device != raw.device:
            self._twobit_rows = torch.empty((c.npol, need), dtype=torch.float32, device=raw.device)
        nwindow = -(-(first_sample + nsamp) // nsample) if nsamp else 0
        self.twobit_weights = torch.empty((c.npol, nwindow), dtype=torch.int32, device=raw.device)
        self.twobit_nlow = torch.empty((c.npol, nwindow), dtype=torch.int32, device=raw.device)
        rows = self._twobit_rows[:, first_sample % 4:first_sample % 4 + nsamp]       # (row + n - first_sample: 16-byte aligned at words)
        if nsamp:
            twobit_unpack(self.ctx, raw, rows, levels, self.twobit_weights, nsample, nlow_min, nlow_max, table_type, first_sample, nsamp,
                          nlow=self.twobit_nlow)
        return rows.unsqueeze(0), self.nsamp_step, self.twobit_weights

    def perform(self, inp, out, npart, in_step, out_step):
        ics, ips = _strides3(inp)
        if npart:
            ndim = 1 if self.cfg.real_input else 2
            self._need("input", inp.shape[2], (npart - 1) * in_step + self.nsamp_fft * ndim)
            if out is not None:
                self._need("output", out.shape[2], (npart - 1) * out_step + 2 * self.nkeep)
        if out is not None:
            ocs, ops = _strides3(out)
            optr = out.data_ptr()
        else:
            ocs = ops = 0
            optr = None
        _check(self.ctx.handle,
               lib.dspsr_amd_filterbank_perform(self.handle, inp.data_ptr(), ics, ips, optr, ocs, ops, npart, in_step,
                                                out_step), "dspsr_amd_filterbank_perform")

    def perform_raw(self, raw, layout, scale, out, npart, out_step=None):
        if out_step is None:
            out_step = 2 * self.nkeep
        rows = self._unpacked_heaps(raw, layout, scale, npart)
        if rows is not None:
            return self.perform(rows[0], out, npart, rows[1], out_step)
        ocs, ops = _strides3(out) if out is not None else (0, 0)
        if npart:
            if layout != _lib.RAW_UWB16:
                self._need("raw block", raw.numel(), self._raw_bytes(npart, layout))
            if out is not None:
                self._need("output", out.shape[2], (npart - 1) * out_step + 2 * self.nkeep)
        _check(self.ctx.handle,
               lib.dspsr_amd_filterbank_perform_raw(self.handle, raw.data_ptr(), layout, scale,
                                                    out.data_ptr() if out is not None else None, ocs, ops, npart,
                                                    out_step), "dspsr_amd_filterbank_perform_raw")

    def perform_detect(self, det, npart, state=_lib.COHERENCE, ndim=4, inp=None, in_step=0, raw=None,
                       layout=_lib.RAW_GENERIC, scale=1.0):
        rows = self._unpacked_heaps(raw, layout, scale, npart)
        if rows is not None:
            inp, in_step, raw = rows[0], rows[1], None
        dcs, dps = _strides3(det)
        square_law = state in (_lib.INTENSITY, _lib.PPQQ)       # dspsr -d 1, -d 2: rows [nchan][1 | 2][npart * nkeep], ndim 1
        if square_law:
            ndim, npo = 1, 2 if state == _lib.PPQQ else 1
        if npart:
            self._need("detected block", det.shape[2], npart * self.nkeep * ndim)
            if square_law and det.shape[1] != npo:
                raise DspsrAmdError("dspsr_amd.FilterbankEngine.perform_detect: %s needs %d polarisation rows per channel, the block "
                                    "has %d" % ("PPQQ" if npo == 2 else "Intensity", npo, det.shape[1]))
            if not square_law and det.shape[1] != 4 // ndim:
                raise DspsrAmdError("dspsr_amd.FilterbankEngine.perform_detect: ndim=%d needs %d planes, the block has %d"
                                    % (ndim, 4 // ndim, det.shape[1]))
            if raw is not None and layout != _lib.RAW_UWB16:
                self._need("raw block", raw.numel(), self._raw_bytes(npart, layout))
            if inp is not None:
                self._need("input", inp.shape[2], (npart - 1) * in_step + self.nsamp_fft * (1 if self.cfg.real_input else 2))
        if inp is not None:
            ics, ips = _strides3(inp)
            iptr = inp.data_ptr()
        else:
            ics = ips = 0
            iptr = None
        _check(self.ctx.handle,
               lib.dspsr_amd_filterbank_perform_detect(self.handle, iptr, ics, ips, in_step,
                                                       raw.data_ptr() if raw is not None else None, layout, scale,
                                                       state, ndim, det.data_ptr(), dcs, dps, npart),
               "dspsr_amd_filterbank_perform_detect")

    def perform_search(self, out, carry, carry_count, npart, tscrunch, state=_lib.INTENSITY, inp=None, in_step=0, raw=None,
                       layout=_lib.RAW_GENERIC, scale=1.0):
        """digifil's convolving branch in one launch group (LoadToFil.C:185-222,250-304): Filterbank -> Detection::square_law
        (Intensity / PPQQ), or Detection of the four Coherence products PP, QQ, Re PQ*, Im PQ* (state COHERENCE: digifits -p 4,
        digifil -d 4) -> TScrunch on the detected stream.  out: device float32 rows [nchan][npol_out][>= nout]; carry:
        device float32 [nchan][npol_out] (the open output sample's partial sums); carry_count: samples already in it.
        npol_out is 1, 2 or 4.  Returns (nout, carry_count_after).  search_fuses(state, tscrunch) tells whether the call runs
        inside the inverse pass."""
        rows = self._unpacked_heaps(raw, layout, scale, npart)
        if rows is not None:
            inp, in_step, raw = rows[0], rows[1], None
        ocs, ops = _strides3(out)
        npo = 4 if state == _lib.COHERENCE else 2 if state == _lib.PPQQ else 1
        if out.shape[1] != npo or carry.numel() < out.shape[0] * npo:
            raise DspsrAmdError("dspsr_amd.FilterbankEngine.perform_search: out needs %d polarisation rows per channel and carry "
                                "[nchan][%d] floats" % (npo, npo))
        if npart:
            self._need("scrunched block", out.shape[2], (carry_count + npart * self.nkeep) // max(1, tscrunch))
            if raw is not None and layout != _lib.RAW_UWB16:
                self._need("raw block", raw.numel(), self._raw_bytes(npart, layout))
        if inp is not None:
            ics, ips = _strides3(inp)
            iptr = inp.data_ptr()
        else:
            ics = ips = 0
            iptr = None
        cc, nout = C.c_uint32(carry_count), C.c_uint64(0)
        _check(self.ctx.handle,
               lib.dspsr_amd_filterbank_perform_search(self.handle, iptr, ics, ips, in_step, raw.data_ptr() if raw is not None else None,
                                                       layout, scale, state, tscrunch, out.data_ptr(), ocs, ops, carry.data_ptr(),
                                                       C.byref(cc), npart, C.byref(nout)), "dspsr_amd_filterbank_perform_search")
        return int(nout.value), int(cc.value)

    def search_is_fused(self) -> bool:
        """perform_search runs detection and the time scrunch inside the inverse pass (else: separate launches, same numbers)."""
        return bool(lib.dspsr_amd_filterbank_search_is_fused(self.handle))

    def search_fuses(self, state, tscrunch) -> bool:
        """perform_search(state, tscrunch) runs inside the inverse pass.  False: separate launches on the object's own block,
        the same numbers -- for COHERENCE wherever tscrunch * G > freq_res (G = ((nkeep + 2 tscrunch - 2) // tscrunch) | 1),
        and for a state that is not a search-mode one."""
        return bool(lib.dspsr_amd_filterbank_search_is_fused_state(self.handle, int(state), int(tscrunch)))

    def npass(self, raw_input: bool = True) -> int:
        """Transform passes of a call: 2 (short responses on the 8-bit block), 3, or 4 (two-pass inverse)."""
        return int(lib.dspsr_amd_filterbank_npass(self.handle, 1 if raw_input else 0))

    def presplit(self) -> bool:
        """True: the forward row pass splits the polarisations and the inverse pass loads them ready."""
        return bool(lib.dspsr_amd_filterbank_presplit(self.handle))

    def fold_is_fused(self, state=_lib.COHERENCE) -> int:
        """0: perform_fold runs Detection + Fold launches; 1: it folds inside the last filterbank pass with exact time-order
        sums (one workgroup per channel tile); 2: it folds inside the last pass with the parts of a launch cut into runs
        (geometries with fewer tiles than compute units): sums re-associated per run, equal to float rounding.
        state: INTENSITY and PPQQ have a fused kernel of their own and never answer 3 (segment sums)."""
        return int(lib.dspsr_amd_filterbank_fold_is_fused_state(self.handle, state))

    def perform_fold(self, fold, npart, state=_lib.COHERENCE, inp=None, in_step=0, raw=None,
                     layout=_lib.RAW_GENERIC, scale=1.0):
        """Fused filterbank -> detection (ndim 4) -> fold into `fold`'s device profile; the bin plan of the
        npart*nkeep output samples must already have been given to `fold` (set_nbin/set_ndat/set_bins).
        state INTENSITY / PPQQ (dspsr -d 1, -d 2): `fold` has the shape npol 1 x ndim 1 / npol 2 x ndim 1."""
        rows = self._unpacked_heaps(raw, layout, scale, npart)
        if rows is not None:
            inp, in_step, raw = rows[0], rows[1], None
        if npart:
            if raw is not None and layout != _lib.RAW_UWB16:
                self._need("raw block", raw.numel(), self._raw_bytes(npart, layout))
            if inp is not None:
                self._need("input", inp.shape[2], (npart - 1) * in_step + self.nsamp_fft * (1 if self.cfg.real_input else 2))
        if inp is not None:
            ics, ips = _strides3(inp)
            iptr = inp.data_ptr()
        else:
            ics = ips = 0
            iptr = None
        _check(self.ctx.handle,
               lib.dspsr_amd_filterbank_perform_fold(self.handle, iptr, ics, ips, in_step,
                                                     raw.data_ptr() if raw is not None else None, layout, scale,
                                                     state, fold.handle, npart),
               "dspsr_amd_filterbank_perform_fold")

    def finish(self):
        self.ctx.synchronize()


class ConvolutionEngine(FilterbankEngine):
    """Mirror of dsp::Convolution::Engine (Signal/General/dsp/Convolution.h:158-167; CUDA twin
    ConvolutionCUDA.cu:202-800): coherent dedispersion of already-channelised (or single-channel) voltages.
    One forward FFT, response multiply and backward FFT of `ndat` points per (channel, pol, part) -- the
    filterbank object with nchan_subband = 1."""

    def prepare(self, ndat, nfilt_pos, nfilt_neg, nchan=1, npol=2, real_input=False, kernel=None, max_parts=1,
                force_four_pass=False):
        return self.setup(1, ndat, nfilt_pos, nfilt_neg, nchan, npol, real_input, kernel, max_parts=max_parts,
                          force_four_pass=force_four_pass)


def tfp_filterbank(ctx: Context, raw, nchan, npart, out, pscrunch=False, tscrunch=1, layout=_lib.RAW_GENERIC,
                   scale=1.0):
    """digifil front end: dsp::TFPFilterbank (+pscrunch) + dsp::TScrunch fused (TFPFilterbank.C:27-101,
    TScrunch.C:180-206).  raw: device int8 block (real, 2 pols); out: device float32
    [npart // tscrunch][nchan][1 or 2]."""
    cfg = _lib.TfpConfig(nchan, 2, int(bool(pscrunch)), int(tscrunch))
    _check(ctx.handle, lib.dspsr_amd_tfp_filterbank(ctx.handle, C.byref(cfg), raw.data_ptr(), layout, scale,
                                                    out.data_ptr(), npart), "dspsr_amd_tfp_filterbank")


def sigproc_digitize_fpt(ctx: Context, inp, out, nbit=8, use_digi_scales=True, input_scale=1.0, scale_fac=1.0, flip_band=False,
                         swap_band=False):
    """dsp::SigProcDigitizer::pack on FPT rows [nchan][npol][ndat] (float32, device) -> packed n-bit device bytes in TPF order."""
    nchan, npol, ndat = inp.shape
    ics, ips = _strides3(inp)
    _check(ctx.handle, lib.dspsr_amd_sigproc_digitize_fpt(ctx.handle, inp.data_ptr(), ics, ips, ndat, nchan, npol, nbit, int(use_digi_scales),
                                                          input_scale, scale_fac, int(flip_band), int(swap_band), out.data_ptr()),
           "dspsr_amd_sigproc_digitize_fpt")
    return out


def tscrunch_fpt(ctx: Context, inp, out, sfactor, carry, carry_count=0, ndim=1):
    """dsp::TScrunch::fpt_tscrunch on device rows [nchan][npol][ndat * ndim] as a stream (carry: device [nchan][npol][ndim]
    floats).  Returns (nout, carry_count_after)."""
    nchan, npol, nfloat = inp.shape
    ics, ips = _strides3(inp)
    ocs, ops = _strides3(out)
    cc, nout = C.c_uint32(carry_count), C.c_uint64(0)
    _check(ctx.handle, lib.dspsr_amd_tscrunch_fpt(ctx.handle, inp.data_ptr(), ics, ips, out.data_ptr(), ocs, ops, nchan, npol, ndim,
                                                  nfloat // ndim, sfactor, carry.data_ptr(), C.byref(cc), C.byref(nout)),
           "dspsr_amd_tscrunch_fpt")
    return int(nout.value), int(cc.value)


def unpack_fpt(ctx: Context, raw, out, nchan, npol, ndim, scale=1.0, ndat=None):
    """The generic 8-bit unpacker on the device (BitUnpacker.C:48-80): raw = device int8 block in DADA order [ndat][nchan][npol][ndim]
    (any byte address), out = float32 device rows [nchan][npol][>= ndat * ndim] (strided views allowed)."""
    per = nchan * npol * ndim
    ndat = raw.numel() // per if ndat is None else ndat
    if raw.numel() < ndat * per:
        raise DspsrAmdError("dspsr_amd.unpack_fpt: block holds %d bytes, %d needed" % (raw.numel(), ndat * per))
    if tuple(out.shape[:2]) != (nchan, npol) or out.shape[2] < ndat * ndim:
        raise DspsrAmdError("dspsr_amd.unpack_fpt: out is %s, [%d][%d][>= %d] needed" % (tuple(out.shape), nchan, npol, ndat * ndim))
    ocs, ops = _strides3(out)
    _check(ctx.handle, lib.dspsr_amd_unpack_fpt(ctx.handle, raw.data_ptr(), scale, nchan, npol, ndim, ndat, out.data_ptr(), ocs, ops),
           "dspsr_amd_unpack_fpt")
    return out


def unpack_heaps_fpt(ctx: Context, raw, out, nchan, npol, layout, scale=1.0, ndat=None):
    """dsp::MeerKATUnpacker on the device: raw = device int8 block of whole heaps [heap][npol][nchan][256][2] (16-byte aligned),
    layout = RAW_MEERKAT / RAW_MEERKAT_SWAP or raw_at(layout, first_sample); out = float32 device rows [nchan][npol][>= 2 * ndat]
    (strided views allowed) that receive stream samples first_sample ... first_sample + ndat - 1.  ndat=None: all the block holds."""
    if not _lib.is_heaps(layout):
        raise DspsrAmdError("dspsr_amd.unpack_heaps_fpt: layout %d is not a heap layout" % layout)
    first = layout >> 8
    per = nchan * npol * _lib.HEAP_NSAMP * 2
    ndat = (raw.numel() // per) * _lib.HEAP_NSAMP - first if ndat is None else ndat
    need = -(-(first + ndat) // _lib.HEAP_NSAMP) * per if ndat > 0 else 0
    if ndat < 0 or raw.numel() < need:
        raise DspsrAmdError("dspsr_amd.unpack_heaps_fpt: block holds %d bytes, %d needed" % (raw.numel(), need))
    if tuple(out.shape[:2]) != (nchan, npol) or out.shape[2] < 2 * ndat:
        raise DspsrAmdError("dspsr_amd.unpack_heaps_fpt: out is %s, [%d][%d][>= %d] needed" % (tuple(out.shape), nchan, npol, 2 * ndat))
    ocs, ops = _strides3(out)
    _check(ctx.handle, lib.dspsr_amd_unpack_heaps_fpt(ctx.handle, raw.data_ptr(), layout, scale, nchan, npol, ndat, out.data_ptr(), ocs, ops),
           "dspsr_amd_unpack_heaps_fpt")
    return out


def unpack_guppi_fpt(ctx: Context, raw, rows, layout, ndat):
    """dsp::GUPPIUnpacker and the un-transpose of GUPPIBlockFile::load_bytes on the device: raw = device int8, the data sections of
    GUPPI raw blocks as they lie in the file, from the block that holds the first sample on; layout = _lib.GuppiLayout (nchan, npol,
    block_nsamp, first, chan_stride, block_stride: dspsr_amd_guppi_layout); rows = float32 device rows [nchan][npol][>= 2 * ndat]
    (strided views allowed) that receive stream samples first ... first + ndat - 1 as float(int8)."""
    nchan, npol = layout.nchan, layout.npol
    if ndat < 0:
        raise DspsrAmdError("dspsr_amd.unpack_guppi_fpt: ndat=%d" % ndat)
    if ndat and layout.block_nsamp and npol:
        need = _lib.guppi_block_bytes(layout.first, ndat, nchan, npol, layout.block_nsamp, layout.chan_stride, layout.block_stride)
        if raw.numel() * raw.element_size() < need:
            raise DspsrAmdError("dspsr_amd.unpack_guppi_fpt: block holds %d bytes, %d needed" % (raw.numel() * raw.element_size(), need))
    if tuple(rows.shape[:2]) != (nchan, npol) or rows.shape[2] < 2 * ndat:
        raise DspsrAmdError("dspsr_amd.unpack_guppi_fpt: rows are %s, [%d][%d][>= %d] needed" % (tuple(rows.shape), nchan, npol, 2 * ndat))
    ocs, ops = _strides3(rows)
    _check(ctx.handle, lib.dspsr_amd_unpack_guppi_fpt(ctx.handle, raw.data_ptr(), C.byref(layout), ndat, rows.data_ptr(), ocs, ops),
           "dspsr_amd_unpack_guppi_fpt")
    return rows


def unpack_sigproc_fpt(ctx: Context, raw, rows, nbit, nchan, npol, ndat):
    """dsp::SigProcUnpacker (OrderFPT) on the device: raw = device bytes (any dtype), `ndat` spectra of a SIGPROC filterbank file as
    they lie in it -- npol * nchan values of nbit bits each, polarisation by polarisation --, at any byte address (nbit 16 / 32: a
    multiple of the value's size); rows = float32 device rows [nchan][npol][>= ndat] (strided views allowed) that receive
    float(value), less 127.5 (nbit 8) or 32768 (nbit 16) in the rows of polarisations 2 and 3; nbit 32: the floats as they are."""
    if ndat < 0:
        raise DspsrAmdError("dspsr_amd.unpack_sigproc_fpt: ndat=%d" % ndat)
    need = ndat * ((npol * nchan * nbit) // 8)
    if raw.numel() * raw.element_size() < need:
        raise DspsrAmdError("dspsr_amd.unpack_sigproc_fpt: block holds %d bytes, %d needed" % (raw.numel() * raw.element_size(), need))
    if tuple(rows.shape[:2]) != (nchan, npol) or rows.shape[2] < ndat:
        raise DspsrAmdError("dspsr_amd.unpack_sigproc_fpt: rows are %s, [%d][%d][>= %d] needed" % (tuple(rows.shape), nchan, npol, ndat))
    ocs, ops = _strides3(rows)
    _check(ctx.handle, lib.dspsr_amd_unpack_sigproc_fpt(ctx.handle, raw.data_ptr(), nbit, nchan, npol, ndat, rows.data_ptr(), ocs, ops),
           "dspsr_amd_unpack_sigproc_fpt")
    return rows


def twobit_block_bytes(first_sample, ndat, nsample, npol):
    """Bytes of the whole windows that hold `ndat` samples from `first_sample` of the first window on."""
    return -(-(first_sample + ndat) // nsample) * (nsample // 4) * npol if ndat > 0 else 0


def twobit_check(raw_addr, table_type, npol, nsample, first_sample, ndat, nlow_min, nlow_max, out_addr=0, out_pol_stride=None):
    """dspsr_amd_twobit_check: what dspsr_amd_twobit_unpack refuses, without a device (addresses as integers)."""
    _host_check(lib.dspsr_amd_twobit_check, raw_addr, table_type, npol, nsample, first_sample, ndat, nlow_min, nlow_max, out_addr,
                ndat if out_pol_stride is None else out_pol_stride)


def twobit_unpack(ctx: Context, raw, out, levels, weights, nsample, nlow_min, nlow_max, table_type=_lib.TWOBIT_OFFSET_BINARY,
                  first_sample=0, ndat=None, nlow=None):
    """dsp::TwoBitCorrection on the device: raw = device uint8 / int8 block of whole windows (4-byte aligned; byte k belongs to
    digitiser k % npol, four samples per byte, first sample in the top bits), out = float32 device rows [npol][>= ndat], levels =
    device float32 [nlow_max - nlow_min + 1][2] (twobit.levels), weights = device int32 [npol][nwindow] (per digitiser, 0 / 1,
    before mask_weights), nlow = the same shape or None.  The rows receive samples first_sample ... first_sample + ndat - 1 of the
    block.  ndat=None: all the block holds behind first_sample."""
    npol = out.shape[0]
    assert out.dim() == 2 and out.stride(1) == 1, "rows must be contiguous"
    per = (nsample // 4) * npol
    if ndat is None:
        ndat = (raw.numel() // per) * nsample - first_sample if per else 0
    need = twobit_block_bytes(first_sample, ndat, nsample, npol) if nsample else 0
    nwindow = need // per if per else 0
    if ndat < 0 or raw.numel() < need:
        raise DspsrAmdError("dspsr_amd.twobit_unpack: block holds %d bytes, %d needed" % (raw.numel(), need))
    if out.shape[1] < ndat:
        raise DspsrAmdError("dspsr_amd.twobit_unpack: out is %s, [%d][>= %d] needed" % (tuple(out.shape), npol, ndat))
    if levels.numel() < 2 * (nlow_max - nlow_min + 1):
        raise DspsrAmdError("dspsr_amd.twobit_unpack: the level table holds %d floats, %d needed"
                            % (levels.numel(), 2 * (nlow_max - nlow_min + 1)))
    for name, t in (("weights", weights), ("nlow", nlow)):
        if t is not None and (t.element_size() != 4 or not t.is_contiguous() or tuple(t.shape) != (npol, nwindow)):
            raise DspsrAmdError("dspsr_amd.twobit_unpack: %s must be contiguous 32-bit [%d][%d], got %s" % (name, npol, nwindow, tuple(t.shape)))
    _check(ctx.handle, lib.dspsr_amd_twobit_unpack(ctx.handle, raw.data_ptr(), table_type, npol, nsample, first_sample, ndat, nlow_min,
                                                   nlow_max, levels.data_ptr(), out.data_ptr(), out.stride(0) if npol > 1 else ndat,
                                                   weights.data_ptr(), nlow.data_ptr() if nlow is not None else None),
           "dspsr_amd_twobit_unpack")
    return out


def detect_raw(ctx: Context, raw, out, carry, carry_count, nchan, npol, tscrunch=1, state=_lib.INTENSITY, scale=1.0, ndat=None):
    """Unpack -> Detection -> TScrunch of a channelised complex 8-bit block [ndat][nchan][npol][2] in one pass, as a stream: out =
    float32 device rows [nchan][npol_out][>= nout] (Intensity 1 / PPQQ 2 / Coherence 4: PP, QQ, Re, Im), carry = device
    [nchan][npol_out] floats (None allowed with tscrunch 1).  Returns (nout, carry_count_after)."""
    per = nchan * npol * 2
    ndat = raw.numel() // per if ndat is None else ndat
    if raw.numel() < ndat * per:
        raise DspsrAmdError("dspsr_amd.detect_raw: block holds %d bytes, %d needed" % (raw.numel(), ndat * per))
    ocs, ops = _strides3(out)
    cc, nout = C.c_uint32(carry_count or 0), C.c_uint64(0)
    _check(ctx.handle, lib.dspsr_amd_detect_raw(ctx.handle, raw.data_ptr(), scale, nchan, npol, ndat, state, tscrunch, out.data_ptr(), ocs, ops,
                                                carry.data_ptr() if carry is not None else None,
                                                C.byref(cc) if carry_count is not None else None, C.byref(nout)),
           "dspsr_amd_detect_raw")
    return int(nout.value), int(cc.value)


def fscrunch_fpt(ctx: Context, inp, out, sfactor):
    """dsp::FScrunch::fpt_fscrunch on device rows [nchan][npol][nfloat] -> [nchan / sfactor][npol][nfloat]."""
    nchan, npol, nfloat = inp.shape
    ics, ips = _strides3(inp)
    ocs, ops = _strides3(out)
    _check(ctx.handle, lib.dspsr_amd_fscrunch_fpt(ctx.handle, inp.data_ptr(), ics, ips, out.data_ptr(), ocs, ops, nchan, npol, nfloat, sfactor),
           "dspsr_amd_fscrunch_fpt")
    return out


def copy_data_fpt(ctx: Context, to, frm):
    """dsp::TimeSeries::Engine::copy_data_fpt: device rows [nchan][npol][nfloat] (strided views allowed)."""
    nchan, npol, nfloat = frm.shape
    _check(ctx.handle, lib.dspsr_amd_copy_fpt(ctx.handle, to.data_ptr(), to.stride(0), to.stride(1), frm.data_ptr(), frm.stride(0),
                                             frm.stride(1), nchan, npol, nfloat), "dspsr_amd_copy_fpt")


def add_fpt(ctx: Context, to, frm):
    """dsp::TimeSeries::operator += on device rows [nchan][npol][nfloat] (PhaseSeries::combine): to += frm."""
    nchan, npol, nfloat = frm.shape
    _check(ctx.handle, lib.dspsr_amd_add_fpt(ctx.handle, to.data_ptr(), to.stride(0), to.stride(1), frm.data_ptr(), frm.stride(0),
                                            frm.stride(1), nchan, npol, nfloat), "dspsr_amd_add_fpt")


def dedispersion_sample_delays(centre_frequency, bandwidth, dispersion_measure, nchan, rate_hz, swap=False, nsub_swap=0,
                               dc_centred=False):
    """Dedispersion::SampleDelay::match (DedispersionSampleDelay.C:24-75): int64 delay of each channel in samples."""
    d = np.zeros(nchan, np.int64)
    rc = lib.dspsr_amd_dedispersion_sample_delays(centre_frequency, bandwidth, dispersion_measure, nchan, rate_hz, int(swap),
                                                  nsub_swap, int(dc_centred), d.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise DspsrAmdError("dsp::Dedispersion::SampleDelay::match invalid input")
    return d


class SampleDelay(_Owned):
    """Mirror of dsp::SampleDelay (Signal/General/SampleDelay.C): delays[ichan][ipol] from a SampleDelayFunction."""

    _abi = "dspsr_amd_sample_delay"

    def __init__(self, ctx: Context, delays, npol=1, absolute=False):
        super().__init__(ctx)
        d = np.ascontiguousarray(np.asarray(delays, np.int64))
        if d.ndim == 1:                                       # per channel, same for every polarisation
            d = np.ascontiguousarray(np.repeat(d[:, None], npol, axis=1))
        self.nchan, self.npol = d.shape
        self._create(self.nchan, self.npol, d.ctypes.data_as(C.c_void_p), int(absolute))
        self.zero_delay = lib.dspsr_amd_sample_delay_zero_delay(self.handle)
        self.total_delay = lib.dspsr_amd_sample_delay_total_delay(self.handle)

    def transform(self, inp, out=None):
        """inp/out: float32 device tensors [nchan][npol][ndat][ndim] (the last axis may be absent); returns ndat_out."""
        out = inp if out is None else out
        ndim = inp.shape[3] if inp.dim() == 4 else 1
        n = C.c_uint64(0)
        _check(self.ctx.handle, lib.dspsr_amd_sample_delay_transform(
            self.handle, inp.data_ptr(), inp.stride(0), inp.stride(1), out.data_ptr(), out.stride(0), out.stride(1), ndim,
            inp.shape[2], C.byref(n)), "dspsr_amd_sample_delay_transform")
        return n.value


class Rescale(_Owned):
    """Mirror of dsp::Rescale for TFP-ordered detected data (Signal/General/Rescale.C): offset/scale per (pol, chan)."""

    _abi = "dspsr_amd_rescale"

    def __init__(self, ctx: Context, nchan, npol=1, interval_samples=0, constant=False):
        super().__init__(ctx)
        self.nchan, self.npol = nchan, npol
        self._create(nchan, npol, interval_samples, int(constant))

    def transform(self, inp, out=None):
        """inp/out: float32 device tensors [ndat][nchan][npol] (out defaults to in place)."""
        out = inp if out is None else out
        ndat = inp.numel() // (self.nchan * self.npol)
        _check(self.ctx.handle, lib.dspsr_amd_rescale_transform(self.handle, inp.data_ptr(), out.data_ptr(), ndat),
               "dspsr_amd_rescale_transform")
        return out

    def transform_fpt(self, inp, out=None):
        """FPT rows: inp/out float32 device tensors [nchan][npol][ndat] (strided views allowed; out defaults to in place)."""
        out = inp if out is None else out
        ics, ips = _strides3(inp)
        ocs, ops = _strides3(out)
        _check(self.ctx.handle, lib.dspsr_amd_rescale_transform_fpt(self.handle, inp.data_ptr(), ics, ips, out.data_ptr(), ocs, ops,
                                                                    inp.shape[2]), "dspsr_amd_rescale_transform_fpt")
        return out

    def digitize_fpt(self, inp, out, nbit=8, scale_fac=1.0, flip_band=False, swap_band=False):
        """Rescale -> SigProcDigitizer of FPT rows [nchan][npol][ndat] in one pass (the bytes of transform_fpt() +
        sigproc_digitize_fpt(), without the rescaled block)."""
        ics, ips = _strides3(inp)
        ndat = inp.shape[2]
        need = ndat * self.nchan * self.npol * nbit // 8
        if out.numel() * out.element_size() < need:
            raise DspsrAmdError("dspsr_amd.Rescale.digitize_fpt: out holds %d bytes, %d needed" % (out.numel() * out.element_size(), need))
        _check(self.ctx.handle, lib.dspsr_amd_rescale_digitize_fpt(self.handle, inp.data_ptr(), ics, ips, ndat, nbit, scale_fac,
                                                                   int(flip_band), int(swap_band), out.data_ptr()),
               "dspsr_amd_rescale_digitize_fpt")
        return out

    def pscrunch_digitize(self, inp, out, nbit=8, scale_fac=1.0, flip_band=False, swap_band=False):
        """Rescale -> PScrunch -> SigProcDigitizer of a PPQQ block [ndat][nchan][2] in one pass (the bytes of transform() +
        pscrunch_tfp() + sigproc_digitize(), without the two intermediate blocks)."""
        ndat = inp.numel() // (self.nchan * self.npol)
        need = ndat * self.nchan * nbit // 8
        if out.numel() * out.element_size() < need:
            raise DspsrAmdError("dspsr_amd.Rescale.pscrunch_digitize: out holds %d bytes, %d needed" % (out.numel() * out.element_size(), need))
        _check(self.ctx.handle,
               lib.dspsr_amd_rescale_pscrunch_digitize(self.handle, inp.data_ptr(), ndat, nbit, scale_fac, int(flip_band), int(swap_band),
                                                       out.data_ptr()), "dspsr_amd_rescale_pscrunch_digitize")
        return out

    def get(self):
        off = np.empty(self.nchan * self.npol, np.float32)
        sc = np.empty(self.nchan * self.npol, np.float32)
        _check(self.ctx.handle, lib.dspsr_amd_rescale_get(self.handle, off.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p)),
               "dspsr_amd_rescale_get")
        return off.reshape(self.nchan, self.npol), sc.reshape(self.nchan, self.npol)


class FITSDigitizer(_Owned):
    """Mirror of dsp::FITSDigitizer with set_rescale_samples(nsblk) (Kernel/Formats/fits/FITSDigitizer.C): the reference spectrum of
    each block of nsblk samples (a running mean over nblock blocks), applied to that block, digi_sigma 8, MSB-first packing."""

    _abi = "dspsr_amd_fits_digitizer"

    def __init__(self, ctx: Context, nchan, npol=1, nbit=2, nsblk=2048, nblock=1, constant=False, flip_band=False, swap_band=False):
        super().__init__(ctx)
        self.nchan, self.npol, self.nbit, self.nsblk, self.nblock = nchan, npol, nbit, nsblk, nblock
        self._create(nchan, npol, nbit, nsblk, nblock, int(constant), int(flip_band), int(swap_band))
        self.block_bytes = nsblk * npol * nchan * nbit // 8

    @property
    def zero_off(self) -> float:
        """ZERO_OFF of the PSRFITS SUBINT header, 2^(nbit-1) - 0.5"""
        return 2.0 ** (self.nbit - 1) - 0.5

    def pack(self, inp, out, dat_scl, dat_offs):
        """rescale_pack() of one block: inp float32 device rows [nchan][npol][nsblk] (strided views allowed), out device uint8
        [nsblk * npol * nchan * nbit / 8] in TPF order, dat_scl / dat_offs device float32 [npol * nchan].  No synchronisation."""
        if tuple(inp.shape) != (self.nchan, self.npol, self.nsblk):
            raise DspsrAmdError("dspsr_amd.FITSDigitizer.pack: rows %s, one block is [%d][%d][%d]"
                                % (tuple(inp.shape), self.nchan, self.npol, self.nsblk))
        for name, t, need in (("out", out, self.block_bytes), ("dat_scl", dat_scl, 4 * self.nchan * self.npol),
                              ("dat_offs", dat_offs, 4 * self.nchan * self.npol)):
            if t.numel() * t.element_size() < need:
                raise DspsrAmdError("dspsr_amd.FITSDigitizer.pack: %s holds %d bytes, %d needed" % (name, t.numel() * t.element_size(), need))
        ics, ips = _strides3(inp)
        _check(self.ctx.handle, lib.dspsr_amd_fits_digitizer_pack(self.handle, inp.data_ptr(), ics, ips, out.data_ptr(), dat_scl.data_ptr(),
                                                                 dat_offs.data_ptr()), "dspsr_amd_fits_digitizer_pack")
        return out


def pscrunch_tfp(ctx: Context, inp, out, nchan, npol=2):
    """dsp::PScrunch on TFP-ordered device data: out[t][c] = (p0 + p1) * float(1/sqrt(2)); out of place."""
    ndat = inp.numel() // (nchan * npol)
    _check(ctx.handle, lib.dspsr_amd_pscrunch_tfp(ctx.handle, inp.data_ptr(), out.data_ptr(), ndat, nchan, npol),
           "dspsr_amd_pscrunch_tfp")
    return out


def sigproc_digitize(ctx: Context, inp, out, nchan, npol=1, nbit=8, use_digi_scales=True, input_scale=1.0, scale_fac=1.0,
                     flip_band=False, swap_band=False):
    """dsp::SigProcDigitizer::pack on TFP-ordered float32 device data -> packed n-bit device bytes."""
    ndat = inp.numel() // (nchan * npol)
    _check(ctx.handle, lib.dspsr_amd_sigproc_digitize(ctx.handle, inp.data_ptr(), ndat, nchan, npol, nbit, int(use_digi_scales),
                                                      input_scale, scale_fac, int(flip_band), int(swap_band), out.data_ptr()),
           "dspsr_amd_sigproc_digitize")
    return out


class DetectionEngine:
    """dsp::Detection::Engine."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def polarimetry(self, ndim, inp, out, state=_lib.COHERENCE):
        ics, ips = _strides3(inp)
        ocs, ops = _strides3(out)
        nchan = inp.shape[0]
        ndat = inp.shape[2] // 2
        _check(self.ctx.handle,
               lib.dspsr_amd_detect_polarimetry(self.ctx.handle, state, ndim, inp.data_ptr(), ics, ips,
                                                out.data_ptr(), ocs, ops, nchan, ndat),
               "dspsr_amd_detect_polarimetry")

    def square_law(self, inp, out, intensity=False):
        ics, ips = _strides3(inp)
        ocs, ops = _strides3(out)
        _check(self.ctx.handle,
               lib.dspsr_amd_detect_square_law(self.ctx.handle, int(intensity), inp.data_ptr(), ics, ips,
                                               out.data_ptr(), ocs, ops, inp.shape[0], inp.shape[1],
                                               inp.shape[2] // 2), "dspsr_amd_detect_square_law")


def fourth_moment(ctx: Context, inp, out, ndat=None):
    """dsp::FourthMoment::transformation (FourthMoment.C:29-77): inp float32 [nchan][1][>= ndat*4] Stokes rows, out float32
    [nchan][1][>= ndat*14]; ndat defaults to the samples inp holds.  Out of place."""
    ics, _ = _strides3(inp)
    ocs, _ = _strides3(out)
    if ndat is None:
        ndat = inp.shape[2] // 4
    _check(ctx.handle, lib.dspsr_amd_fourth_moment(ctx.handle, inp.data_ptr(), ics, out.data_ptr(), ocs, inp.shape[0], ndat),
           "dspsr_amd_fourth_moment")


class FoldEngine(_Owned):
    """dsp::Fold::Engine; owns the device-resident profiles (get_profiles)."""

    _abi = "dspsr_amd_fold"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self._create()
        self.shape = None

    def set_shape(self, nchan, npol, ndim, nbin):
        _check(self.ctx.handle, lib.dspsr_amd_fold_set_shape(self.handle, nchan, npol, ndim, nbin),
               "dspsr_amd_fold_set_shape")
        self.shape = (nchan, npol, nbin, ndim)

    def bind_profile(self, prof, nchan, npol, ndim, nbin):
        """Fold::Engine::setup: fold into the caller's device PhaseSeries buffer; prof: float32 device tensor
        [nchan*npol][span >= nbin*ndim] (rows may be padded), None = back to a library-owned profile."""
        if prof is None:
            _check(self.ctx.handle, lib.dspsr_amd_fold_bind_profile(self.handle, None, 0, nchan, npol, ndim, nbin),
                   "dspsr_amd_fold_bind_profile")
        else:
            assert prof.dim() == 2 and prof.shape[0] == nchan * npol and prof.stride(1) == 1
            _check(self.ctx.handle, lib.dspsr_amd_fold_bind_profile(self.handle, prof.data_ptr(), prof.stride(0), nchan, npol,
                                                                    ndim, nbin), "dspsr_amd_fold_bind_profile")
        self.shape = (nchan, npol, nbin, ndim)

    def set_nbin(self, nbin):
        _check(self.ctx.handle, lib.dspsr_amd_fold_set_nbin(self.handle, nbin), "dspsr_amd_fold_set_nbin")

    def set_ndat(self, ndat, idat_start):
        _check(self.ctx.handle, lib.dspsr_amd_fold_set_ndat(self.handle, ndat, idat_start), "dspsr_amd_fold_set_ndat")

    def set_bin(self, idat, ibin, bins_per_samp=0.0):
        _check(self.ctx.handle, lib.dspsr_amd_fold_set_bin(self.handle, idat, ibin, bins_per_samp),
               "dspsr_amd_fold_set_bin")

    def set_bins(self, phi, phase_per_sample, ndat, idat_start, hits: np.ndarray | None = None, weights=None,
                 ndatperweight=0, weight_idat=0):
        """weights (uint32, one per ndatperweight samples; sample idat belongs to weight (idat + weight_idat) //
        ndatperweight): samples of a zero weight are not folded (Fold.C:686-716,746-763)."""
        n = C.c_uint64()
        hp = hits.ctypes.data_as(C.c_void_p) if hits is not None else None
        if weights is None:
            _check(self.ctx.handle,
                   lib.dspsr_amd_fold_set_bins(self.handle, phi, phase_per_sample, ndat, idat_start, hp, C.byref(n)),
                   "dspsr_amd_fold_set_bins")
        else:
            w = np.ascontiguousarray(weights, dtype=np.uint32)
            _check(self.ctx.handle,
                   lib.dspsr_amd_fold_set_bins_weighted(self.handle, phi, phase_per_sample, ndat, idat_start,
                                                        w.ctypes.data_as(C.c_void_p), w.size, ndatperweight, weight_idat, hp,
                                                        C.byref(n)), "dspsr_amd_fold_set_bins_weighted")
        return n.value

    def get_ndat_folded(self):
        return lib.dspsr_amd_fold_get_ndat_folded(self.handle)

    def fold(self, inp):
        cs, ps = _strides3(inp)
        _check(self.ctx.handle, lib.dspsr_amd_fold_fold(self.handle, inp.data_ptr(), cs, ps), "dspsr_amd_fold_fold")

    def fold_moments(self, stokes):
        """fold() of a shape (nchan, 1, 14, nbin) from the ndim 4 Stokes rows themselves, float32 [nchan][1][>= ndat*4]: the ten
        products of dsp::FourthMoment are formed in registers (dspsr_amd_fold_fold_moments).  Bit-identical to fold() of the
        rows fourth_moment() writes."""
        cs, _ps = _strides3(stokes)
        _check(self.ctx.handle, lib.dspsr_amd_fold_fold_moments(self.handle, stokes.data_ptr(), cs), "dspsr_amd_fold_fold_moments")

    @staticmethod
    def fold_many(folds, inp) -> int:
        """fold() of several engines over the same detected rows (one Fold per pulsar): the exact-order plans share launches that
        read `inp` once (dspsr_amd_fold_fold_many); every profile ends bit-identical to its own fold().  Returns how many engines
        took a shared launch (two or more exact-order plans share; a lone one is folded by fold())."""
        folds = list(folds)
        if not folds:
            return 0
        cs, ps = _strides3(inp)
        handles = (C.c_void_p * len(folds))(*[f.handle for f in folds])
        n = C.c_uint32(0)
        _check(folds[0].ctx.handle, lib.dspsr_amd_fold_fold_many(handles, len(folds), inp.data_ptr(), cs, ps, C.byref(n)),
               "dspsr_amd_fold_fold_many")
        return n.value

    def fold_zeroed(self, inp, hits_dev):
        """fold() of an input with zeroed samples: hits_dev (uint32 device tensor [nchan][nbin]) counts, per channel, the
        planned samples of polarisation 0 whose first float is not zero (Fold.C:853-866)."""
        cs, ps = _strides3(inp)
        assert hits_dev.is_contiguous() and hits_dev.numel() == self.shape[0] * self.shape[2]
        _check(self.ctx.handle, lib.dspsr_amd_fold_fold_zeroed(self.handle, inp.data_ptr(), cs, ps, hits_dev.data_ptr()),
               "dspsr_amd_fold_fold_zeroed")

    def get_profiles_ptr(self):
        return lib.dspsr_amd_fold_profiles_dev(self.handle)

    def zero(self):
        _check(self.ctx.handle, lib.dspsr_amd_fold_zero(self.handle), "dspsr_amd_fold_zero")

    def synch(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float32)
        _check(self.ctx.handle, lib.dspsr_amd_fold_synch(self.handle, out.ctypes.data_as(C.c_void_p)),
               "dspsr_amd_fold_synch")
        return out


def cyclic_binplan(phi: float, phase_per_sample: float, nbin: int, ndat: int):
    """The two plans of lag folding (CyclicFold.C:293-301 fed by Fold.C:744-787) and hits[nbin]."""
    p0, p1 = np.empty(ndat, dtype=np.uint32), np.empty(ndat, dtype=np.uint32)
    hits = np.zeros(nbin, dtype=np.uint32)
    code = lib.dspsr_amd_cyclic_binplan(phi, phase_per_sample, nbin, ndat, p0.ctypes.data_as(C.c_void_p),
                                        p1.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p))
    if code != 0:
        raise DspsrAmdError("dspsr_amd_cyclic_binplan failed (%d)" % code)
    return p0, p1, hits


def cyclic_lags_to_spectra(lags: np.ndarray, mover: int = 1) -> np.ndarray:
    """CyclicFoldEngine::synch (CyclicFold.C:450-555): lags float32 [nbin][npol][nchan][nlag][2] -> spectra float32
    [nchan * (2 nlag - 2) / mover][npol][nbin].  The transform runs inside the library (host code, no numpy)."""
    lags = np.ascontiguousarray(lags, dtype=np.float32)
    assert lags.ndim == 5 and lags.shape[4] == 2
    nbin, npol, nchan, nlag = lags.shape[:4]
    if nlag < 2 or mover < 1 or (2 * nlag - 2) % mover:
        raise DspsrAmdError("dspsr_amd_cyclic_lags_to_spectra: nlag=%d, mover=%d" % (nlag, mover))
    out = np.empty((nchan * ((2 * nlag - 2) // mover), npol, nbin), dtype=np.float32)
    code = lib.dspsr_amd_cyclic_lags_to_spectra(lags.ctypes.data_as(C.c_void_p), nchan, npol, nbin, nlag, mover,
                                                out.ctypes.data_as(C.c_void_p))
    if code != 0:
        raise DspsrAmdError("dspsr_amd_cyclic_lags_to_spectra failed (%d): 2*nlag-2 = %d must be a power of two and a "
                            "multiple of mover = %d" % (code, 2 * nlag - 2, mover))
    return out


class CyclicFoldEngine(_Owned):
    """dsp::CyclicFoldEngine (Signal/Pulsar/dsp/CyclicFold.h:93-160); owns the device-resident lag data."""

    _abi = "dspsr_amd_cyclic_fold"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self._create()
        self.shape = None
        self.mover = 1

    def set_shape(self, nchan, npol_in, npol_out, nlag, mover, nbin):
        _check(self.ctx.handle, lib.dspsr_amd_cyclic_fold_set_shape(self.handle, nchan, npol_in, npol_out, nlag, mover, nbin),
               "dspsr_amd_cyclic_fold_set_shape")
        self.shape = (nbin, npol_out, nchan, nlag, 2)
        self.mover = mover

    def set_ndat(self, ndat, idat_start=0):
        _check(self.ctx.handle, lib.dspsr_amd_cyclic_fold_set_ndat(self.handle, ndat, idat_start), "dspsr_amd_cyclic_fold_set_ndat")

    def set_bin(self, idat, ibin, bins_per_sample):
        _check(self.ctx.handle, lib.dspsr_amd_cyclic_fold_set_bin(self.handle, idat, ibin, bins_per_sample),
               "dspsr_amd_cyclic_fold_set_bin")

    def set_bins(self, phi, phase_per_sample, ndat, idat_start=0, hits: np.ndarray | None = None):
        n = C.c_uint64()
        hp = hits.ctypes.data_as(C.c_void_p) if hits is not None else None
        _check(self.ctx.handle, lib.dspsr_amd_cyclic_fold_set_bins(self.handle, phi, phase_per_sample, ndat, idat_start, hp,
                                                                   C.byref(n)), "dspsr_amd_cyclic_fold_set_bins")
        return n.value

    def fold(self, inp):
        """inp: float32 device tensor [nchan][npol_in][>= 2 * (idat_start + ndat)] of complex samples (FPT order)."""
        cs, ps = _strides3(inp)
        _check(self.ctx.handle, lib.dspsr_amd_cyclic_fold_fold(self.handle, inp.data_ptr(), cs, ps), "dspsr_amd_cyclic_fold_fold")

    def zero(self):
        _check(self.ctx.handle, lib.dspsr_amd_cyclic_fold_zero(self.handle), "dspsr_amd_cyclic_fold_zero")

    def get_lagdata_ptr(self):
        return lib.dspsr_amd_cyclic_fold_lagdata_dev(self.handle)

    def synch_lags(self) -> np.ndarray:
        """The lag data on the host, [nbin][npol_out][nchan][nlag][re, im] (blocks)."""
        out = np.empty(self.shape, dtype=np.float32)
        _check(self.ctx.handle, lib.dspsr_amd_cyclic_fold_synch_lags(self.handle, out.ctypes.data_as(C.c_void_p)),
               "dspsr_amd_cyclic_fold_synch_lags")
        return out

    def synch(self) -> np.ndarray:
        """CyclicFoldEngine::synch: spectra [nchan * nchan_spec / mover][npol_out][nbin]."""
        return cyclic_lags_to_spectra(self.synch_lags(), self.mover)


def plfb_check_shape(nchan_in, npol_in, ndim_in, nchan, npol_out, nbin):
    """The refusals of PhaseLockedFilterbankEngine.set_shape, on the host alone (no device)."""
    _host_check(lib.dspsr_amd_plfb_check_shape, nchan_in, npol_in, ndim_in, nchan, npol_out, nbin)


def plfb_check_windows(nchan_in, npol_in, ndim_in, nchan, nbin, in_addr, chan_stride, pol_stride, ndat, idat_start, bins):
    """The refusals of PhaseLockedFilterbankEngine.accumulate, on the host alone (no device)."""
    st = np.ascontiguousarray(idat_start, dtype=np.uint64)
    bn = np.ascontiguousarray(bins, dtype=np.uint32)
    if st.shape != bn.shape or st.ndim != 1:
        raise DspsrAmdError("plfb: idat_start and bin must be one-dimensional and of one length")
    _host_check(lib.dspsr_amd_plfb_check_windows, nchan_in, npol_in, ndim_in, nchan, nbin, in_addr, chan_stride, pol_stride, ndat, st.size,
                st.ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p))


class PhaseLockedFilterbankEngine(_Owned):
    """The loop body of dsp::PhaseLockedFilterbank::transformation (Signal/Pulsar/PhaseLockedFilterbank.C:254-297) on the device;
    owns the device-resident profile [nchan_in * nchan][npol_out][nbin]."""

    _abi = "dspsr_amd_plfb"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self._create()
        self.shape = None

    def set_shape(self, nchan_in, npol_in, ndim_in, nchan, npol_out, nbin):
        _check(self.ctx.handle, lib.dspsr_amd_plfb_set_shape(self.handle, nchan_in, npol_in, ndim_in, nchan, npol_out, nbin),
               "dspsr_amd_plfb_set_shape")
        self.shape = (nchan_in * nchan, npol_out, nbin)

    def accumulate(self, inp, ndat, idat_start, bins):
        """inp: float32 device tensor [nchan_in][npol_in][>= ndat * ndim_in] (FPT order); windows (idat_start[w], bins[w]) in
        time order."""
        st = np.ascontiguousarray(idat_start, dtype=np.uint64)
        bn = np.ascontiguousarray(bins, dtype=np.uint32)
        if st.shape != bn.shape or st.ndim != 1:
            raise DspsrAmdError("plfb: idat_start and bin must be one-dimensional and of one length")
        cs, ps = _strides3(inp)
        _check(self.ctx.handle, lib.dspsr_amd_plfb_accumulate(self.handle, inp.data_ptr(), cs, ps, ndat, st.size,
                                                              st.ctypes.data_as(C.c_void_p), bn.ctypes.data_as(C.c_void_p)),
               "dspsr_amd_plfb_accumulate")

    def zero(self):
        _check(self.ctx.handle, lib.dspsr_amd_plfb_zero(self.handle), "dspsr_amd_plfb_zero")

    def get_profile_ptr(self):
        return lib.dspsr_amd_plfb_profile_dev(self.handle)

    def synch(self) -> np.ndarray:
        """The profile on the host, [nchan_in * nchan][npol_out][nbin] (blocks)."""
        out = np.empty(self.shape, dtype=np.float32)
        _check(self.ctx.handle, lib.dspsr_amd_plfb_synch(self.handle, out.ctypes.data_as(C.c_void_p)), "dspsr_amd_plfb_synch")
        return out


def bandpass_check_shape(nchan_in, npol_in, ndim_in, resolution, npol_out):
    """The refusals of BandpassEngine.set_shape, on the host alone (no device)."""
    _host_check(lib.dspsr_amd_bandpass_check_shape, nchan_in, npol_in, ndim_in, resolution, npol_out)


def bandpass_check_input(nchan_in, npol_in, ndim_in, resolution, raw_layout, in_addr, chan_stride, pol_stride, ndat):
    """The refusals of BandpassEngine.accumulate (raw_layout -1) / accumulate_raw, on the host alone (no device).  Returns the launch
    arithmetic: (parts per workgroup tile, tiles per segment, segments)."""
    tp, tps, nseg = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _host_check(lib.dspsr_amd_bandpass_check_input, nchan_in, npol_in, ndim_in, resolution, raw_layout, in_addr, chan_stride, pol_stride,
                ndat, C.byref(tp), C.byref(tps), C.byref(nseg))
    return tp.value, tps.value, nseg.value


class BandpassEngine(_Owned):
    """dsp::Bandpass::transformation (Signal/General/Bandpass.C:50-175) on the device; owns the device-resident passband
    [npol_out][nchan_in][resolution]."""

    _abi = "dspsr_amd_bandpass"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self._create()
        self.shape = None
        self.integration_samples = 0.0

    def set_shape(self, nchan_in, npol_in, ndim_in, resolution, npol_out):
        _check(self.ctx.handle, lib.dspsr_amd_bandpass_set_shape(self.handle, nchan_in, npol_in, ndim_in, resolution, npol_out),
               "dspsr_amd_bandpass_set_shape")
        self.shape = (npol_out, nchan_in, resolution)

    def accumulate(self, inp, ndat):
        """inp: float32 device tensor [nchan_in][npol_in][>= ndat * ndim_in] (FPT order), any float-aligned address and strides."""
        cs, ps = _strides3(inp)
        _check(self.ctx.handle, lib.dspsr_amd_bandpass_accumulate(self.handle, inp.data_ptr(), cs, ps, ndat),
               "dspsr_amd_bandpass_accumulate")

    def accumulate_raw(self, raw, ndat, layout=_lib.RAW_GENERIC, scale=1.0):
        """raw: the 8-bit block on the device (int8 / uint8 tensor) holding at least ndat samples in `layout` order."""
        _check(self.ctx.handle, lib.dspsr_amd_bandpass_accumulate_raw(self.handle, raw.data_ptr(), layout, scale, ndat),
               "dspsr_amd_bandpass_accumulate_raw")

    def zero(self):
        _check(self.ctx.handle, lib.dspsr_amd_bandpass_zero(self.handle), "dspsr_amd_bandpass_zero")

    def get_pass_ptr(self):
        return lib.dspsr_amd_bandpass_pass_dev(self.handle)

    def synch(self) -> np.ndarray:
        """The passband on the host, [npol_out][nchan_in][resolution] (blocks); integration_samples = samples integrated per row."""
        if self.shape is None:
            raise DspsrAmdError("dspsr_amd_bandpass_synch: no shape")
        out = np.empty(self.shape, dtype=np.float32)
        n = C.c_double()
        _check(self.ctx.handle, lib.dspsr_amd_bandpass_synch(self.handle, out.ctypes.data_as(C.c_void_p), C.byref(n)),
               "dspsr_amd_bandpass_synch")
        self.integration_samples = n.value
        return out


def sk_limits(M: int, std_devs: int = 3):
    """dsp::SKLimits(M, std_devs) rounded to float32 (lower, upper): csrc/host_prep.cpp dspsr_amd_sk_limits, no device."""
    lo, hi = C.c_float(), C.c_float()
    if lib.dspsr_amd_sk_limits(int(M), int(std_devs), C.byref(lo), C.byref(hi)) != _lib.OK:
        raise DspsrAmdError("dspsr_amd_sk_limits: M=%d < 32 or std_devs=%d == 0 (dsp::SKLimits::calc_limits invalid inputs)" % (M, std_devs))
    return np.float32(lo.value), np.float32(hi.value)


class SpectralKurtosisEngine(_Owned):
    """dsp::SpectralKurtosis (Signal/General/SpectralKurtosis.C, the CPU branch) on the device: compute / detect / mask of complex
    rows [nchan][npol][2 * ndat] (FPT, as the filterbank writes them).  The detection steps are those of
    SpectralKurtosis::Engine; transform runs them in the reference's order with the limits of sk_limits."""

    _abi = "dspsr_amd_sk"
    ZAP_ALL, ZAP_SKFB, ZAP_FSCR, ZAP_TSCR = 0, 1, 2, 3

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self._create()
        self.shape = None

    def _call(self, name, *args):
        _check(self.ctx.handle, getattr(lib, name)(self.handle, *args), name)

    def set_shape(self, nchan, npol, M):
        self._call("dspsr_amd_sk_set_shape", nchan, npol, M)
        self.shape = (nchan, npol, M)

    def set_options(self, std_devs=3, chan_start=0, chan_end=0, no_fscr=False, no_tscr=False, no_ft=False):
        self._call("dspsr_amd_sk_set_options", std_devs, chan_start, chan_end, int(no_fscr), int(no_tscr), int(no_ft))

    def compute(self, inp, ndat):
        cs, ps = _strides3(inp)
        self._call("dspsr_amd_sk_compute", inp.data_ptr(), cs, ps, ndat)

    def reset_mask(self):
        self._call("dspsr_amd_sk_reset_mask")

    def detect_tscr(self, lower, upper):
        self._call("dspsr_amd_sk_detect_tscr", lower, upper)

    def detect_skfb(self, lower, upper):
        self._call("dspsr_amd_sk_detect_skfb", lower, upper)

    def detect_fscr(self):
        self._call("dspsr_amd_sk_detect_fscr")

    def count_zapped(self):
        self._call("dspsr_amd_sk_count_zapped")

    def mask(self, inp, out):
        """out may be inp itself: zeros are then written over the zapped parts only."""
        ics, ips = _strides3(inp)
        ocs, ops = _strides3(out)
        self._call("dspsr_amd_sk_mask", inp.data_ptr(), ics, ips, out.data_ptr(), ocs, ops)

    def transform(self, inp, out, ndat):
        """compute, detect and mask of ndat samples; returns the samples the output holds, ndat // M * M (it carries zeroed data)."""
        ics, ips = _strides3(inp)
        ocs, ops = _strides3(out)
        self._call("dspsr_amd_sk_transform", inp.data_ptr(), ics, ips, out.data_ptr(), ocs, ops, ndat)
        return self.npart * self.shape[2]

    def reset_count(self):
        self._call("dspsr_amd_sk_reset_count")

    @property
    def npart(self) -> int:
        return int(lib.dspsr_amd_sk_npart(self.handle))

    def get_estimates_ptr(self):
        return lib.dspsr_amd_sk_estimates_dev(self.handle)

    def get_estimates_tscr_ptr(self):
        return lib.dspsr_amd_sk_estimates_tscr_dev(self.handle)

    def get_zapmask_ptr(self):
        return lib.dspsr_amd_sk_zapmask_dev(self.handle)

    def _fetch(self, ptr, shape, dtype):
        out = np.empty(shape, dtype)
        if out.size:
            _check(self.ctx.handle, lib.dspsr_amd_copy(self.ctx.handle, out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, _lib.D2H), "dspsr_amd_copy")
        return out

    def estimates(self) -> np.ndarray:
        """The estimates of the last compute on the host, float32 [npart][nchan][npol] (blocks)."""
        nchan, npol, _ = self.shape
        return self._fetch(self.get_estimates_ptr(), (self.npart, nchan, npol), np.float32)

    def estimates_tscr(self) -> np.ndarray:
        nchan, npol, _ = self.shape
        return self._fetch(self.get_estimates_tscr_ptr(), (nchan, npol), np.float32)

    def zapmask(self) -> np.ndarray:
        """The mask of the last detection on the host, uint8 [npart][nchan] (blocks)."""
        return self._fetch(self.get_zapmask_ptr(), (self.npart, self.shape[0]), np.uint8)

    def get_statistics(self) -> dict:
        """The counters of SpectralKurtosis (blocks): zap_counts[all, skfb, fscr, tscr], npart_total, unfiltered_hits,
        filtered_hits[nchan], filtered_sum / unfiltered_sum[nchan][npol]."""
        if self.shape is None:
            raise DspsrAmdError("dspsr_amd_sk_get_statistics: no shape")
        nchan, npol, _ = self.shape
        counts, hits = np.zeros(6, np.uint64), np.zeros(nchan, np.uint64)
        fsum, usum = np.zeros((nchan, npol), np.float32), np.zeros((nchan, npol), np.float32)
        self._call("dspsr_amd_sk_get_statistics", *(a.ctypes.data_as(C.c_void_p) for a in (counts, hits, fsum, usum)))
        return {"zap_counts": counts[:4].copy(), "npart_total": int(counts[4]), "unfiltered_hits": int(counts[5]),
                "filtered_hits": hits, "filtered_sum": fsum, "unfiltered_sum": usum}


class Communicator(_Owned):
    """The sub-integration exchange over RCCL / xGMI behind the C-ABI (dspsr_amd_comm_*, csrc/comm.hip): the same entry
    points DSPSR's C++ host calls.  One per pipeline context.  `unique_id` = the 128 bytes of `Communicator.unique_id()`
    made on rank 0 and handed to every rank by the host (bench.py: torch.distributed's store; DSPSR: its MPI transport).
    The Python host shares PyTorch's ROCm runtime (see _lib.load), so the RCCL opened is the one PyTorch ships."""

    _abi = "dspsr_amd_comm"
    SUM, GATHER = _lib.REDUCE_SUM, _lib.REDUCE_GATHER

    @staticmethod
    def _use_torch_rccl():
        try:
            import torch
            path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
            if os.path.exists(path):
                lib.dspsr_amd_comm_set_library(path.encode())
        except ImportError:
            pass

    @staticmethod
    def unique_id() -> bytes:
        Communicator._use_torch_rccl()
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        if lib.dspsr_amd_comm_unique_id(buf) != 0:
            raise DspsrAmdError("dspsr_amd_comm_unique_id: RCCL not available")
        return buf.raw

    def __init__(self, ctx: Context, nranks: int, rank: int, unique_id: bytes):
        Communicator._use_torch_rccl()
        assert len(unique_id) == _lib.UNIQUE_ID_BYTES
        super().__init__(ctx)
        self._create(nranks, rank, unique_id)
        self.nranks, self.rank = nranks, rank
        self._shape = None

    def start(self, mode, profile_ptr, span, nrow, row_floats, hits, integration_length, ndat_total, root=0, check_hits=False):
        """Snapshot + collective, asynchronous: the caller may zero the profile and go on at once."""
        hits = np.ascontiguousarray(hits, dtype=np.uint32)
        _check(self.ctx.handle,
               lib.dspsr_amd_reduce_profiles_start(self.handle, mode, root, profile_ptr, span, nrow, row_floats,
                                                   hits.ctypes.data_as(C.c_void_p), hits.size, float(integration_length),
                                                   int(ndat_total), 1 if check_hits else 0), "dspsr_amd_reduce_profiles_start")
        self._shape = (mode, root, nrow * row_floats, hits.size)

    def finish(self, copy=True):
        """Waits.  Returns (profile, hits, integration_length, ndat_total, hits_identical): numpy arrays on the root
        (profile flat: the SUM, or the nranks slices in rank order), None for the first four elsewhere.
        copy=False: `profile` is a view of the communicator's pinned host buffer (valid until the next start) -- what a writer
        that consumes the sub-integration at once wants."""
        mode, root, n, nbin = self._shape
        same = C.c_int(1)
        if self.rank != root:
            _check(self.ctx.handle, lib.dspsr_amd_reduce_profiles_finish(self.handle, None, None, None, None, C.byref(same)),
                   "dspsr_amd_reduce_profiles_finish")
            return None, None, None, None, bool(same.value)
        hits = np.empty(nbin, np.uint32)
        length, ndat = C.c_double(), C.c_uint64()
        _check(self.ctx.handle,
               lib.dspsr_amd_reduce_profiles_finish(self.handle, None, hits.ctypes.data_as(C.c_void_p),
                                                    C.byref(length), C.byref(ndat), C.byref(same)), "dspsr_amd_reduce_profiles_finish")
        nf = C.c_uint64()
        ptr = lib.dspsr_amd_reduce_profiles_result(self.handle, C.byref(nf))
        prof = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(nf.value,))
        return (prof.copy() if copy else prof), hits, length.value, ndat.value, bool(same.value)
