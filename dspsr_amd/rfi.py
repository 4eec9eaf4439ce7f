"""`dspsr -R`: the narrow-band RFI filter, dsp::RFIFilter (Signal/General/RFIFilter.C).

The filter is a Response: a 0/1 mask over `nchan_bandpass` channels of the band, multiplied into the dedispersion kernel
(ResponseProduct, LoadToFold1.C:248-266) and handed to the filterbank through its ordinary set_kernel.  The mask comes from the
passband of the first `interval` seconds of the stream, integrated on the device by BandpassEngine (dsp::Bandpass); everything else is
the reference's host code, restated in csrc/host_prep.cpp.

Two facts about the reference, decided here:
  * RFIFilter::calculate (:139-158) leaves a mask of all ones whatever the data: every round sets a channel that does not trigger to
    1, also one zapped in an earlier round, and the loop ends only after a round without a trigger.  `keep_zapped=True` (the default,
    what Config.zap_rfi uses) keeps a channel zapped in any round at 0; `keep_zapped=False` is the literal loop.
  * The filter is not time-variable: Filterbank and Convolution match their response once, in prepare (Filterbank.C:84,
    Convolution.C:115), so the mask is that of the first interval.  The same here.
The mask is in forward-transform bin order and is never swapped: RFIFilter::match(const Observation*, unsigned) overrides
Response::match and does no doswap."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .engine import BandpassEngine, DspsrAmdError, eight_bit_scale
from .inputs import raw_form

BLOCK = 8 * 1024                      # RFIFilter.C:26: maximum_block_size, the unit the reference reads the interval in


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


def mask_calculate(p0, p1, median_window=51, keep_zapped=True, allow_endless=False):
    """RFIFilter::calculate (:105-162) on the passbands of the two polarisations.  Returns a dict: mask (float32 0/1), p0, p1 (copies,
    zeroed where zapped), total_zapped (re-zaps counted), rounds, cutoffs (one per round), endless.  Where the reference's loop would
    not end (a round of re-zaps only: a cutoff below zero) the library stops; that raises, or with allow_endless returns the
    state of that round with endless = True."""
    p0 = np.array(p0, dtype=np.float32).ravel()
    p1 = np.array(p1, dtype=np.float32).ravel()
    if p0.shape != p1.shape or not p0.size:
        raise DspsrAmdError("dspsr_amd.rfi.mask_calculate: p0 and p1 must be of one length > 0")
    n = p0.size
    mask = np.empty(n, dtype=np.float32)
    cut = np.zeros(n + 2, dtype=np.float32)
    total, rounds = C.c_uint32(), C.c_uint32()
    rc = lib.dspsr_amd_rfi_mask_calculate_log(_fp(p0), _fp(p1), n, int(median_window), 1 if keep_zapped else 0, _fp(mask),
                                              C.byref(total), C.byref(rounds), _fp(cut), cut.size)
    if rc == _lib.ESTATE and not allow_endless:
        raise DspsrAmdError("dsp::RFIFilter::calculate round %d (cutoff = %g) re-zapped channels and zapped no new one: the "
                            "reference's loop does not end" % (rounds.value, cut[min(rounds.value, cut.size) - 1]))
    if rc not in (_lib.OK, _lib.ESTATE):
        raise DspsrAmdError("dspsr_amd_rfi_mask_calculate failed (%d)" % rc)
    return {"mask": mask, "p0": p0, "p1": p1, "total_zapped": total.value, "rounds": rounds.value, "endless": rc == _lib.ESTATE,
            "cutoffs": cut[:min(rounds.value, cut.size)].copy()}


def mask_expand(mask, required):
    """RFIFilter::match(const Response*) (:165-206): complex64 [required]."""
    mask = np.ascontiguousarray(mask, dtype=np.float32).ravel()
    out = np.empty(int(required), dtype=np.complex64)
    rc = lib.dspsr_amd_rfi_mask_expand(_fp(mask), mask.size, int(required), _fp(out))
    if rc != _lib.OK:
        raise DspsrAmdError("dspsr_amd_rfi_mask_expand failed (%d)" % rc)
    return out


def response_multiply(kernel, phasors):
    """Response::operator *= : a new complex64 array kernel x phasors."""
    out = np.array(kernel, dtype=np.complex64).ravel()
    ph = np.ascontiguousarray(phasors, dtype=np.complex64).ravel()
    if out.size != ph.size:
        raise DspsrAmdError("dsp::Response::operator *= ndat*nchan=%d != other ndat*nchan=%d" % (out.size, ph.size))
    rc = lib.dspsr_amd_response_multiply(_fp(out), _fp(ph), out.size)
    if rc != _lib.OK:
        raise DspsrAmdError("dspsr_amd_response_multiply failed (%d)" % rc)
    return out


def report_lines(result):
    """What the reference prints to stderr (:142, :160)."""
    lines = ["\tround %d cutoff = %g" % (k + 1, c) for k, c in enumerate(result["cutoffs"])]
    lines.append("\tzapped %d channels" % result["total_zapped"])
    return lines


class RfiFilter:
    """dsp::RFIFilter with its dsp::Bandpass on the device.  `info`: the pipeline's InputInfo (rate, nchan, npol, ndim, machine)."""

    def __init__(self, ctx, info, nchan_bandpass=1024, interval=1.0, median_window=51, keep_zapped=True, log=None):
        if info.npol != 2:
            raise DspsrAmdError("dsp::RFIFilter::calculate reads the passbands of two polarisations (npol=%d)" % info.npol)
        nsamp_fft = nchan_bandpass * (2 if info.ndim == 1 else 1)
        if nsamp_fft < 1 or BLOCK % nsamp_fft:
            raise DspsrAmdError("dsp::Bandpass::transformation error ndat=%d < nfft=%d: the filter reads blocks of %d samples, "
                                "which must hold whole transforms" % (BLOCK, nsamp_fft, BLOCK))
        self.ctx, self.info = ctx, info
        self.nchan_bandpass, self.interval, self.median_window, self.keep_zapped = nchan_bandpass, float(interval), median_window, keep_zapped
        self.log = log
        self.bandpass = BandpassEngine(ctx)
        self.bandpass.set_shape(info.nchan, info.npol, info.ndim, nchan_bandpass, info.npol)
        self.form = raw_form(info)
        self.layout = self.form.layout
        self.scale8 = eight_bit_scale()
        self.integration_length = 0.0
        self.result = None
        self.mask = None
        self.passband = None                        # the integrated passband [npol][nchan][nchan_bandpass] calculate() read

    def _take(self, ndat):
        """whole 8192-sample blocks of `ndat` offered samples that the reference's loop (:91-95) would still read"""
        blocks, length = 0, self.integration_length
        while length < self.interval and (blocks + 1) * BLOCK <= ndat:
            blocks += 1
            length += float(BLOCK) / self.info.rate                            # Bandpass.C:164, one block at a time
        self.integration_length = length
        return blocks * BLOCK

    def integrate_raw(self, raw_dev, ndat):
        """Adds the 8-bit block (device tensor in the stream's layout, `ndat` samples from its first) until integration_length >=
        interval; excess input is not used.  Returns the samples used, a whole number of 8192-sample blocks."""
        if self.form.name == "heaps":
            raise DspsrAmdError("dspsr_amd.rfi.RfiFilter.integrate_raw: the heaps of INSTRUMENT %s are not read here (the Bandpass operator "
                                "takes the generic and CASPSR byte orders): unpack with dspsr_amd.unpack_heaps_fpt and call integrate"
                                % self.info.machine)
        used = self._take(ndat)
        if used:
            self.bandpass.accumulate_raw(raw_dev, used, self.layout, self.scale8)
            self.result = None
        return used

    def integrate(self, rows, ndat):
        """The same from unpacked float rows [nchan][npol][>= ndat * ndim]."""
        used = self._take(ndat)
        if used:
            self.bandpass.accumulate(rows, used)
            self.result = None
        return used

    @property
    def complete(self):
        return self.integration_length >= self.interval

    def calculate(self):
        """Waits for the passband, runs RFIFilter::calculate on input channel 0 (get_datptr(0, .), :109-110) and returns the mask."""
        if self.integration_length <= 0:
            raise DspsrAmdError("dsp::RFIFilter::calculate no data integrated")
        band = self.bandpass.synch()
        self.passband = band
        self.result = mask_calculate(band[0, 0], band[1, 0], self.median_window, self.keep_zapped)
        self.mask = self.result["mask"]
        if self.log is not None:
            for line in report_lines(self.result):
                print(line, file=self.log)
        return self.mask

    def product(self, kernel, nchan, ndat):
        """kernel x expand(mask): the ResponseProduct for a response of nchan channels of ndat points."""
        if self.result is None:
            self.calculate()
        return response_multiply(kernel, mask_expand(self.mask, int(nchan) * int(ndat)))

    def close(self):
        """Frees the device passband; the mask, the result and the passband's host copy stay (product() goes on working once
        calculated)."""
        self.bandpass.close()
