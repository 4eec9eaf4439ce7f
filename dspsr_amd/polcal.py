"""Phase-coherent polarimetric calibration (`dspsr -pac`): the host side of the matrix response.

The reference multiplies a PolnCalibration response (one Jones matrix per spectral bin, from PSRCHIVE's Pulsar::Database /
PolnCalibrator) with the Dedispersion chirp as a ResponseProduct (LoadToFold1.C:270-289) and the filterbank applies the product
inside its response multiply (Filterbank.C:186-206,574-656; Response::operate(data1, data2), Response.C:515-585).  PSRCHIVE is
not part of this tree, so the calibrator solution enters as DATA -- frequencies and Jones matrices -- and this module builds
what dspsr_amd_filterbank_set_response_matrix takes: float32 [N][8], N = nchan * freq_res, each matrix in the reference's
element order f11, f21, f22, f12 (Response::set(vector<Jones>), Response.C:614-640), bins in the order the engine takes the
chirp.

Deviation from the reference, stated: `jones_response` takes for every bin the matrix of the calibrator channel NEAREST in
frequency (piecewise constant).  The reference asks the calibrator for a solution at the response's own resolution
(pcal->set_response_nchan(ndat), PolnCalibration.C:130-155): interpolation code of PSRCHIVE, external to both trees.
"""
from __future__ import annotations

import numpy as np

from .engine import DspsrAmdError

# Response.C:629-631: for j in 0..1, for i in 0..1: response(row (i + j) % 2, column j)
JONES_ORDER = ((0, 0), (1, 0), (1, 1), (0, 1))        # f11, f21, f22, f12


def load_calibrator(path):
    """A calibrator solution from an .npz file: `freq` (MHz, centre of each calibrator channel, any order) and `jones`
    ([n][2][2] complex).  Returns (freq float64 [n], jones complex128 [n][2][2])."""
    with np.load(path) as z:
        if "freq" not in z.files or "jones" not in z.files:
            raise DspsrAmdError("dspsr_amd.polcal.load_calibrator: %s must hold the arrays 'freq' and 'jones'" % (path,))
        freq, jones = np.asarray(z["freq"], dtype=np.float64), np.asarray(z["jones"], dtype=np.complex128)
    return _check_calibrator(freq, jones)


def _check_calibrator(freq, jones):
    freq = np.asarray(freq, dtype=np.float64).reshape(-1)
    jones = np.asarray(jones, dtype=np.complex128)
    if freq.size == 0 or jones.shape != (freq.size, 2, 2):
        raise DspsrAmdError("dspsr_amd.polcal: calibrator needs freq [n] and jones [n][2][2] with n >= 1 (got %s and %s)"
                            % (freq.shape, jones.shape))
    if not (np.isfinite(freq).all() and np.isfinite(jones).all()):
        raise DspsrAmdError("dspsr_amd.polcal: calibrator holds non-finite values")
    return freq, jones


def _attr(obs, name, default):
    return getattr(obs, name, default)


def response_bin_frequencies(obs, nchan, freq_res):
    """Sky frequency of every response bin of a filterbank that divides the single input channel of `obs` into `nchan` channels
    with `freq_res` bins each, in the order the engine takes the chirp: (chan_centre_MHz[N], offset_MHz[N]), N = nchan * freq_res;
    the frequency of bin j is chan_centre[j] + offset[j].

    SURVEY Appendix A.1 (Dedispersion.C:478-556): chanwidth = bw / nchan, binwidth = chanwidth / freq_res,
    lower = f0 - bw / 2 (+ chanwidth / 2 unless dc_centred); bin k of channel c has the centre lower + c * chanwidth and the offset
    k * binwidth - chanwidth / 2.  Appendix A.3 (Response::match, Response.C:132-181): real (Nyquist) input keeps that order;
    complex single-channel input is dual sideband (Observation.C:80-87) and the two halves of the whole response are swapped.
    `obs` needs centre_frequency, bandwidth (signed, MHz) and ndim (1 real, 2 complex); nchan (default 1), dc_centred (default
    False) and dual_sideband (-1: from the state) are read when present.  Several input channels, and `swap`, are other
    permutations of A.3: refused, not guessed."""
    nchan, freq_res = int(nchan), int(freq_res)
    if nchan < 1 or freq_res < 1:
        raise DspsrAmdError("dspsr_amd.polcal.response_bin_frequencies: nchan=%d and freq_res=%d must be positive" % (nchan, freq_res))
    if int(_attr(obs, "nchan", 1)) != 1:
        raise DspsrAmdError("dspsr_amd.polcal.response_bin_frequencies: input_nchan=%d: the matrix response takes one input channel "
                            "(Filterbank.C:199-201)" % int(_attr(obs, "nchan", 1)))
    if _attr(obs, "swap", False):
        raise DspsrAmdError("dspsr_amd.polcal.response_bin_frequencies: a swapped band (Observation::swap) is not restated here")
    f0, bw = float(obs.centre_frequency), float(obs.bandwidth)
    if bw == 0.0:
        raise DspsrAmdError("dspsr_amd.polcal.response_bin_frequencies: bandwidth = 0")
    chanwidth = bw / float(nchan)
    binwidth = chanwidth / float(freq_res)
    lower = f0 - 0.5 * bw
    if not _attr(obs, "dc_centred", False):
        lower += 0.5 * chanwidth
    centre = np.repeat(lower + np.arange(nchan, dtype=np.float64) * chanwidth, freq_res)
    offset = np.tile(np.arange(freq_res, dtype=np.float64) * binwidth - 0.5 * chanwidth, nchan)
    ds = int(_attr(obs, "dual_sideband", -1))
    dual = (ds == 1) if ds != -1 else int(obs.ndim) == 2
    if dual:                                         # Response::doswap(1): the halves of the whole response change places
        n = nchan * freq_res
        if n % 2:
            raise DspsrAmdError("dspsr_amd.polcal.response_bin_frequencies: a dual-sideband response needs an even number of bins")
        centre = np.concatenate((centre[n // 2:], centre[:n // 2]))
        offset = np.concatenate((offset[n // 2:], offset[:n // 2]))
    return centre, offset


def jones_response(freq, jones, obs, nchan, freq_res):
    """The calibrator as a matrix response: float32 [N][8], bin j = the Jones matrix of the calibrator channel nearest in
    frequency to response_bin_frequencies(obs, nchan, freq_res)[j] (ties: the lower calibrator frequency), written f11, f21,
    f22, f12."""
    freq, jones = _check_calibrator(freq, jones)
    centre, offset = response_bin_frequencies(obs, nchan, freq_res)
    sky = centre + offset
    order = np.argsort(freq, kind="stable")
    fs = freq[order]
    hi = np.clip(np.searchsorted(fs, sky, side="left"), 1, fs.size - 1) if fs.size > 1 else np.zeros(sky.size, dtype=np.int64)
    lo = np.maximum(hi - 1, 0)
    pick = np.where(np.abs(sky - fs[lo]) <= np.abs(fs[hi] - sky), lo, hi)
    j = jones[order[pick]]
    out = np.empty((sky.size, 8), dtype=np.float32)
    for e, (r, c) in enumerate(JONES_ORDER):
        out[:, 2 * e] = j[:, r, c].real
        out[:, 2 * e + 1] = j[:, r, c].imag
    return out


def response_product(matrix8, chirp):
    """Response::operator*= of a matrix response with a scalar one (Response.C:73-104): each of the four elements of bin j times
    chirp[j], in float32 by the formula of Response.C:429-441 (re = f_r d_r - f_i d_i, im = f_i d_r + f_r d_i with f the chirp).
    matrix8: float32 [N][8]; chirp: complex64 [N].  Bin 0 of a dedispersion chirp is zero, so bin 0 of the product is."""
    m = np.ascontiguousarray(matrix8, dtype=np.float32)
    k = np.ascontiguousarray(chirp, dtype=np.complex64).reshape(-1)
    if m.ndim != 2 or m.shape[1] != 8 or m.shape[0] != k.size:
        raise DspsrAmdError("dspsr_amd.polcal.response_product: matrix response %s and chirp of %d bins do not match" % (m.shape, k.size))
    f_r, f_i = k.real.astype(np.float32)[:, None], k.imag.astype(np.float32)[:, None]
    d_r, d_i = m[:, 0::2], m[:, 1::2]
    out = np.empty_like(m)
    out[:, 0::2] = f_r * d_r - f_i * d_i
    out[:, 1::2] = f_i * d_r + f_r * d_i
    return out


def identity_calibrator(freq_mhz=0.0):
    """One calibrator channel holding the unit matrix: every bin gets it."""
    return np.array([float(freq_mhz)]), np.eye(2, dtype=np.complex128)[None]
