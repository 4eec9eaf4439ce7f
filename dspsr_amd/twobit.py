"""Two-bit voltages: the host side of dsp::TwoBitCorrection (Kernel/Classes/TwoBitCorrection.C, ExcisionUnpacker.C, TwoBitLookup.C)
and of the weights a dsp::WeightedTimeSeries carries from the unpacker to the fold (WeightedTimeSeries.C).

The unpacker estimates the digitised power of every window of `nsample` samples from the number of low-voltage states n_low, takes
the window's output levels (lo, hi) from the Jenet & Anderson (1998) dynamic-level-setting table and zeroes and flags the windows
whose n_low lies outside [nlow_min, nlow_max].  The counting and the unpacking run on the device (csrc/twobit.hip); what needs no
device is here: the limits, the level table, and the three weight operations between the unpacker and the fold.  Pure Python.

Parity is unpinned at one boundary, as it is for the 8-bit spacing: mean_Phi, var_Phi and the (lo, hi) pair come from
PSRCHIVE's JenetAnderson98 class, which is not in the reference tree.  The definitions below are the paper's:
    mean_Phi = erf(t / sqrt 2)          the expected fraction of low states for a threshold of t sigma
    var_Phi  = mean_Phi (1 - mean_Phi)
    eq. 41   x = erf^-1(Phi), sigma = t / (sqrt 2 x),
             lo = sigma sqrt(1 - (2 x / sqrt pi) exp(-x^2) / Phi),   hi = sigma sqrt(1 + (2 x / sqrt pi) exp(-x^2) / (1 - Phi))
"""
from __future__ import annotations

import math

import numpy as np

from .engine import DspsrAmdError

# the constants of the feature, in one place
THRESHOLD = 0.9674                    # the optimal two-bit sampling threshold in units of sigma (JA98)
CUTOFF_SIGMA = 10.0                   # ExcisionUnpacker: cutoff_sigma
NSAMPLE = 512                         # ExcisionUnpacker: ndat_per_weight
NSAMPLE_MAX = 65536                   # the longest window dspsr_amd_twobit_unpack takes (csrc/twobit.hip)
OFFSET_BINARY, SIGN_MAGNITUDE, TWOS_COMPLEMENT = 0, 1, 2        # DSPSR_AMD_TWOBIT_*: BitTable::Type


def mean_phi(threshold=THRESHOLD):
    """JenetAnderson98::get_mean_Phi: the expected fraction of samples between -t and +t."""
    return math.erf(threshold / math.sqrt(2.0))


def var_phi(threshold=THRESHOLD):
    m = mean_phi(threshold)
    return m * (1.0 - m)


def limits(nsample, threshold=THRESHOLD, cutoff_sigma=CUTOFF_SIGMA):
    """ExcisionUnpacker::set_limits (ExcisionUnpacker.C:95-158) in the reference's float arithmetic: (nlow_min, nlow_max)."""
    f32 = np.float32
    nsample = int(nsample)
    cutoff = f32(cutoff_sigma)
    if cutoff == 0.0:
        return 0, nsample
    fsample = f32(nsample)
    nlo_mean = f32(float(fsample) * mean_phi(threshold))             # float = float * double
    nlo_variance = f32(float(fsample) * var_phi(threshold))
    if nlo_mean == fsample:
        raise DspsrAmdError("dsp::ExcisionUnpacker::set_limits sampling threshold error: mean nlow=%f == sample size=%f"
                            % (nlo_mean, fsample))
    nlo_sigma = f32(np.sqrt(nlo_variance))
    spread = f32(cutoff * nlo_sigma)
    nlow_max = int(f32(nlo_mean + spread))
    if nlow_max >= nsample:
        nlow_max = nsample - 1
    if float(spread) >= float(nlo_mean) + 1.0:
        nlow_min = 1
    else:
        nlow_min = int(f32(nlo_mean - spread))
    return nlow_min, nlow_max


def erf_inverse(p):
    """x with erf(x) = p, 0 < p < 1: Newton steps on math.erf from a series start."""
    if not 0.0 < p < 1.0:
        raise DspsrAmdError("dspsr_amd.twobit.erf_inverse: %r is outside (0, 1)" % (p,))
    # start: Winitzki's approximation (a few per cent), then Newton on erf(x) - p with erf' = 2/sqrt(pi) exp(-x^2)
    a = 0.147
    ln = math.log(1.0 - p * p)
    t = 2.0 / (math.pi * a) + 0.5 * ln
    x = math.sqrt(math.sqrt(t * t - ln / a) - t)
    for _ in range(60):
        step = (math.erf(x) - p) / (2.0 / math.sqrt(math.pi) * math.exp(-x * x))
        x -= step
        if abs(step) <= 1e-17 * abs(x):
            break
    return x


def ja98_levels(phi, threshold=THRESHOLD):
    """JA98 eq. 41 in double: the (lo, hi) output levels for a fraction `phi` of low states."""
    x = erf_inverse(phi)
    sigma = threshold / (math.sqrt(2.0) * x)
    e = (2.0 * x / math.sqrt(math.pi)) * math.exp(-x * x)
    return sigma * math.sqrt(1.0 - e / phi), sigma * math.sqrt(1.0 + e / (1.0 - phi))


def levels(nsample, nlow_min, nlow_max, threshold=THRESHOLD):
    """The (lo, hi) pair TwoBitLookup::lookup_build (TwoBitLookup.C:63-98) obtains for each nlo in [nlow_min, nlow_max]:
    float32 [nlow_max - nlow_min + 1][2].  nlo = 0 uses 1; nlo = nsample uses nsample - 1 (the reference's clamp tests another
    variable and never fires: DESIGN 4.15)."""
    nsample, nlow_min, nlow_max = int(nsample), int(nlow_min), int(nlow_max)
    if not 0 <= nlow_min < nlow_max <= nsample:
        raise DspsrAmdError("dspsr_amd.twobit.levels: 0 <= nlow_min=%d < nlow_max=%d <= nsample=%d must hold"
                            % (nlow_min, nlow_max, nsample))
    out = np.empty((nlow_max - nlow_min + 1, 2), dtype=np.float32)
    for k, nlo in enumerate(range(nlow_min, nlow_max + 1)):
        use = min(max(nlo, 1), nsample - 1)
        p_in = np.float32(use) / np.float32(nsample)                 # float p_in = (float) use_nlow / (float) ndat
        out[k] = ja98_levels(float(p_in), threshold)
    return out


def get_nweights(nsamples, ndat_per_weight):
    """WeightedTimeSeries::get_nweights(nsamples) (:156-170)."""
    if ndat_per_weight == 0:
        return 0
    return -(-int(nsamples) // int(ndat_per_weight))


def _row(weights, who):
    w = np.array(weights, dtype=np.uint32)
    if w.ndim != 1:
        raise DspsrAmdError("dspsr_amd.twobit.%s: one row of weights expected, got shape %s" % (who, w.shape))
    return w


def mask_weights(weights):
    """WeightedTimeSeries::mask_weights (:539-575) on uint32 [npart][nweights]: a weight that is zero in any row becomes zero in
    every row.  Returns the new array."""
    w = np.array(weights, dtype=np.uint32)
    if w.ndim != 2:
        raise DspsrAmdError("dspsr_amd.twobit.mask_weights: [npart][nweights] expected, got shape %s" % (w.shape,))
    nparts, nweights = w.shape
    for ipart in range(1, nparts):                       # collect all of the bad weights in the first array
        for iwt in range(nweights):
            if w[ipart, iwt] == 0:
                w[0, iwt] = 0
    for ipart in range(1, nparts):                       # distribute the bad weights to all of the arrays
        for iwt in range(nweights):
            if w[0, iwt] == 0:
                w[ipart, iwt] = 0
    return w


def convolve_weights(weights, ndat, ndat_per_weight, weight_idat, nfft, nkeep):
    """WeightedTimeSeries::convolve_weights (:581-697) on one row: every transform of nfft samples (nkeep apart) that touches a
    zero weight is flagged over the samples it delivers -- the previous transform is flagged, then the next is tested.
    Returns (new row, ndat_per_weight, weight_idat)."""
    w = _row(weights, "convolve_weights")
    ndat, ndat_per_weight, weight_idat, nfft, nkeep = int(ndat), int(ndat_per_weight), int(weight_idat), int(nfft), int(nkeep)
    if ndat_per_weight >= nfft:                          # the fft happens within one weight
        return w, ndat_per_weight, weight_idat
    if ndat + nkeep < nfft:
        return w, ndat_per_weight, weight_idat
    nweights_tot = get_nweights(ndat + weight_idat, ndat_per_weight)
    if ndat_per_weight == 0:
        return w, ndat_per_weight, weight_idat
    if w.size < nweights_tot:
        raise DspsrAmdError("dspsr_amd.twobit.convolve_weights: %d weights given, ndat=%d + weight_idat=%d need %d"
                            % (w.size, ndat, weight_idat, nweights_tot))
    weights_per_dat = 1.0 / ndat_per_weight
    blocks = (ndat + nkeep - nfft) // nkeep
    end_idat = blocks * nkeep
    zero_start = zero_end = 0
    for start_idat in range(0, end_idat, nkeep):
        wt_idat = start_idat + weight_idat
        start_weight = int(wt_idat * weights_per_dat)
        end_weight = int(math.ceil((wt_idat + nfft) * weights_per_dat))
        if end_weight > nweights_tot:
            raise DspsrAmdError("dsp::WeightedTimeSeries::convolve_weights end_weight=%d > nweights=%d \n\tblocks=%d end_idat=%d"
                                % (end_weight, nweights_tot, blocks, end_idat))
        zero_weights = 0
        for iweight in range(start_weight, end_weight):
            if w[iweight] == 0:
                zero_weights += 1
        for iweight in range(zero_start, zero_end):      # flag the previous transform ...
            w[iweight] = 0
        if zero_weights == 0:                            # ... then set the flag for the next loop
            zero_start = zero_end = 0
        else:
            zero_start = start_weight
            zero_end = int(math.ceil((start_idat + nkeep) * weights_per_dat))
    for iweight in range(zero_start, zero_end):
        w[iweight] = 0
    return w, ndat_per_weight, weight_idat


def scrunch_weights(weights, ndat_per_weight, weight_idat, nscrunch, ndat=None):
    """WeightedTimeSeries::scrunch_weights (:703-775) on one row: the time resolution drops by `nscrunch`.  While a weight still
    covers one output sample or more only ndat_per_weight and weight_idat change; below that, groups of nscrunch weights are
    averaged (zero if any is zero) and ndat_per_weight becomes 1 (weight_idat stays, as in the reference).  ndat: the samples
    the row covers (default: every weight given counts).  Returns (new row, ndat_per_weight, weight_idat)."""
    w = _row(weights, "scrunch_weights")
    ndat_per_weight, weight_idat, nscrunch = int(ndat_per_weight), int(weight_idat), int(nscrunch)
    if not ndat_per_weight:
        return w, ndat_per_weight, weight_idat
    nweights_tot = w.size if ndat is None else get_nweights(int(ndat) + weight_idat, ndat_per_weight)
    points_per_weight = float(ndat_per_weight) / float(nscrunch)
    if points_per_weight >= 1.0:
        ndat_per_weight = int(points_per_weight)
        leftover = weight_idat % ndat_per_weight != 0
        weight_idat //= ndat_per_weight
        if leftover:
            weight_idat += 1
        return w, ndat_per_weight, weight_idat
    new_nweights, extra = divmod(nweights_tot, nscrunch)
    if extra:
        new_nweights += 1
    for iwt in range(new_nweights):
        base = iwt * nscrunch
        if (iwt + 1) * nscrunch > nweights_tot:
            nscrunch = extra
        acc = 0
        for ivt in range(nscrunch):
            if w[base + ivt] == 0:
                acc = 0
                break
            acc = int(w[base + ivt]) if ivt == 0 else acc + int(w[base + ivt])
        w[iwt] = acc // nscrunch
    return w[:new_nweights].copy(), 1, weight_idat
