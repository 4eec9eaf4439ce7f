"""Host pipeline for the hot path: the caller of the engines, mirroring what
dsp::LoadToFold / SingleThread::run do around them (Signal/Pulsar/LoadToFold1.C:117-880,
Signal/General/SingleThread.C:355-497):

  per block:  Filterbank (+ fused Detection) -> Fold::fold plan + accumulate
  per sub-integration (Subint<Fold>, Signal/Pulsar/dsp/Subint.h:234-309): emit + zero the profile;
      with more than one rank this is where the single RCCL reduce of the per-sub-band
      profiles happens (PhaseSeries::combine semantics, PhaseSeries.C:442-484).

Only plumbing lives here; all arithmetic on samples is done by libdspsr_amd.so.
"""
from __future__ import annotations

import math
import os
import sys
import dataclasses
from dataclasses import dataclass

import numpy as np

from . import _lib
from .engine import (Context, ConvolutionEngine, CyclicFoldEngine, Dedispersion, DetectionEngine, DspsrAmdError, SpectralKurtosisEngine, FilterbankEngine, FITSDigitizer, FoldEngine, PhaseLockedFilterbankEngine, plfb_check_shape, Rescale, SampleDelay, add_fpt, copy_data_fpt, fourth_moment, unpack_sigproc_fpt,
                     dedispersion_sample_delays, detect_raw, eight_bit_scale, fscrunch_fpt, pscrunch_tfp, sigproc_digitize, sigproc_digitize_fpt,
                     tfp_filterbank, tscrunch_fpt)
from .inputs import FORMS, VOLTAGES, raw_form, refuse_forms


def move_tail_fpt(ctx, buf, dst, src, n, unit=1):
    """InputBuffering's carry inside one buffer: samples [src, src + n) of the rows of `buf` ([nchan][npol][nsample * unit]) go to
    [dst, dst + n), dst < src.  The ranges overlap when fewer samples were consumed than are carried (a short block of -K):
    copy_data_fpt is a parallel copy and refuses overlapping rows, so the move is made in ascending, stream-ordered chunks of at
    most src - dst samples -- each chunk lands on samples that earlier chunks have already moved."""
    if not 0 <= dst < src:
        raise DspsrAmdError("dspsr_amd.move_tail_fpt: destination %d must lie in front of the source %d" % (dst, src))
    shift = src - dst
    for k in range(0, n, shift):
        m = min(shift, n - k)
        copy_data_fpt(ctx, buf[:, :, (dst + k) * unit:(dst + k + m) * unit], buf[:, :, (src + k) * unit:(src + k + m) * unit])


@dataclass
class Config:
    """The dspsr command-line options that matter on this path (dspsr.C:207-510)."""
    nchan: int = 1024                 # -F nchan:D
    dispersion_measure: float = 1000  # -D
    nbin: int = 1024                  # -b
    folding_period: float = 0.0       # -c  (seconds); 0 => polyco
    freq_res: int = 0                 # -x  (0 => optimal)
    subint_seconds: float = 0.0       # -L  (0 => single integration)
    subint_turns: float = 0.0         # -s (1 turn: single pulses) / -turns N: sub-integrations of N pulse periods
    fractional_pulses: bool = False   # -fractional_pulses: start the first division at the first sample, not at phase 0
    stokes: bool = False              # -4? (default Coherence, LoadToFold1.C:1119-1134)
    ndim: int = 4                     # detected layout (CPU default 4, CUDA engine 2; LoadToFoldConfig.C:104)
    parts_per_block: int = 64         # block size in overlap-save parts (LoadToFold1.C:825-835 sizes blocks likewise)
    max_parts: int = 32               # parts per launch group (persistent kernels: 32 amortise ramp-up and tail)
    fused_fold: bool = True           # fold inside the last filterbank pass when possible (identical sums, no
                                      # detected time series in HBM); False = Detection and Fold as separate ops
    force_fused: bool = False         # fuse also where the channel tiles do not fill the chip (slower there, same sums)
    two_pass: bool = True             # short responses (complex dual-pol input, nchan_subband * freq_res^2 == 2^27): forward and
                                      # inverse transforms in two workgroup tiles; False = the three-pass kernels (A/B runs)
    interchan_dedispersion: bool = False   # -K: remove the inter-channel dispersion delay (LoadToFold1.C:605-624)
    convolve_when: str = "during"          # -F N:D = "during" (the response inside the filterbank, LoadToFold1.C:318-323); -F N = "after":
                                           # non-convolving filterbank (freq_res 1), then dsp::Convolution on its channels
                                           # (Filterbank::Config::After, FilterbankConfig.C:56, LoadToFold1.C:337-380); -F N:B = "before":
                                           # dsp::Convolution of the whole input channel, then the non-convolving filterbank
                                           # (Config::Before, FilterbankConfig.C:76-78, LoadToFold1.C:326-385); "never": the filterbank
                                           # alone (no coherent dedispersion)
    record_time: bool = False              # -r: time every operation (Operation.C:90-113); each one then ends with a stream
                                           # synchronisation so that the wall times are honest (FilterbankCUDA.cu:302-303)
    cyclic_nchan: int = 0                  # -cyclic N: cyclic spectra of N channels per filterbank channel; dsp::CyclicFold replaces
                                           # Detection + Fold (LoadToFold1.C:534-539,999-1044).  0: off -- today's path, untouched
    cyclic_mover: int = 1                  # -cyclicoversample M: nlag = M * N / 2 + 1 (dsp/CyclicFold.h:66)
    cyclic_npol: int = 0                   # output polarisations of the cyclic fold (the reference passes config->npol): 1, 2 or 4;
                                           # 0 = 4 (Coherence) for two input polarisations, 1 for one
    fourth_moment: bool = False            # -4: fold the Stokes parameters and their ten pairwise products (dsp::FourthMoment,
                                           # LoadToFold1.C:557-568): detection forced to Stokes with ndim 4 (:1119-1123), the fold has
                                           # shape (nchan, 1, 14, nbin), the fused fold is off
    plfb_nbin: int = 0                     # -G nbin: phase-locked filterbank (dsp::PhaseLockedFilterbank replaces Detection + Fold,
                                           # LoadToFold1.C:386-456): pulse-phase-resolved spectra in nbin phase bins.  0: off
    plfb_nchan: int = 0                    # channels per window of -G; 0 = the reference's choice, the largest power of two <=
                                           # period * rate / nbin (PhaseLockedFilterbank.C:65-73); output polarisations = npol (:425)
    calibrator: object = None              # -pac: phase-coherent polarimetric calibration (LoadToFold1.C:270-289).  A path to an .npz
                                           # with `freq` (MHz) and `jones` [n][2][2], or a (freq, jones) pair (polcal.load_calibrator):
                                           # the Jones matrix of every response bin times the chirp goes to the filterbank as a matrix
                                           # response (calibrator_response below says what it works with and what it refuses)
    zap_rfi: bool = False                  # -R: the narrow-band RFI filter (dsp::RFIFilter, LoadToFold1.C:248-266): a 0/1 mask from the
                                           # passband of the first second, multiplied into the dedispersion kernel.  The pipeline wants
                                           # its filter before the first block: LoadToFold.set_rfi_filter (dada.fold_file does it)
    fuse_heaps: bool = True                # MeerKAT heaps (INSTRUMENT MKBF / MKBFRo): True = the one-pass convolution reads the 8-bit
                                           # block itself where the front end has that loader (FilterbankEngine.takes_heaps); False = the
                                           # engine unpacks into float rows first, as it does for every other geometry (A/B runs,
                                           # the same numbers bit for bit)
    npol: int = 4                          # -d: the reference's config->npol, Detection's output (LoadToFold1.C:552-568,1098-1134): 4 the
                                           # four products (Coherence / Stokes, laid out by ndim), 1 Intensity, 2 PPQQ -- rows and profile
                                           # of npol x ndim 1 --, 3 the reference's refusal of NthPower.  1 or 3 win over -4, which is then
                                           # ignored.  One input polarisation folds as PP with any npol but the default 4, which keeps
                                           # its refusal.  -cyclic and -G read it their own way (cyclic_npol, plfb)
    sk_zap: bool = False                   # -skz: spectral-kurtosis RFI excision (dsp::SpectralKurtosis between the filterbank and
                                           # Detection, LoadToFold1.C:458-532; defaults of LoadToFoldConfig.C:71-89).  False: off --
                                           # today's paths, untouched
    sk_m: int = 128                        # -skzm: samples per SK estimate
    sk_std_devs: int = 3                   # -skzs: excision threshold in standard deviations
    sk_chan_start: int = 0                 # -skz_start / -skz_end: channel range of the tscr and fscr detections; taken only when
    sk_chan_end: int = 0                   # start > 0 and end < nchan (LoadToFold1.C:527-528); end 0: nchan
    sk_no_fscr: bool = False               # -skz_no_fscr / -skz_no_tscr / -skz_no_ft: disable one of the three detections
    sk_no_tscr: bool = False
    sk_no_ft: bool = False
    excision_nsample: int = 0              # -2n: samples per window of the two-bit unpacker's power estimate (0: 512); two-bit input only
    excision_threshold: float = -1.0       # -2t: the sampling threshold at record time in sigma (<= 0: 0.9674)
    excision_cutoff: float = -1.0          # -2c: excision cutoff in standard deviations of n_low (< 0: 10; 0: keep every window)
                                           # (LoadToFoldConfig.C:22-28, LoadToFold1.C:731-743)


@dataclass
class FoldTarget:
    """One pulsar of a multi-pulsar run (dspsr -P a.polyco -P b.polyco / -c ... -c ...; LoadToFold1.C:917-960 gives each its own
    Fold, sub-integration divider and unloader)."""
    name: str = ""
    polyco: object = None             # Polyco / ChebyPredictor, or None with folding_period
    folding_period: float = 0.0       # seconds (used when polyco is None)
    reference_phase: float = 0.0
    nbin: int = 0                     # 0: dsp::Fold::choose_nbin for this pulsar's period (Fold.C:291-382, per Fold)


class _PulsarFold:
    """The per-pulsar state of a multi-target LoadToFold: the fold engine and the PhaseSeries bookkeeping."""

    def __init__(self, target, nbin, fold):
        self.target, self.nbin, self.fold = target, nbin, fold
        self.hits = np.zeros(nbin, dtype=np.uint32)
        self.integration_length, self.ndat_total = 0.0, 0
        self.turns = None             # TurnsDivider (-s / -turns: boundaries differ per pulsar)
        self.subints = []


@dataclass
class InputInfo:
    """What ASCIIObservation.C:82-415 reads from the DADA header."""
    centre_frequency: float = 1382.0
    bandwidth: float = -400.0
    nchan: int = 1
    npol: int = 2
    ndim: int = 1
    tsamp_us: float = 0.00125
    machine: str = "CASPSR"
    start_seconds: float = 0.0        # of the first sample, relative to UTC_START
    mjd_day: int = 55299
    mjd_sec: float = 7545.0
    source: str = "unknown"
    telescope: str = "unknown"
    nbit: int = 8                     # NBIT of the file (every path here reads 8-bit samples)
    guppi: tuple | None = None        # a GUPPI raw file (dspsr_amd.guppi.GuppiFile): (block_nsamp, chan_stride, block_stride) of its blocks
    detected: str | None = None       # detected input (a SIGPROC filterbank file, dspsr_amd.sigproc.SigprocFile): the state of its rows --
                                      # "Intensity", "PPQQ" or "Coherence" for npol 1, 2, 4; nchan channels, ndim 1, nbit bits per value

    @property
    def rate(self):
        return 1e6 / self.tsamp_us


class Polyco:
    """TEMPO polyco predictor (the role of Pulsar::Predictor, PSRCHIVE ext): phase and frequency."""

    def __init__(self, text: str):
        tok = text.replace("D", "E").split()
        day, frac = tok[3].split(".")
        ri, rf = tok[7].split(".")
        self.tmid_day, self.tmid_frac = int(day), float("0." + frac)
        self.rphase_int, self.rphase_frac = int(ri), float("0." + rf)
        self.f0 = float(tok[8])
        ncoef = int(tok[11])
        self.coef = [float(t) for t in tok[13:13 + ncoef]]

    def _dt(self, day, sec):
        return ((day - self.tmid_day) + (sec / 86400.0 - self.tmid_frac)) * 1440.0

    def phase_frac(self, day, sec):
        dt = self._dt(day, sec)
        poly = 0.0
        for c in reversed(self.coef):
            poly = poly * dt + c
        spin = 60.0 * dt * self.f0
        ph = (self.rphase_frac + (spin - math.floor(spin))) + poly
        return ph - math.floor(ph)

    def frequency(self, day, sec):
        dt = self._dt(day, sec)
        d = 0.0
        for k in range(len(self.coef) - 1, 0, -1):
            d = d * dt + k * self.coef[k]
        return self.f0 + d / 60.0

    def phase(self, day, sec):
        """Absolute phase as (integer turns, fractional turns) -- Pulsar::Predictor::phase keeps the two apart because
        the total (3.6e9 turns for vela.polyco) does not fit a double to 1e-6 turns."""
        dt = self._dt(day, sec)
        poly = 0.0
        for c in reversed(self.coef):
            poly = poly * dt + c
        spin = 60.0 * dt * self.f0
        si = math.floor(spin)
        fr = self.rphase_frac + (spin - si) + poly
        fi = math.floor(fr)
        return int(self.rphase_int + si + fi), fr - fi

    def iphase(self, phase, day, sec_guess):
        """Pulsar::Predictor::iphase: the epoch (seconds of `day`) at which the phase is `phase` = (int, frac) turns,
        by Newton iteration with slope frequency(t)."""
        sec = sec_guess
        for _ in range(20):
            pi, pf = self.phase(day, sec)
            step = ((pi - phase[0]) + (pf - phase[1])) / self.frequency(day, sec)
            sec -= step
            if abs(step) < 1e-12:
                break
        return sec


class ChebyPredictor:
    """TEMPO2 predictor (`dspsr -P file` with a `ChebyModelSet`; PSRCHIVE `Pulsar::T2Predictor` over tempo2's
    `T2Predictor` library -- both external to the reference tree, `Fold.C:229-262` only asks the generator for one): per
    segment a two-dimensional Chebyshev series in time and observing frequency,
        phase(t, f) = sum'_i sum'_j c[i][j] T_i(x) T_j(y) + DISPERSION_CONSTANT / f^2,
        x = -1 + 2 (t - t0) / (t1 - t0) over TIME_RANGE (MJD),  y = -1 + 2 (f - f0) / (f1 - f0) over FREQ_RANGE (MHz),
    primed sums (first term halved), spin frequency = d phase / dt.  Same duck-typed interface as `Polyco` (phase_frac,
    frequency, phase, iphase), so `LoadToFold(polyco=ChebyPredictor(text))` folds with it.  The constant term (1e9 ... 1e11
    turns) is split into integer and fractional turns from its decimal text, so that the fractional phase keeps double
    precision.  Parity: unpinned (tempo2 is not in the image; the series convention is the one its published
    construction -- coefficients 4/(nx ny) times the cosine sums -- implies)."""

    def __init__(self, text: str, observing_frequency: float | None = None):
        from decimal import Decimal
        self.segments = []
        seg = None
        for line in text.splitlines():
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "ChebyModel" and tok[1] == "BEGIN":
                seg = {"coef": []}
            elif tok[0] == "ChebyModel" and tok[1] == "END":
                nx, ny = seg["nx"], seg["ny"]
                flat = seg.pop("coef")
                if len(flat) != nx * ny:
                    raise DspsrAmdError("ChebyPredictor: %d coefficients, NCOEFF_TIME x NCOEFF_FREQ = %d" % (len(flat), nx * ny))
                # c[i][j]: one COEFFS record per time index i, NCOEFF_FREQ values each; the constant is kept as text
                c00 = Decimal(flat[0]) / 4
                seg["c00_int"] = int(c00 // 1)
                seg["c00_frac"] = float(c00 - (c00 // 1))
                seg["c"] = [[float(flat[i * ny + j]) for j in range(ny)] for i in range(nx)]
                seg["c"][0][0] = 0.0
                self.segments.append(seg)
                seg = None
            elif seg is not None:
                if tok[0] == "TIME_RANGE":
                    seg["t0"], seg["t1"] = self._mjd(tok[1]), self._mjd(tok[2])
                elif tok[0] == "FREQ_RANGE":
                    seg["f0"], seg["f1"] = float(tok[1]), float(tok[2])
                elif tok[0] == "DISPERSION_CONSTANT":
                    seg["dc"] = float(tok[1])
                elif tok[0] == "NCOEFF_TIME":
                    seg["nx"] = int(tok[1])
                elif tok[0] == "NCOEFF_FREQ":
                    seg["ny"] = int(tok[1])
                elif tok[0] == "COEFFS":
                    seg["coef"].extend(tok[1:])
                elif tok[0][0] in "+-.0123456789":       # continuation line of a COEFFS record
                    seg["coef"].extend(tok)
        if not self.segments:
            raise DspsrAmdError("ChebyPredictor: no ChebyModel in the predictor text")
        s0 = self.segments[0]
        self.observing_frequency = observing_frequency if observing_frequency is not None else 0.5 * (s0["f0"] + s0["f1"])

    @staticmethod
    def _mjd(tok):
        day, _, frac = tok.partition(".")
        return int(day), float("0." + (frac or "0"))

    def _segment(self, day, sec):
        t = sec / 86400.0
        for s in self.segments:
            a = (day - s["t0"][0]) + (t - s["t0"][1])
            b = (s["t1"][0] - day) + (s["t1"][1] - t)
            if a >= 0.0 and b >= 0.0:
                return s, a, a + b
        raise DspsrAmdError("ChebyPredictor: MJD %d + %.3f s is outside every TIME_RANGE" % (day, sec))

    def _time_series(self, s):
        """The series in x alone at the observing frequency: a[i] = sum'_j c[i][j] T_j(y); plus the constant parts."""
        key = ("a", self.observing_frequency)
        if s.get("key") != key:
            y = -1.0 + 2.0 * (self.observing_frequency - s["f0"]) / (s["f1"] - s["f0"])
            ty = [1.0, y]
            for j in range(2, s["ny"]):
                ty.append(2.0 * y * ty[-1] - ty[-2])
            s["a"] = [sum((0.5 if j == 0 else 1.0) * s["c"][i][j] * ty[j] for j in range(s["ny"])) for i in range(s["nx"])]
            s["disp"] = s.get("dc", 0.0) / (self.observing_frequency * self.observing_frequency)
            s["key"] = key
        return s["a"]

    def _eval(self, day, sec):
        s, a, span = self._segment(day, sec)
        x = -1.0 + 2.0 * a / span
        co = self._time_series(s)
        tprev, tcur = 1.0, x
        val = 0.5 * co[0] + (co[1] * x if len(co) > 1 else 0.0)
        # derivative with respect to x: T_n' = n U_{n-1};  U_0 = 1, U_1 = 2x, U_n = 2x U_{n-1} - U_{n-2}
        uprev, ucur = 1.0, 2.0 * x
        der = co[1] if len(co) > 1 else 0.0
        for n in range(2, len(co)):
            tprev, tcur = tcur, 2.0 * x * tcur - tprev
            val += co[n] * tcur
            der += co[n] * n * ucur
            uprev, ucur = ucur, 2.0 * x * ucur - uprev
        return s, val + s["disp"], der * 2.0 / (span * 86400.0)

    def phase(self, day, sec):
        s, val, _ = self._eval(day, sec)
        fr = s["c00_frac"] + val
        fi = math.floor(fr)
        return int(s["c00_int"] + fi), fr - fi

    def phase_frac(self, day, sec):
        return self.phase(day, sec)[1]

    def frequency(self, day, sec):
        return self._eval(day, sec)[2]

    def iphase(self, phase, day, sec_guess):
        sec = sec_guess
        for _ in range(20):
            pi, pf = self.phase(day, sec)
            step = ((pi - phase[0]) + (pf - phase[1])) / self.frequency(day, sec)
            sec -= step
            if abs(step) < 1e-12:
                break
        return sec


def choose_nbin(folding_period, rate, requested_nbin=0, maximum_nbin=1024, minimum_bin_width=1.2,
                power_of_two=True, force_sensible_nbin=False):
    """dsp::Fold::choose_nbin (Fold.C:291-382): largest power of two <= period / (1.2 * tsamp), capped at
    maximum_nbin, unless -b requested_nbin was given."""
    if folding_period <= 0.0:
        raise DspsrAmdError("dsp::Fold::choose_nbin invalid folding period=%f" % folding_period)
    ratio = folding_period / (minimum_bin_width / rate)
    sensible = int(2.0 ** math.floor(math.log(ratio) / math.log(2.0))) if power_of_two else int(ratio)
    sensible = max(sensible, 1)
    if requested_nbin > 1:
        return sensible if (force_sensible_nbin and requested_nbin > sensible) else requested_nbin
    return maximum_nbin if (maximum_nbin and sensible > maximum_nbin) else sensible


def subint_bounds(k, division_seconds, rate):
    """[first, last) output sample of division k, with the two roundings of TimeDivide::set_boundaries
    (TimeDivide.C:503-540): lower = lrint(k*L*rate); division_ndat = lrint((k+1)*L*rate - lower) evaluated in
    seconds like the reference.  Python's round() is the same round-half-even as lrint."""
    lower = int(round(float(k) * division_seconds * rate))
    ndat = int(round((float(k + 1) * division_seconds - lower / rate) * rate))
    return lower, lower + ndat


def subint_pieces(first_sample, ndat, division_seconds, rate):
    """Subint<Fold> / TimeDivide in seconds mode (TimeDivide.C:440-459,503-540, Subint.h:234-309), expressed
    in output samples (the observation start is the start of division 0).  Splits the block
    [first_sample, first_sample+ndat) into (idat_start, ndat_fold, division, division_complete) pieces."""
    out = []
    pos = first_sample
    end = first_sample + ndat
    k = max(int(pos / (division_seconds * rate)) - 1, 0)
    while subint_bounds(k, division_seconds, rate)[1] <= pos:
        k += 1
    while pos < end:
        upper = subint_bounds(k, division_seconds, rate)[1]
        stop = min(end, upper)
        out.append((pos - first_sample, stop - pos, k, stop == upper))
        pos = stop
        if pos == upper:
            k += 1
    return out


class TurnsDivider:
    """dsp::TimeDivide in turns mode (dspsr -s / -turns N; TimeDivide.C:360-436,461-500): division k spans pulse phases
    [start_phase + k*D, start_phase + (k+1)*D), start_phase = the first phase at or after the observation start whose
    fractional part is reference_phase (the leading partial turn is not folded) unless fractional_pulses.  Boundaries
    are snapped to output samples like set_boundaries(mjd1, mjd2) (:503-540).  D < 1 (phase-resolved divisions): the first
    boundary reference_phase + N*D after the start (:374-425).  phase(t) -> (int, frac), iphase((int, frac), t_guess) -> t, t in seconds of the stream."""

    def __init__(self, phase, iphase, period_guess, t_start, rate, division_turns, reference_phase=0.0,
                 fractional_pulses=False):
        if division_turns <= 0.0:
            raise DspsrAmdError("dsp::TimeDivide division_turns must be positive")
        self.iphase, self.t_start, self.rate, self.D, self.pguess = iphase, t_start, rate, float(division_turns), period_guess
        pi, pf = phase(t_start)
        if division_turns < 1.0:
            # phase-resolved divisions (:374-425): X = R + N*D, the first division boundary after the current phase
            x_minus_r = pf - reference_phase
            if pf < reference_phase:
                x_minus_r += 1.0
                pi -= 1
            x = reference_phase + int(math.ceil(x_minus_r / division_turns)) * division_turns
            xi = math.floor(x)
            self.start_phase = (pi + int(xi), x - xi)
        else:
            if not fractional_pulses and pf > reference_phase:
                pi += 1
            self.start_phase = (pi, reference_phase)
        self.start_time = iphase(self.start_phase, t_start)
        self._cache = {}

    def _at(self, turns):
        tot = self.start_phase[1] + turns
        ti = math.floor(tot)
        return self.iphase((self.start_phase[0] + int(ti), tot - ti), self.start_time + turns * self.pguess)

    def bounds(self, k):
        """[first, last) output sample of division k (sample 0 = first output sample of the stream)."""
        if k not in self._cache:
            mjd1, mjd2 = self._at(k * self.D), self._at((k + 1) * self.D)
            lower = int(round((mjd1 - self.t_start) * self.rate))                      # lrint
            ndat = int(round((mjd2 - (self.t_start + lower / self.rate)) * self.rate))
            self._cache[k] = (lower, lower + ndat)
            if len(self._cache) > 64:
                self._cache.pop(next(iter(self._cache)))
        return self._cache[k]

    def pieces(self, first_sample, ndat):
        """Subint<Fold> over one block: (idat_start, ndat_fold, division, division_complete) pieces; samples in front of
        division 0 are skipped (TimeDivide::set_bounds, :196-246: idat_start = rint((lower - input_start) * rate))."""
        out = []
        pos, end = first_sample, first_sample + ndat
        pos = max(pos, self.bounds(0)[0])
        if pos >= end:
            return out
        k = max(int((pos - self.bounds(0)[0]) / (self.D * self.pguess * self.rate)) - 1, 0)
        while self.bounds(k)[1] <= pos:
            k += 1
        while pos < end:
            upper = self.bounds(k)[1]
            stop = min(end, upper)
            out.append((pos - first_sample, stop - pos, k, stop == upper))
            pos = stop
            if pos == upper:
                k += 1
        return out


MOMENT_PAIRS = tuple((i, j) for i in range(4) for j in range(i, 4))    # FourthMoment.C:67-72 = Archiver.C:747-767


def moments_to_central(profile, hits, scale):
    """The Archiver's treatment of folded fourth moments (Archiver.C:679-713,738-771).  profile: [nchan][1][nbin][14] sums,
    hits: [nbin].  The four Stokes sums are divided by scale * hits, the ten product sums by scale^2 * hits ("FourthMoments
    start with Stokes squared", :684), both kept as float32 amps as there; then raw_to_central, in double:
    (moment - mean_i * mean_j) / hits, the covariance of the mean.  Returns (means float32 [nchan][4][nbin], central float32
    [nchan][10][nbin]), the ten in the order MOMENT_PAIRS.  Bins without hits: means as normalise_profile (the mean of the
    others), central moments 0 (the reference divides by hits = 0 there)."""
    prof = np.asarray(profile, dtype=np.float64)
    if prof.ndim != 4 or prof.shape[1] != 1 or prof.shape[3] != 14:
        raise DspsrAmdError("moments_to_central: profile of shape %r is not [nchan][1][nbin][14]" % (prof.shape,))
    hits = np.asarray(hits, dtype=np.float64)
    ok = hits > 0
    means = normalise_profile(prof[..., :4], hits, scale)[:, 0].transpose(0, 2, 1)             # float32 [nchan][4][nbin]
    raw = normalise_profile(prof[..., 4:], hits, float(scale) * float(scale))[:, 0].transpose(0, 2, 1)
    central = np.zeros(raw.shape, dtype=np.float32)
    for k, (i, j) in enumerate(MOMENT_PAIRS):
        pi, pj = means[:, i, ok].astype(np.float64), means[:, j, ok].astype(np.float64)
        central[:, k, ok] = ((raw[:, k, ok].astype(np.float64) - pi * pj) / hits[ok]).astype(np.float32)
    return means, central


def normalise_profile(profile, hits, scale):
    """dsp::Archiver::set (Archiver.C:773-893): amps = sum / (scale * hits); bins without hits take the mean
    of the others.  profile: [nchan][npol][nbin][ndim] sums, hits: [nbin]."""
    hits = np.asarray(hits, dtype=np.float64)
    prof = np.asarray(profile, dtype=np.float64)
    ok = hits > 0
    amps = np.zeros_like(prof)
    amps[:, :, ok, :] = prof[:, :, ok, :] / (scale * hits[ok])[None, None, :, None]
    if ok.any() and not ok.all():
        amps[:, :, ~ok, :] = amps[:, :, ok, :].mean(axis=2, keepdims=True)
    return amps.astype(np.float32)


# ---- archive hand-off: a PhaseSeries on disk, one file per sub-integration ------------------------
# DSPSR's Archiver needs PSRCHIVE (not available to this library), so a finished sub-integration is handed over as a
# self-describing file that carries exactly the members dsp::Archiver::set reads from a dsp::PhaseSeries
# (Archiver.C:430-893): the Observation keys in the DADA ASCII convention (ASCIIObservation.C:82-415), then
# hits[nbin] (uint32, little endian) and the profile sums [nchan][npol][nbin][ndim] (float32, little endian,
# un-normalised: Archiver divides by scale*hits, :773-893).  INTEGRATION.md shows the reader a maintainer adds.
def subint_profile(sub):
    """The profile of one entry of LoadToFold.subints as a host float32 array, whichever path delivered it: `profile` (host
    memory: the RCCL exchange of dspsr_amd_reduce_profiles_finish, or merge_subints) or `profile_dev` (a device tensor: one
    rank, or the torch.distributed forms)."""
    prof = sub.get("profile")
    if prof is None:
        prof = sub["profile_dev"].cpu().numpy()
    return np.asarray(prof, dtype=np.float32)


PHASE_SERIES_MAGIC = "DSPSR_AMD_PHASESERIES"
PHASE_SERIES_HDR_SIZE = 4096


def write_phase_series(path, sub, info: "InputInfo", cfg: "Config", *, nchan=None, npol=1, scale=1.0, division=0,
                       start_seconds=0.0, folding_period=0.0, reference_phase=0.0, state=None, ndim=None, rate=None, nsub_swap=None):
    """sub: a dict as LoadToFold.subints holds (hits, integration_length, ndat_total, profile or profile_dev).  A -4 run
    (fourth_moment_active(cfg)) writes STATE FourthMoment, NPOL 1, NDIM 14 whatever npol / state say.  rate / nsub_swap (a -G run:
    spectra per second, and the input channels whose raw transform order the output channels keep) add the keys RATE and
    NSUB_SWAP; without them the header is what it always was.  hits of two dimensions ([nchan][nbin]: a -skz run, whose fold counts
    per channel) add the key HITS_NCHAN and are written whole; one-dimensional hits leave header and body as they always were."""
    prof = sub.get("profile")
    if prof is None:
        prof = sub["profile_dev"].cpu().numpy()
    nchan = nchan or cfg.nchan
    hits = np.asarray(sub["hits"])
    nbin = hits.shape[-1]
    if state is None and ndim is None and info.detected is not None:                       # detected input: the file's own state
        state, ndim = info.detected, 1
    if state is None and ndim is None and square_law_state(cfg, info, strict=False):       # -d 1 / -d 2 / one polarisation: rows of ndim 1
        state, ndim = square_law_state(cfg, info, strict=False)[0], 1
    ndim = ndim or cfg.ndim
    if fourth_moment_active(cfg) and not cfg.cyclic_nchan and not cfg.plfb_nbin:
        npol, ndim, state = 1, 14, "FourthMoment"
    prof = np.ascontiguousarray(np.asarray(prof, dtype="<f4").reshape(nchan, npol, nbin, ndim))
    keys = [("HDR_MAGIC", PHASE_SERIES_MAGIC), ("HDR_VERSION", "1.0"), ("HDR_SIZE", PHASE_SERIES_HDR_SIZE),
            ("FREQ", repr(float(info.centre_frequency))), ("BW", repr(float(info.bandwidth))), ("NCHAN", nchan),
            ("NPOL", npol), ("NDIM", ndim), ("NBIN", nbin),
            ("STATE", state or ("Stokes" if cfg.stokes else "Coherence")),
            ("DM", repr(float(cfg.dispersion_measure))), ("SCALE", repr(float(scale))),
            ("MJD_DAY", info.mjd_day), ("MJD_SEC", repr(float(info.mjd_sec))),
            ("OBS_OFFSET_SECONDS", repr(float(start_seconds))), ("DIVISION", division),
            ("INTEGRATION_LENGTH", repr(float(sub["integration_length"]))), ("NDAT_TOTAL", int(sub["ndat_total"])),
            ("FOLDING_PERIOD", repr(float(folding_period))), ("REFERENCE_PHASE", repr(float(reference_phase)))]
    if rate is not None:
        keys.append(("RATE", repr(float(rate))))
    if nsub_swap is not None:
        keys.append(("NSUB_SWAP", int(nsub_swap)))
    if hits.ndim == 2:
        keys.append(("HITS_NCHAN", hits.shape[0]))
    text = "".join("%-20s %s\n" % (k, v) for k, v in keys)
    if len(text) >= PHASE_SERIES_HDR_SIZE:
        raise DspsrAmdError("write_phase_series: header does not fit %d bytes" % PHASE_SERIES_HDR_SIZE)
    with open(path, "wb") as f:
        f.write(text.encode("ascii").ljust(PHASE_SERIES_HDR_SIZE, b"\0"))
        f.write(np.ascontiguousarray(hits, dtype="<u4").tobytes())
        f.write(prof.tobytes())


def read_phase_series(path):
    """Returns (header dict, hits uint32[nbin] -- [HITS_NCHAN][nbin] where the header has that key --, profile float32
    [nchan][npol][nbin][ndim])."""
    with open(path, "rb") as f:
        raw = f.read(PHASE_SERIES_HDR_SIZE)
        hdr = {}
        for line in raw.split(b"\0", 1)[0].decode("ascii").splitlines():
            parts = line.split(None, 1)
            if len(parts) == 2:
                hdr[parts[0]] = parts[1].strip()
        if hdr.get("HDR_MAGIC") != PHASE_SERIES_MAGIC:
            raise DspsrAmdError("read_phase_series: %s is not a %s file" % (path, PHASE_SERIES_MAGIC))
        nchan, npol, nbin, ndim = (int(hdr[k]) for k in ("NCHAN", "NPOL", "NBIN", "NDIM"))
        hits_nchan = int(hdr.get("HITS_NCHAN", 0))
        hits = np.frombuffer(f.read(4 * nbin * max(1, hits_nchan)), dtype="<u4").copy()
        body = f.read(4 * nchan * npol * nbin * ndim)
        if len(hits) != nbin * max(1, hits_nchan) or len(body) != 4 * nchan * npol * nbin * ndim:
            raise DspsrAmdError("read_phase_series: %s is truncated" % path)
        if hits_nchan:
            hits = hits.reshape(hits_nchan, nbin)
        prof = np.frombuffer(body, dtype="<f4").reshape(nchan, npol, nbin, ndim).copy()
    return hdr, hits, prof


class PhaseSeries:
    """The product's dsp::PhaseSeries (Signal/Pulsar/dsp/PhaseSeries.h:163-200): profile sums resident on the device
    ([nchan][npol][nbin*ndim] float32 tensor), hits[] and the integration bookkeeping on the host, plus the Observation
    attributes `combinable` compares.  mixable / combine follow PhaseSeries.C:336-418,442-484; the profile half of
    combine is TimeSeries::operator += on the device (dspsr_amd_add_fpt)."""

    OBS_KEYS = ("centre_frequency", "bandwidth", "nchan", "npol", "ndim", "state", "rate")

    def __init__(self, ctx, obs=None):
        self.ctx = ctx
        self.obs = dict(obs or {})
        self.nbin = 0
        self.profile = None
        self.hits = np.zeros(0, np.uint32)
        self.integration_length = 0.0
        self.ndat_total = 0
        self.start_time = self.end_time = 0.0

    @classmethod
    def from_subint(cls, ctx, sub, obs, start_time=0.0, end_time=0.0):
        """Wrap a dict of LoadToFold.subints (hits, integration_length, ndat_total and the device copy `profile_dev`, or the
        host array `profile` an RCCL exchange delivered -- uploaded here)."""
        ps = cls(ctx, obs)
        ps.nbin = len(sub["hits"])
        dev = sub.get("profile_dev")
        if dev is None:
            import torch
            dev = torch.from_numpy(np.ascontiguousarray(subint_profile(sub)).reshape(-1)).to(_device(ctx))
        ps.profile = dev.view(obs["nchan"], obs["npol"], ps.nbin * obs["ndim"])
        ps.hits = np.array(sub["hits"], dtype=np.uint32)
        ps.integration_length, ps.ndat_total = float(sub["integration_length"]), int(sub["ndat_total"])
        ps.start_time, ps.end_time = start_time, end_time
        return ps

    def zero(self):                                            # PhaseSeries::zero, PhaseSeries.C:239-256
        self.integration_length, self.ndat_total = 0.0, 0
        self.hits[:] = 0
        if self.profile is not None:
            self.profile.zero_()

    def combinable(self, obs):                                 # Observation::combinable: the attributes that must agree
        return all(self.obs.get(k) == obs.get(k) for k in self.OBS_KEYS)

    def mixable(self, obs, nbin, start_time, end_time):
        """PhaseSeries::mixable (PhaseSeries.C:336-418): an empty integration adopts `obs`, is resized and zeroed (the
        count of dropped samples ndat_total survives); otherwise the observations must be combinable and nbin equal, and
        the time span is extended."""
        if self.integration_length == 0.0:
            self.obs = {k: obs.get(k) for k in self.OBS_KEYS}
            keep = self.ndat_total
            self.nbin = nbin
            shape = (obs["nchan"], obs["npol"], nbin * obs["ndim"])
            if self.profile is None or tuple(self.profile.shape) != shape:
                self.profile = _device_empty(self.ctx, shape)
            self.hits = np.zeros(nbin, np.uint32)
            self.zero()
            self.ndat_total = keep
            self.start_time, self.end_time = start_time, end_time
            return True
        if not self.combinable(obs) or self.nbin != nbin:
            return False
        self.end_time = max(self.end_time, end_time)
        self.start_time = min(self.start_time, start_time)
        return True

    def combine(self, other):
        """PhaseSeries::combine (PhaseSeries.C:442-484)."""
        if other is None or other.nbin == 0:
            return self
        if not self.integration_length:                        # this is empty: *this = *prof
            keep = self.ndat_total
            self.mixable(other.obs, other.nbin, other.start_time, other.end_time)
            self.profile.copy_(other.profile)
            self.hits = other.hits.copy()
            self.integration_length, self.ndat_total = other.integration_length, other.ndat_total + 0 * keep
            return self
        if not self.mixable(other.obs, other.nbin, other.start_time, other.end_time):
            raise DspsrAmdError("PhaseSeries::combine PhaseSeries !mixable")
        add_fpt(self.ctx, self.profile, other.profile)         # TimeSeries::operator +=
        self.hits += other.hits
        self.integration_length += other.integration_length
        self.ndat_total += other.ndat_total
        return self


def combine_phase_series(a, b):
    """dsp::PhaseSeries::combine (PhaseSeries.C:442-484) on sub-integration dicts (host arrays): how UnloaderShare
    merges the pieces of one division folded by time-sliced replicas.  An empty `a` (integration_length 0) becomes a
    copy of `b`; otherwise profiles, hits, integration_length and ndat_total add."""
    if b is None or len(b["hits"]) == 0:
        return a
    pb = b.get("profile")
    if pb is None:
        pb = b["profile_dev"].cpu().numpy()
    if a is None or not a["integration_length"]:
        return {"hits": np.array(b["hits"], dtype=np.uint32), "integration_length": float(b["integration_length"]),
                "ndat_total": int(b["ndat_total"]), "profile": np.array(pb, dtype=np.float32)}
    pa = a.get("profile")
    if pa is None:
        pa = a["profile_dev"].cpu().numpy()
    if np.shape(pa) != np.shape(pb) or len(a["hits"]) != len(b["hits"]):
        raise DspsrAmdError("PhaseSeries::combine PhaseSeries !mixable")
    return {"hits": (np.asarray(a["hits"], dtype=np.uint32) + np.asarray(b["hits"], dtype=np.uint32)),
            "integration_length": float(a["integration_length"]) + float(b["integration_length"]),
            "ndat_total": int(a["ndat_total"]) + int(b["ndat_total"]),
            "profile": (np.asarray(pa, dtype=np.float32) + np.asarray(pb, dtype=np.float32))}


def reduce_subbands(prof, dist=None, rank=0, world=1, gather_buffer=None):
    """torch.distributed form of the sub-band exchange (the product's own is dspsr_amd_reduce_profiles_*, csrc/comm.hip,
    DSPSR_AMD_REDUCE_GATHER; this one serves the gloo CPU tests and one-device rehearsals, where RCCL cannot run).
    Each rank holds the folded profile of its own frequency sub-band (flat [nchan*npol*nbin*ndim] float32); a gather
    delivers the slices to rank 0 in rank order = the concatenated band, which is what PhaseSeries::combine of
    disjoint channel ranges amounts to (PhaseSeries.C:442-484).  hits / integration_length are identical on all ranks
    (channel-independent bin plan, Fold.C:744-787) and are taken from rank 0.
    Returns the full-band tensor on rank 0, None elsewhere; with world == 1 returns `prof` itself."""
    if world <= 1:
        return prof
    if gather_buffer is None or gather_buffer.numel() != world * prof.numel():
        raise DspsrAmdError("reduce_subbands: gather buffer must hold world*profile = %d floats"
                            % (world * prof.numel()))
    mine = prof.reshape(-1).contiguous()
    if rank == 0:
        dist.gather(mine, list(gather_buffer.view(world, -1).unbind(0)), dst=0)
        return gather_buffer
    dist.gather(mine, None, dst=0)
    return None


def check_identical_hits(hits, dist, rank, world):
    """Sub-band sharding: every rank folds with the same channel-independent bin plan (Fold.C:744-787), so hits[] must
    be identical on all ranks ('assert equality in debug').  One small all-reduce pair (MAX and MIN);
    raises on every rank when they differ.  Debug/test aid: not part of the timed path."""
    if world <= 1:
        return
    import torch
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    h = torch.as_tensor(np.asarray(hits, dtype=np.int64), device=dev)
    hi, lo = h.clone(), h.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    if not bool(torch.equal(hi, lo)):
        raise DspsrAmdError("sub-band ranks disagree on hits[]: the shards are not sample aligned "
                            "(different nfilt_pos/neg, start time or rate)")


def reduce_replicas(prof, hits, integration_length, ndat_total, dist=None, rank=0, world=1):
    """Time-slice replicas (single-channel input has no exchange-free frequency split; the reference runs one thread
    per time block, MultiThread.C:65-82,120-148, and merges the pieces of a division with PhaseSeries::combine,
    PhaseSeries.C:442-484): a true SUM of profiles, hits, integration_length and ndat_total onto rank 0.
    prof is reduced in place (one reduce of the profile buffer -- RCCL over xGMI on GPUs, gloo in the CPU tests --
    plus two tiny ones for the counters).  Returns (prof, hits, integration_length, ndat_total) on rank 0, None elsewhere."""
    if world <= 1:
        return prof, np.asarray(hits, dtype=np.uint32), float(integration_length), int(ndat_total)
    import torch
    dev = prof.device
    dist.reduce(prof, dst=0, op=dist.ReduceOp.SUM)
    cnt = torch.as_tensor(np.concatenate([np.asarray(hits, dtype=np.int64), [int(ndat_total)]]), device=dev)
    dist.reduce(cnt, dst=0, op=dist.ReduceOp.SUM)
    length = torch.tensor([float(integration_length)], dtype=torch.float64, device=dev)
    dist.reduce(length, dst=0, op=dist.ReduceOp.SUM)
    if rank != 0:
        return None
    cnt = cnt.cpu().numpy()
    return prof, cnt[:-1].astype(np.uint32), float(length.item()), int(cnt[-1])


class FilterbankThenConvolution:
    """`dspsr -F N` (Filterbank::Config::After, the default of FilterbankConfig.C:56): dsp::Filterbank with freq_res = 1 -- one
    nsub-point forward transform per output sample, no response (LoadToFold1.C:318-323 sets it only for Config::During) -- then
    dsp::Convolution with the dedispersion response on the filterbank's channels (LoadToFold1.C:337-380, Convolution.C:338-461),
    here the filterbank object with nchan_subband = 1 per channel.  `response` None: the filterbank alone (Config::Never /
    no coherent dedispersion).

    Presents the interface LoadToFold uses of a FilterbankEngine (perform_raw / perform_detect / perform_fold on the 8-bit block,
    nkeep / nsamp_step / nsamp_overlap in INPUT samples), so one part here = one part of the convolution = nsamp_step filterbank
    output samples.  The reference carries the convolution's overlap from block to block (InputBuffering); the blocks this
    pipeline is handed overlap in the raw samples instead (block_bytes), and the filterbank recomputes those few samples."""

    def __init__(self, ctx, nsub, input_nchan, npol, real_input, response, max_parts=1, parts_per_block=1,
                 fused_fold=_lib.FUSED_AUTO):
        self.ctx = ctx
        self.front = FilterbankEngine(ctx).setup(nsub, 1, 0, 0, input_nchan, npol, real_input, None)
        self.nchan, self.npol = nsub * input_nchan, npol
        self.nsamp_fft_front = self.front.nsamp_fft                      # input samples per filterbank output sample
        self.conv = None
        if response is not None:
            # (the convolution's fused fold -- segment sums inside the second inverse pass -- pays a combine launch per input channel:
            #  with 128 channels the detected block + one Fold launch is faster, 12.4 against 18.2 ms per block of `dspsr -F 128`)
            if self.nchan > 8 and fused_fold == _lib.FUSED_AUTO:
                fused_fold = _lib.FUSED_NEVER
            self.conv = ConvolutionEngine(ctx).setup(1, response.ndat, response.impulse_pos, response.impulse_neg, self.nchan, npol,
                                                     False, response.kernel, max_parts=max_parts, fused_fold=fused_fold)
            self.nkeep, self.part_out, self.ovl_out = self.conv.nkeep, self.conv.nsamp_step, self.conv.nsamp_overlap
        else:
            self.nkeep, self.part_out, self.ovl_out = 1, 1, 0
        self.nsamp_step = self.part_out * self.nsamp_fft_front
        self.nsamp_overlap = self.ovl_out * self.nsamp_fft_front
        self.nsamp_fft = self.nsamp_step + self.nsamp_overlap
        self.channelised = None                                           # the filterbank's output block [chan][pol][2 * ndat]
        self._cap = parts_per_block

    def _front(self, raw, layout, scale, npart):
        ndat = npart * self.part_out + self.ovl_out
        if self.channelised is None or self.channelised.shape[2] < 2 * ndat:
            n = max(ndat, self._cap * self.part_out + self.ovl_out)
            n += (-n) % 64                                  # rows start on 512-byte boundaries: the filterbank's runs of 32 samples are whole lines
            self.channelised = _device_empty(self.ctx, (self.nchan, self.npol, 2 * n))
        self.front.perform_raw(raw, layout, scale, self.channelised, ndat)
        return self.channelised

    def set_guppi(self, *geometry):
        self.front.set_guppi(*geometry)                     # (the engine that reads the 8-bit block)

    def perform_raw(self, raw, layout, scale, out, npart, out_step=None):
        if self.conv is None:
            return self.front.perform_raw(raw, layout, scale, out, npart, out_step)
        x = self._front(raw, layout, scale, npart)
        self.conv.perform(x, out, npart, 2 * self.part_out, out_step or 2 * self.nkeep)

    def perform_detect(self, det, npart, state=_lib.COHERENCE, ndim=4, raw=None, layout=_lib.RAW_GENERIC, scale=1.0):
        if self.conv is None:
            return self.front.perform_detect(det, npart, state, ndim, raw=raw, layout=layout, scale=scale)
        x = self._front(raw, layout, scale, npart)
        self.conv.perform_detect(det, npart, state, ndim, inp=x, in_step=2 * self.part_out)

    def perform_fold(self, fold, npart, state=_lib.COHERENCE, raw=None, layout=_lib.RAW_GENERIC, scale=1.0):
        if self.conv is None:
            return self.front.perform_fold(fold, npart, state, raw=raw, layout=layout, scale=scale)
        x = self._front(raw, layout, scale, npart)
        self.conv.perform_fold(fold, npart, state, inp=x, in_step=2 * self.part_out)

    def fold_is_fused(self):
        return (self.conv or self.front).fold_is_fused()

    def npass(self, raw_input=True):
        return 1 + (self.conv.npass(False) if self.conv is not None else 0)

    def finish(self):
        self.ctx.synchronize()

    def close(self):
        self.front.close()
        if self.conv is not None:
            self.conv.close()
        self.channelised = None


class ConvolutionThenFilterbank:
    """`dspsr -F N:B` (Filterbank::Config::Before, FilterbankConfig.C:76-78; LoadToFold1.C:326-385): dsp::Convolution with the dedispersion
    response of the WHOLE input channel first (the filterbank object with nchan_subband = 1 on the 8-bit block: Convolution.C:338-461),
    then the non-convolving filterbank (freq_res = 1, Filterbank.C:614-623) on the dedispersed complex rows.  Every channel then
    refers to the input channel's centre frequency: no dispersion delay is left between the output channels.
    The convolution keeps `ck` complex samples per part and the filterbank consumes `nsub` per output sample; the reference carries
    the remainder from block to block (InputBuffering).  Here one part of the interface LoadToFold uses is P = nsub / gcd(ck, nsub)
    parts of the convolution, which hold a whole number of filterbank transforms -- no remainder, same samples."""

    def __init__(self, ctx, nsub, input_nchan, npol, real_input, response, max_parts=1, parts_per_block=1):
        self.ctx = ctx
        self.conv = ConvolutionEngine(ctx).setup(1, response.ndat, response.impulse_pos, response.impulse_neg, input_nchan, npol, real_input,
                                                 response.kernel, max_parts=max_parts)
        self.back = FilterbankEngine(ctx).setup(nsub, 1, 0, 0, input_nchan, npol, False, None)
        ck = self.conv.nkeep
        self.P = nsub // math.gcd(ck, nsub)
        self.nsub, self.in_nchan, self.npol = nsub, input_nchan, npol
        self.nkeep = self.P * ck // nsub                         # filterbank output samples per (super) part
        self.nsamp_step = self.P * self.conv.nsamp_step
        self.nsamp_overlap = self.conv.nsamp_overlap
        self.nsamp_fft = self.nsamp_step + self.nsamp_overlap
        self.dedispersed = None                                   # the convolution's output block [input chan][pol][2 * ndat]
        self._cap = parts_per_block

    def _front(self, raw, layout, scale, npart):
        ncv = npart * self.P
        ndat = ncv * self.conv.nkeep
        if self.dedispersed is None or self.dedispersed.shape[2] < 2 * ndat:
            n = max(ndat, self._cap * self.P * self.conv.nkeep)
            self.dedispersed = _device_empty(self.ctx, (self.in_nchan, self.npol, 2 * n))
        self.conv.perform_raw(raw, layout, scale, self.dedispersed, ncv)
        return self.dedispersed, ndat // self.nsub

    def set_guppi(self, *geometry):
        self.conv.set_guppi(*geometry)                      # (the engine that reads the 8-bit block)

    def perform_raw(self, raw, layout, scale, out, npart, out_step=None):
        x, nfb = self._front(raw, layout, scale, npart)
        self.back.perform(x, out, nfb, 2 * self.nsub, out_step or 2)

    def perform_detect(self, det, npart, state=_lib.COHERENCE, ndim=4, raw=None, layout=_lib.RAW_GENERIC, scale=1.0):
        x, nfb = self._front(raw, layout, scale, npart)
        self.back.perform_detect(det, nfb, state, ndim, inp=x, in_step=2 * self.nsub)

    def perform_fold(self, fold, npart, state=_lib.COHERENCE, raw=None, layout=_lib.RAW_GENERIC, scale=1.0):
        x, nfb = self._front(raw, layout, scale, npart)
        self.back.perform_fold(fold, nfb, state, inp=x, in_step=2 * self.nsub)

    def fold_is_fused(self):
        return 0

    def npass(self, raw_input=True):
        return self.conv.npass(raw_input) + 1

    def finish(self):
        self.ctx.synchronize()

    def close(self):
        self.conv.close()
        self.back.close()
        self.dedispersed = None


def cyclic_geometry(cfg: "Config", info: "InputInfo"):
    """Sizes and state of a cyclic-spectrum run (dsp/CyclicFold.h:66, CyclicFold.C:96-119): nlag, nchan_spec = 2 nlag - 2,
    nchan_spec / mover output channels per filterbank channel, ndim 1, npol 1 (Intensity; PP for one input polarisation),
    2 (PPQQ) or 4 (Coherence).  Raises DspsrAmdError for what the reference refuses or this path does not build."""
    n, m = int(cfg.cyclic_nchan), int(cfg.cyclic_mover)
    if n <= 0:
        raise DspsrAmdError("dspsr_amd.cyclic_geometry: cyclic_nchan=%d" % n)
    if m < 1 or (m * n) % 2:
        raise DspsrAmdError("dsp::CyclicFold nlag = mover*nchan/2 + 1 needs an even mover*nchan (nchan=%d, mover=%d)" % (n, m))
    nlag = m * n // 2 + 1
    nchan_spec = 2 * nlag - 2
    if nchan_spec & (nchan_spec - 1):
        raise DspsrAmdError("dspsr_amd.LoadToFold: cyclic spectra of %d x %d points: the backward transform of the lags is built "
                            "for powers of two" % (n, m))
    npol = int(cfg.cyclic_npol) or (4 if info.npol == 2 else 1)
    if npol not in (1, 2, 4):
        raise DspsrAmdError("dsp::CyclicFold::prepare_output invalid npol=%d" % npol)             # CyclicFold.C:117-119
    if info.npol == 1 and npol != 1:
        raise DspsrAmdError("dsp::CyclicFold: one input polarisation gives npol=1 only (asked for %d)" % npol)
    if info.npol not in (1, 2):
        raise DspsrAmdError("dsp::CyclicFoldEngine::fold Invalid npol=%d" % info.npol)             # CyclicFold.C:443-445
    state = {1: "PP" if info.npol == 1 else "Intensity", 2: "PPQQ", 4: "Coherence"}[npol]
    return {"nlag": nlag, "mover": m, "nchan_spec": nchan_spec, "nchan_per_channel": nchan_spec // m,
            "nchan": cfg.nchan * (nchan_spec // m), "npol": npol, "ndim": 1, "state": state}


def cyclic_check(cfg: "Config", info: "InputInfo", ntargets=0, subband=None, dump_before=()):
    """What a cyclic run refuses, before any device resource is opened; returns cyclic_geometry."""
    if cfg.subint_turns == 1.0:
        raise DspsrAmdError("dsp::LoadToFold::build Single-pulse and cyclic spectrum modes are incompatible")  # LoadToFold1.C:1037-1039
    if ntargets > 1:
        raise DspsrAmdError("dspsr_amd.LoadToFold: cyclic spectra fold one pulsar; %d targets given" % ntargets)
    if cfg.interchan_dedispersion:
        raise DspsrAmdError("dspsr_amd.LoadToFold: -K is not built for cyclic spectra")
    if cfg.convolve_when != "during":
        raise DspsrAmdError("dspsr_amd.LoadToFold: cyclic spectra are built for -F N:D (convolve_when = during), not %r"
                            % (cfg.convolve_when,))
    if subband is not None:
        raise DspsrAmdError("dspsr_amd.LoadToFold: cyclic spectra are not built for sub-band sharded runs / communicators")
    if tuple(dump_before):
        raise DspsrAmdError("dspsr_amd.LoadToFold: the dump taps are not built for cyclic spectra")
    return cyclic_geometry(cfg, info)


def plfb_choose_nchan(period, rate, nbin):
    """PhaseLockedFilterbank::prepare (PhaseLockedFilterbank.C:65-73): the largest power of two <= the samples per phase bin."""
    samples_per_bin = period * rate / nbin
    return int(math.pow(2.0, math.floor(math.log(samples_per_bin) / math.log(2.0))))


class PlfbPlan:
    """The windows of dsp::PhaseLockedFilterbank for ONE transformation call over the whole stream (PhaseLockedFilterbank.C:
    208-235): `divider` is a TurnsDivider with D = 1 / nbin (:36-40).  Every division yields a window at its first sample --
    max(its lower boundary, the end of the division before), as TimeDivide::set_bounds chains them (TimeDivide.C:146-211) --
    with the phase bin of TimeDivide.C:486-492: profile_phase = division start phase - reference_phase + D / 2,
    bin = unsigned(frac / D).  A window is kept iff ndat_fft samples from there exist (:224-228).
    The plan is a function of the stream, not of how it is cut into blocks: take(avail) hands out, once each and in time order,
    the windows whose last sample lies in front of stream sample `avail`; what does not fit yet waits for the next call."""

    def __init__(self, divider, nbin, reference_phase, ndat_fft):
        self.div, self.nbin, self.ref, self.ndat_fft = divider, int(nbin), float(reference_phase), int(ndat_fft)
        self.k, self.pos, self._cur = 0, 0, None

    def phase_bin(self, k):
        d = self.div.D
        x = self.div.start_phase[1] + k * d - self.ref + 0.5 * d
        return int((x - math.floor(x)) / d)

    def _window(self):
        """(first sample, bin, end) of the next division that has samples"""
        if self._cur is None:
            while self.div.bounds(self.k)[1] <= self.pos:
                self.k += 1
            lo, hi = self.div.bounds(self.k)
            self._cur = (max(lo, self.pos), self.phase_bin(self.k), hi)
        return self._cur

    def next_start(self):
        """first sample of the first window not handed out yet"""
        return self._window()[0]

    def take(self, avail):
        """(idat_start uint64[], bin uint32[]) in stream samples"""
        starts, bins = [], []
        while True:
            s, b, hi = self._window()
            if s + self.ndat_fft > avail:
                break
            starts.append(s)
            bins.append(b)
            self.pos, self.k, self._cur = hi, self.k + 1, None
        return np.array(starts, dtype=np.uint64), np.array(bins, dtype=np.uint32)


def plfb_check(cfg: "Config", info: "InputInfo", ntargets=0, subband=None, dump_before=()):
    """What a -G run refuses, before any device resource is opened."""
    who = "dspsr_amd.LoadToFold: the phase-locked filterbank (-G)"
    if cfg.subint_seconds > 0 or cfg.subint_turns > 0:
        # Subint<PhaseLockedFilterbank> limits only the END of each piece (dsp/Subint.h:312-318) while transformation re-walks the
        # block from its first sample (PhaseLockedFilterbank.C:166-185): every piece after the first counts its windows twice
        raise DspsrAmdError("%s is not built for sub-integrations (-L, -s, -turns): the reference's Subint<PhaseLockedFilterbank> "
                            "re-walks each block from its start and counts windows twice" % who)
    if cfg.interchan_dedispersion:
        raise DspsrAmdError("%s is not built for -K" % who)
    if ntargets > 1:
        raise DspsrAmdError("%s folds one pulsar; %d targets given" % (who, ntargets))
    if cfg.cyclic_nchan > 0:
        raise DspsrAmdError("%s and cyclic spectra (-cyclic) exclude each other" % who)
    if cfg.fourth_moment:
        raise DspsrAmdError("%s and fourth moments (-4) exclude each other: it replaces Detection" % who)
    if cfg.convolve_when != "during":
        raise DspsrAmdError("%s is built for -F N:D (convolve_when = during), not %r" % (who, cfg.convolve_when))
    if subband is not None:
        raise DspsrAmdError("%s is not built for sub-band sharded runs / communicators" % who)
    if tuple(dump_before):
        raise DspsrAmdError("%s: the dump taps are not built for it" % who)
    if cfg.npol not in (1, 2, 4):
        raise DspsrAmdError("dsp::PhaseLockedFilterbank::set_npol Invalid npol (%d)" % cfg.npol)      # PhaseLockedFilterbank.C:44-46
    if info.npol < 2 and cfg.npol > 1:                                                                 # :138-141
        raise DspsrAmdError("dsp::PhaseLockedFilterbank::transformation Not enough input polns (%d) for output npol (%d)"
                            % (info.npol, cfg.npol))
    if cfg.plfb_nchan < 0 or cfg.plfb_nbin < 1 or (cfg.plfb_nchan == 1 and cfg.plfb_nbin < 2):
        raise DspsrAmdError("dsp::PhaseLockedFilterbank::prepare invalid dimensions.  nchan=%d nbin=%d" % (cfg.plfb_nchan, cfg.plfb_nbin))


def rfi_check(cfg: "Config", info: "InputInfo", subband=None):
    """What a -R run refuses, before any device resource is opened."""
    who, instead = "dspsr_amd.LoadToFold: the RFI filter (-R)", "the Bandpass operator's integrate_raw reads the generic and CASPSR byte orders"
    refuse_forms(who, info, FORMS - {"guppi"}, instead)          # (GUPPI raw blocks are refused first and heaps last, as they always were)
    if cfg.calibrator is not None:
        raise DspsrAmdError("%s with -pac (calibrator) is not built: the product of the mask, the chirp and a matrix response is open" % who)
    if info.nchan > 1:
        # the reference takes the mask from input channel 0 and stretches it over all channels (get_datptr(0, .), RFIFilter.C:109-110)
        raise DspsrAmdError("%s is built for one input channel (info.nchan=%d): the reference stretches channel 0's mask over "
                            "all of them, which is not reproduced" % (who, info.nchan))
    if info.npol != 2:
        raise DspsrAmdError("%s reads the passbands of two polarisations (info.npol=%d): dsp::RFIFilter::calculate takes "
                            "get_datptr(0, 0) and get_datptr(0, 1)" % (who, info.npol))
    if cfg.convolve_when == "never" or cfg.dispersion_measure == 0:
        raise DspsrAmdError("%s needs a dedispersion kernel to multiply into (convolve_when=%r, dispersion_measure=%g)"
                            % (who, cfg.convolve_when, cfg.dispersion_measure))
    if subband is not None:
        raise DspsrAmdError("%s is not built for sub-band sharded runs (subband=%d)" % (who, subband))
    if info.nbit != 8:
        raise DspsrAmdError("%s reads 8-bit input (info.nbit=%d): 16-bit input is not built" % (who, info.nbit))
    refuse_forms(who, info, FORMS - {"heaps"}, instead)


def calibrator_response(cfg: "Config", info: "InputInfo", subband=None):
    """`dspsr -pac`: the matrix response of a run with cfg.calibrator -- (Dedispersion response, float32 [N][8]) -- or None without
    one.  Host work only: LoadToFold calls it before it opens any device resource, and every limit raises DspsrAmdError by name.

    The product PolnCalibration x Dedispersion (LoadToFold1.C:270-289) is applied inside the convolving filterbank, so:
      * convolve_when must be "during" (-F N:D): the reference builds the ResponseProduct for that filterbank only;
      * one input channel (Filterbank.C:199-201 throws for more; sub-band sharded runs read several) and two polarisations;
      * a geometry the library takes: nchan and freq_res powers of two, nchan >= 2, 2 <= freq_res <= 8192.
    Detection, Fold, -K, -L / -s, several pulsars and -4 consume the filterbank's detected output as before and work with a
    calibrator (the fold is never fused into the inverse pass then: FilterbankEngine.fold_is_fused() == 0).  -cyclic and -G
    read the complex rows of filterbank objects of their own: refused with a calibrator, by name."""
    if cfg.calibrator is None:
        return None
    from . import polcal
    if cfg.cyclic_nchan > 0:
        raise DspsrAmdError("dspsr_amd.LoadToFold: -pac (calibrator) with -cyclic is not built")
    if cfg.plfb_nbin > 0:
        raise DspsrAmdError("dspsr_amd.LoadToFold: -pac (calibrator) with -G (phase-locked filterbank) is not built")
    if cfg.convolve_when != "during":
        raise DspsrAmdError("dspsr_amd.LoadToFold: -pac (calibrator) needs convolve_when='during' (-F N:D), not %r: the matrix "
                            "response is applied inside the convolving filterbank" % (cfg.convolve_when,))
    if info.nchan != 1 or subband is not None:
        raise DspsrAmdError("dsp::Filterbank::make_preparations matrix convolution untested for > one input channel (input nchan=%d)"
                            % info.nchan)
    if info.npol != 2:
        raise DspsrAmdError("dspsr_amd.LoadToFold: -pac (calibrator) needs two polarisations (npol=%d)" % info.npol)
    freq, jones = polcal.load_calibrator(cfg.calibrator) if isinstance(cfg.calibrator, (str, bytes, os.PathLike)) \
        else polcal._check_calibrator(*cfg.calibrator)
    response = matched_response(info, cfg.dispersion_measure, cfg.freq_res, cfg.nchan, input_nchan=1, ndim=info.ndim,
                                fractional_delay=cfg.interchan_dedispersion)
    pow2 = lambda v: v >= 1 and not (v & (v - 1))
    if cfg.nchan < 2 or not pow2(cfg.nchan) or not pow2(response.ndat) or not 2 <= response.ndat <= 8192:
        raise DspsrAmdError("dspsr_amd.LoadToFold: -pac (calibrator) needs nchan=%d >= 2 and freq_res=%d in [2, 8192], both powers of "
                            "two (the three-pass filterbank)" % (cfg.nchan, response.ndat))
    matrix = polcal.response_product(polcal.jones_response(freq, jones, info, cfg.nchan, response.ndat), response.kernel)
    return response, matrix


def square_law_state(cfg: "Config", info: "InputInfo", strict=True):
    """`-d 1`, `-d 2` and one-polarisation input on the plain path (Detection + Fold; -cyclic and -G have their own reading of
    npol): None where Detection forms the four products or -4 folds their moments -- today's path --, else (state name,
    library state, output polarisations) of Detection::square_law.  The branch order of LoadToFold1.C:552-568 and 1098-1134:
    npol 1 or 3 first (Intensity; `Detection::transformation` does not know NthPower, Detection.C:112-133), then -4, then 2
    (PPQQ), then 4.  One input polarisation folds as PP whatever npol asks for (LoadToFold1.C:1112-1116) -- except under the
    default npol = 4, where this path keeps the refusal it has always had ("Cannot detect polarization when npol != 2")."""
    if cfg.cyclic_nchan > 0 or cfg.plfb_nbin > 0 or cfg.npol == 4 or fourth_moment_active(cfg):
        return None
    if info.npol == 1:
        return "PP", _lib.INTENSITY, 1
    if cfg.npol not in (1, 2) and not strict:                       # (a writer asking what a finished run folded)
        return None
    if cfg.npol == 3:
        raise DspsrAmdError("dsp::Detection cannot convert from Analytic to NthPower")
    if cfg.npol not in (1, 2):
        raise DspsrAmdError("dspsr_amd.LoadToFold: npol=%d is not one of 1 (Intensity), 2 (PPQQ), 4 (Coherence / Stokes)" % cfg.npol)
    return ("Intensity", _lib.INTENSITY, 1) if cfg.npol == 1 else ("PPQQ", _lib.PPQQ, 2)


def square_law_check(cfg: "Config", info: "InputInfo"):
    """What a run with npol != 4 refuses by name, before any device resource is opened: the combinations whose detected rows are
    not formed by Detection::square_law on this path yet."""
    who = "dspsr_amd.LoadToFold: npol=%d (-d %d)" % (cfg.npol, cfg.npol)
    for on, what in ((cfg.sk_zap, "spectral kurtosis (-skz): dsp::SpectralKurtosis hands its rows to Detection::polarimetry here"),
                     (raw_form(info).name == "twobit", "two-bit input (NBIT 2): the unpacker's weights are carried to the Coherence fold alone"),
                     (cfg.calibrator is not None, "the calibrator (-pac): the matrix response has no square-law form"),
                     (cfg.convolve_when != "during", "convolve_when=%r (-F N, -F N:B): built for -F N:D (convolve_when = during)" % (cfg.convolve_when,))):
        if on:
            raise DspsrAmdError("%s is not built with %s" % (who, what))


def fourth_moment_active(cfg: "Config") -> bool:
    """The branch order of LoadToFold1.C:552-568: npol 1 or 3 takes the first branch, -4 only the second."""
    return bool(cfg.fourth_moment) and cfg.npol not in (1, 3)


def fourth_moment_check(cfg: "Config", ntargets=0, subband=None):
    """What a -4 run refuses, before any device resource is opened; returns the Config the chain is built with -- detection
    forced to Stokes with ndim 4 (LoadToFold1.C:1119-1123), no fused fold (the fused kernels fold ndim 4 / 2 x 2 only) -- or
    `cfg` itself when -4 is off or loses to npol 1 / 3."""
    if not fourth_moment_active(cfg):
        return cfg
    if cfg.cyclic_nchan > 0:
        raise DspsrAmdError("dspsr_amd.LoadToFold: fourth_moment (-4) and cyclic_nchan (-cyclic) exclude each other: the cyclic "
                            "fold replaces Detection (LoadToFold1.C:534-539)")
    if ntargets > 1:
        raise DspsrAmdError("dspsr_amd.LoadToFold: fourth_moment (-4) folds one pulsar; %d targets given" % ntargets)
    if subband is not None:
        raise DspsrAmdError("dspsr_amd.LoadToFold: fourth_moment (-4) is not built for sub-band sharded runs / the multi-GPU exchange")
    return dataclasses.replace(cfg, stokes=True, ndim=4, fused_fold=False, force_fused=False)


@dataclass
class TwoBitPlan:
    """dsp::TwoBitCorrection of a two-bit run (NBIT 2): the excision window, its limits, the level table and the books."""
    nsample: int
    threshold: float
    cutoff: float
    nlow_min: int
    nlow_max: int
    table_type: int
    levels: object                    # float32 [nlow_max - nlow_min + 1][2]
    first_sample: int = 0             # of the block in hand, inside its first window
    discarded_weights: int = 0        # ExcisionUnpacker::unpack: zero weights after mask_weights, summed over the blocks
    blocks_fused: int = 0             # blocks that folded inside the filterbank's last pass (no zero weight)
    blocks_weighted: int = 0          # blocks that took Detection + Fold with weights


def twobit_check(cfg: "Config", info: "InputInfo", ntargets=0, subband=None, dump_before=()):
    """What a two-bit run refuses, before any device resource is opened, and its plan (LoadToFold1.C:731-743)."""
    from . import twobit
    who = "dspsr_amd.LoadToFold: two-bit input (NBIT 2)"
    for on, what in ((cfg.cyclic_nchan > 0, "-cyclic"), (cfg.plfb_nbin > 0, "-G"), (fourth_moment_active(cfg), "-4"),
                     (cfg.interchan_dedispersion, "-K"), (cfg.zap_rfi, "-R"), (cfg.sk_zap, "-skz"), (cfg.calibrator is not None, "-pac")):
        if on:
            raise DspsrAmdError("%s with %s is not built: carrying the unpacker's weights through it is open" % (who, what))
    if ntargets > 1:
        raise DspsrAmdError("%s folds one pulsar (%d targets given): the weights of several folds are open" % (who, ntargets))
    if cfg.convolve_when != "during":
        raise DspsrAmdError("%s is built for -F N:D (convolve_when = during), not %r: the weights of dsp::Convolution are open"
                            % (who, cfg.convolve_when))
    if subband is not None:
        raise DspsrAmdError("%s is not built for sub-band sharded runs (subband=%d)" % (who, subband))
    if dump_before:
        raise DspsrAmdError("%s with the dump taps is not built" % who)
    if info.machine not in _lib.TWOBIT_MACHINES:
        raise DspsrAmdError("%s is read for INSTRUMENT %s alone, not %s" % (who, ", ".join(sorted(_lib.TWOBIT_MACHINES)), info.machine))
    if info.ndim != 1 or info.nchan != 1 or info.npol not in (1, 2):
        raise DspsrAmdError("%s is one channel of real samples from one or two digitisers (ndim=%d nchan=%d npol=%d)"
                            % (who, info.ndim, info.nchan, info.npol))
    nsample = cfg.excision_nsample or twobit.NSAMPLE
    threshold = cfg.excision_threshold if cfg.excision_threshold > 0 else twobit.THRESHOLD
    cutoff = cfg.excision_cutoff if cfg.excision_cutoff >= 0 else twobit.CUTOFF_SIGMA
    if nsample % 4 or not 4 <= nsample <= twobit.NSAMPLE_MAX:
        raise DspsrAmdError("%s: excision_nsample=%d must be a multiple of 4 in [4, %d]" % (who, nsample, twobit.NSAMPLE_MAX))
    nlow_min, nlow_max = twobit.limits(nsample, threshold, cutoff)
    return TwoBitPlan(nsample, threshold, cutoff, nlow_min, nlow_max, _lib.TWOBIT_MACHINES[info.machine],
                      twobit.levels(nsample, nlow_min, nlow_max, threshold))


def sk_check(cfg: "Config", info: "InputInfo", ntargets=0, subband=None, dump_before=()):
    """What a -skz run refuses, on the host, after every refusal the run had without it.  Returns the channel range the engine gets."""
    who = "dspsr_amd.LoadToFold: spectral kurtosis (-skz)"
    for on, what in ((cfg.cyclic_nchan > 0, "cyclic_nchan (-cyclic)"), (cfg.plfb_nbin > 0, "plfb_nbin (-G)"),
                     (fourth_moment_active(cfg), "fourth_moment (-4)"), (cfg.interchan_dedispersion, "interchan_dedispersion (-K)")):
        if on:
            raise DspsrAmdError("%s is not built with %s" % (who, what))
    if ntargets > 1:
        raise DspsrAmdError("%s folds one pulsar; %d targets given" % (who, ntargets))
    if subband is not None:
        raise DspsrAmdError("%s is not built for sub-band sharded runs / the multi-GPU exchange" % who)
    if cfg.convolve_when != "during":
        raise DspsrAmdError("%s is built for -F N:D (convolve_when = during), not %r" % (who, cfg.convolve_when))
    if dump_before:
        raise DspsrAmdError("%s is not built with the dump taps" % who)
    if info.npol == 1 and cfg.ndim == 4:
        raise DspsrAmdError("%s: one input polarisation cannot be detected with ndim 4" % who)
    if not 32 <= cfg.sk_m <= 65536:
        raise DspsrAmdError("%s: sk_m=%d outside [32, 65536] (below 32 the Pearson IV limits do not exist)" % (who, cfg.sk_m))
    if cfg.sk_std_devs < 1:
        raise DspsrAmdError("%s: sk_std_devs == 0 (SKLimits::calc_limits invalid inputs)" % who)
    if not (cfg.sk_chan_start > 0 and cfg.sk_chan_end < cfg.nchan):                 # LoadToFold1.C:527-528: no range is set
        return 0, 0
    if cfg.sk_chan_start >= (cfg.sk_chan_end or cfg.nchan):
        raise DspsrAmdError("%s: sk_chan_start=%d >= sk_chan_end=%d" % (who, cfg.sk_chan_start, cfg.sk_chan_end or cfg.nchan))
    return cfg.sk_chan_start, cfg.sk_chan_end


def _device(ctx):
    return "cuda:%d" % ctx.device


def _device_empty(ctx, shape, dtype="float32", zero=False):
    """Every device allocation of the drivers: an uninitialised (zero: zeroed) tensor on the context's device."""
    import torch
    return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, dtype), device=_device(ctx))


def matched_response(info, dispersion_measure, freq_res, nchan, *, input_nchan, ndim, dual_sideband=-1, dc_centred=False, swap=False,
                     fractional_delay=False):
    """dsp::Dedispersion over the band of `info`, its frequency resolution set where -x gives one, matched to `nchan` channels."""
    r = Dedispersion(info.centre_frequency, info.bandwidth, dispersion_measure, input_nchan=input_nchan, ndim=ndim,
                     dual_sideband=dual_sideband, dc_centred=dc_centred, swap=swap, fractional_delay=fractional_delay)
    if freq_res:
        r.set_frequency_resolution(freq_res)
    r.match(nchan)
    return r


def filterbank_output(info, r, nsub):
    """The output observation of the convolving filterbank of -F N:D (Filterbank::prepare_output, Filterbank.C:265-379), host
    arithmetic: (rate, start in seconds, scale)."""
    n_fft = nsub * r.ndat
    nsamp_fft = 2 * n_fft if info.ndim == 1 else n_fft
    rate = info.rate * (float(r.ndat) / float(nsamp_fft))
    return rate, info.start_seconds + r.impulse_pos / rate, float(n_fft) * float(r.ndat)


def detected_check(cfg: "Config", info: "InputInfo", subband=None, dump_before=()):
    """What a fold of detected input (info.detected: the first branch of LoadToFold::construct, LoadToFold1.C:126-180) refuses by
    name, before any device resource is opened, each with the option's spelling; returns the Config the chain is built with: the
    file's own polarisations, rows of ndim 1.  The reference ignores -F silently on this branch; here a filterbank is refused
    (SURVEY Appendix C).  cfg.npol = 4 is the option's default and reads as `not given`."""
    who = "dspsr_amd.LoadToFold: detected input (STATE %s)" % info.detected
    if info.ndim != 1 or info.npol not in (1, 2, 4):
        raise DspsrAmdError("%s holds rows of ndim 1 in 1, 2 or 4 polarisations; the input says ndim=%d npol=%d" % (who, info.ndim, info.npol))
    if cfg.nchan != info.nchan:
        raise DspsrAmdError("%s has no voltages to filter: nchan=%d (-F %d) asks for a filterbank, the file holds %d channels "
                            "(give no -F, or -F %d)" % (who, cfg.nchan, cfg.nchan, info.nchan, info.nchan))
    for on, what in ((cfg.cyclic_nchan > 0, "cyclic_nchan (-cyclic): cyclic spectra are formed from voltages"),
                     (cfg.plfb_nbin > 0, "plfb_nbin (-G): the phase-locked filterbank transforms voltages"),
                     (cfg.fourth_moment, "fourth_moment (-4): the moments are formed from the Stokes parameters of voltages"),
                     (cfg.sk_zap, "sk_zap (-skz): dsp::SpectralKurtosis reads voltages"),
                     (cfg.zap_rfi, "zap_rfi (-R): the RFI filter is multiplied into a dedispersion kernel, and there is none"),
                     (cfg.calibrator is not None, "calibrator (-pac): the Jones matrices multiply voltages")):
        if on:
            raise DspsrAmdError("%s is not built with %s" % (who, what))
    if cfg.npol not in (4, info.npol):
        raise DspsrAmdError("%s: npol=%d (-d %d) asks for another state than the file's %d polarisations; detected rows are folded "
                            "as they are (give no -d, or -d %d)" % (who, cfg.npol, cfg.npol, info.npol, info.npol))
    if dump_before:
        raise DspsrAmdError("%s: the dump taps (--dump %s) are not built here: there is no Detection, and pre_Fold would hold the "
                            "file's own values" % (who, ", ".join(dump_before)))
    if subband is not None:
        raise DspsrAmdError("%s is not built for sub-band sharded runs (subband=%d) / the multi-GPU exchange" % (who, subband))
    return dataclasses.replace(cfg, npol=info.npol, ndim=1, stokes=False, fused_fold=False, force_fused=False)


def _adopt_front(drv, fb):
    """`fb` (a FilterbankEngine, or one of the two wrappers above) becomes the front end of the driver: what every path reads of it.
    The form of the blocks (drv.form) is the driver's plan; drv.layout is the layout word of the block in hand."""
    drv.fb = fb
    drv.nkeep, drv.nsamp_step, drv.nsamp_overlap = fb.nkeep, fb.nsamp_step, fb.nsamp_overlap
    drv.scale8 = eight_bit_scale()
    drv.layout, drv.guppi = drv.form.layout, drv.form.geometry
    if drv.form.geometry is not None:                   # a GUPPI raw file: the engine takes the geometry of its blocks once
        fb.set_guppi(*drv.form.geometry)


def _block_layout(drv, first_sample):
    """The layout word of THIS block, for every path below: it names the block's first sample where blocks start inside a heap, a
    GUPPI raw block or an excision window, and refuses one where they do not."""
    drv.layout = drv.form.layout_word(first_sample)


def _open_convolving_front(drv, r, nsub, in_nchan, kernel, **setup):
    """The convolving filterbank of -F N:D with the response `r` on the driver's context, `in_nchan` input channels per block."""
    info = drv.info
    _adopt_front(drv, FilterbankEngine(drv.ctx).setup(nsub, r.ndat, r.impulse_pos, r.impulse_neg, in_nchan, info.npol, info.ndim == 1,
                                                      kernel, **setup))


class DelayCarry:
    """The head room in front of a block's rows, and the tail carried in it (InputBuffering): a block's new samples are written
    behind `head` samples of room, the `carried` ones that the block before did not consume sit right in front of them.
    -K: dsp::SampleDelay gives up its total_delay at the end of every block and InputBuffering re-presents those samples in front
    of the next one (SampleDelay.C:117,146).  `short`: samples a sub-band rank gives up on top of its own delay, so that all ranks
    emit the same ones.  `delays` (relative, per channel): SampleDelay::build on the host (SampleDelay.C:75-99) -- zero, head =
    dsp::SampleDelay's zero_delay and total_delay.  -G and -skz give `head` itself: a window, or a part of M samples, waits there."""

    def __init__(self, delays=None, head=0):
        self.zero = self.carried = self.short = 0
        self.head, self.delays = head, delays
        if delays is not None:
            d = np.asarray(delays, np.int64)
            self.zero = int(d.max())
            self.head = int((self.zero - d).max())

    def check_block(self, who, block):
        if self.head > block:
            raise DspsrAmdError("dspsr_amd.%s: inter-channel delay of %d samples exceeds the block of %d" % (who, self.head, block))

    def new(self, buf, ndim=1):
        """where a block's new samples are written: behind the head room of buf [chan][pol][sample * ndim]"""
        return buf[:, :, self.head * ndim:]

    def rows(self, buf, ndat=None, ndim=1):
        """the samples to transform, `ndat` new ones lying behind the head room of buf [chan][pol][sample * ndim]: the carried tail
        and the new samples less `short` (empty when nothing is left: no transform then).  Without `ndat`: everything from the
        carried tail on (the caller gives its engine the count)"""
        off = self.head - self.carried
        end = None if ndat is None else (off + max(self.carried + ndat - self.short, 0)) * ndim
        return buf[:, :, off * ndim:end]

    def keep_tail(self, ctx, buf, ndat, nout, ndim=1):
        """InputBuffering::set_next_start(output_ndat): the transform delivered `nout` samples; the unshifted tail goes in front of
        the next block (nothing to move when it lies there already)"""
        off, nin = self.head - self.carried, self.carried + ndat
        carry = nin - nout
        if carry and off + nout != self.head - carry:
            move_tail_fpt(ctx, buf, self.head - carry, off + nout, carry, ndim)
        self.carried = carry

    def delayed(self, ctx, sample_delay, buf, ndat, use):
        """The -K step of a block whose `ndat` new samples lie behind the head room of `buf`: SampleDelay in place over the carried
        tail and the new samples, `use(rows)` on the samples it delivers (they are read before the tail moves over them), the
        unshifted tail kept for the next block.  Returns what `use` returns."""
        rows = self.rows(buf, ndat)
        nout = sample_delay.transform(rows) if rows.shape[2] else 0
        result = use(rows[:, :, :nout])
        self.keep_tail(ctx, buf, ndat, nout)
        return result


def _carry_view(name):
    return property(lambda self: getattr(self.sd, name))


def _books(acc, **profile):
    """The entry of `subints` for the integration the accumulator holds"""
    return {"hits": acc.hits.copy(), "integration_length": acc.integration_length, "ndat_total": acc.ndat_total, **profile}


def _emit(acc, entry, zero):
    """Subint<Fold> (Subint.h:291-303): hand over the sub-integration (entry None: it went another way) and start the next one"""
    if entry is not None:
        acc.subints.append(entry)
    zero()
    acc.hits[:] = 0
    acc.integration_length = 0.0
    acc.ndat_total = 0


def _close_all(*objs):
    for o in objs:
        if o is not None:
            o.close()


# ---- the back ends of LoadToFold: what stands behind the front end, one plain class per mode ----------------------------------
# A back end holds the driver `lt` and owns the mode's share of the host plan (plan), of the device (open), of a block (process:
# returns the output samples it consumed), of one piece of the shared walk (plan_piece), of a sub-integration (finish), what
# follows the number of phase bins (shape: at open, and when a single target brings its own), the names of the engines to close (engines) and the words with which the mode
# refuses a multi-GPU exchange (no_exchange).  The engines stay fields of the driver (lt.fold, lt.cyclic, lt.plfb, lt.sk), read
# at every call: that is where callers find, and tests replace, them.

def tap_check(cfg: "Config", dump_before):
    """stage capture (dspsr --dump <Operation>, SingleThread.C:315-346): pre_Detection.dump / pre_Fold.dump"""
    for name in dump_before:
        if name not in ("Detection", "Fold"):
            raise DspsrAmdError("dsp::SingleThread::insert_dump_point no operation named '%s' on this path "
                                "(Detection, Fold)" % name)
        if name == "Detection" and cfg.interchan_dedispersion:
            raise DspsrAmdError("dspsr_amd.LoadToFold: the pre_Detection tap is not built for -K (the delay is applied "
                                "to the detected rows here); tap pre_Fold instead")
    return dump_before


class _BackEnd:
    """What every back end answers; a mode overrides what differs."""

    fronted = True                       # a front end (filterbank / convolution) stands before it; False: the back end plans and opens the whole run

    def __init__(self, lt):
        self.lt = lt

    def state_name(self):
        """Observation::get_state of what the mode folds, where the mode and not Detection decides it (None: Detection's)"""
        return None

    def vitals(self):
        """the lines of LoadToFold.vitals where the run has no filter to report (None: the driver's)"""
        return None


class _RowFold(_BackEnd):
    """The fold of detected float rows, shared by Detection + Fold and by detected input: the plan of a piece, several pulsars over
    the same rows, the end of a sub-integration."""

    def plan_piece(self, acc, phi, phase_per_sample, ndat_fold, idat_start):
        """The host plan loop of Fold::fold (Fold.C:718-787) on the accumulator's fold: the driver's, or a pulsar's"""
        acc.fold.set_nbin(self.lt.cfg.nbin if acc is self.lt else acc.nbin)
        acc.fold.set_ndat(ndat_fold, idat_start)
        if self.lt._weights is not None:             # two-bit input: samples of a zero weight are not folded
            row, npw, widat = self.lt._weights
            return acc.fold.set_bins(phi, phase_per_sample, ndat_fold, idat_start, acc.hits, weights=row, ndatperweight=npw, weight_idat=widat)
        return acc.fold.set_bins(phi, phase_per_sample, ndat_fold, idat_start, acc.hits)

    def _fold_pulsars(self, rows, ndat):
        """Several pulsars over the same detected rows.  The pulsars whose share of the block is one piece of a sub-integration
        fold together (FoldEngine.fold_many: the rows are read once for all of them); a pulsar with a sub-integration boundary
        inside the block folds piece by piece and emits its sub-integration in between."""
        lt = self.lt
        pieces = [lt._pieces(ndat, p) for p in lt.pulsars]
        group = [(p, pc[0]) for p, pc in zip(lt.pulsars, pieces) if len(pc) == 1]
        folded = [lt._plan_piece(piece, p) for p, piece in group]
        if group:
            lt._op("Fold", lambda: FoldEngine.fold_many([p.fold for p, _ in group], rows))
        for (p, piece), n in zip(group, folded):
            lt._book_piece(piece, n, p)
        for p, pc in zip(lt.pulsars, pieces):
            if len(pc) > 1:
                lt._fold_pieces(pc, lambda: lt._op("Fold", lambda: p.fold.fold(rows)), p)

    def finish(self, *exchange):
        """Several pulsars (one GPU): the open sub-integration of each that has folded samples since its last; one: the exchange"""
        lt = self.lt
        if not lt.pulsars:
            return lt._exchange_subint(*exchange)
        for p in lt.pulsars:
            if p.ndat_total:
                lt._finish_pulsar_subint(p)


class DetectFold(_RowFold):
    """Detection + Fold: fused into the filterbank's last pass or on the detected block, with the dump taps, -4, several pulsars
    and -K."""

    detects = True                       # dsp::Detection reads the front end: two polarisations, a convolve_when it knows
    fuses = True                         # the front end may fold in its last pass (cfg.fused_fold)
    engines = ("fold",)
    no_exchange = property(lambda self: "fourth_moment (-4) is" if self.lt.moments else None)

    def plan(self, ntargets, subband, dump_before):
        """-K: dsp::SampleDelay on the filterbank output.  Detection acts sample by sample, so delaying the detected rows gives the
        same numbers as delaying the complex rows first (the reference's order) and keeps the fused filterbank+detect launch group.
        The samples it gives up at the end of a block wait in the head room in front of `detected` (DelayCarry: lt.sd)."""
        lt, cfg, info = self.lt, self.lt.cfg, self.lt.info
        if cfg.interchan_dedispersion:
            dual = info.ndim == 2                              # Observation.C:80-87; Filterbank.C:358-364
            lt._delays = dedispersion_sample_delays(info.centre_frequency, info.bandwidth, cfg.dispersion_measure, cfg.nchan, lt.out_rate,
                                                    swap=dual and info.nchan == 1, nsub_swap=info.nchan if dual and info.nchan > 1 else 0)
            lt.sd = DelayCarry(lt._delays)
            lt.out_start += lt.sd.zero / lt.out_rate                                 # SampleDelay.C:159
        lt._taps = tap_check(cfg, dump_before)

    def open(self, rows, dump_dir):
        lt, cfg, info, nsub = self.lt, self.lt.cfg, self.lt.info, self.lt.cfg.nchan // self.lt.info.nchan
        lt.fold = FoldEngine(lt.ctx)
        self.shape(cfg.nbin)
        if cfg.interchan_dedispersion:
            if lt.subband is None:
                lt.sample_delay = SampleDelay(lt.ctx, lt._delays, lt.npol_out)
            else:
                # a sub-band rank applies ITS channels' delays relative to the zero of the WHOLE band and gives up the
                # whole band's total delay per block, so that every rank emits the same samples with the same start time
                # (SampleDelay.C:75-99 on the full band; the rank's slice goes in as absolute delays)
                applied = lt.sd.zero - np.asarray(lt._delays, np.int64)
                lt.sample_delay = SampleDelay(lt.ctx, applied[lt.subband * nsub:(lt.subband + 1) * nsub], lt.npol_out, absolute=True)
                lt.sd.short = lt.sd.head - lt.sample_delay.total_delay       # samples this rank must NOT emit
            lt.sd.check_block("LoadToFold", rows * lt.nkeep)
        lt.detected = _device_empty(lt.ctx, (lt.nchan_out, lt.npol_out, (lt.sd.head + rows * lt.nkeep) * cfg.ndim))
        # fused filterbank+detect+fold (no detected time series in HBM): ndim 4, three-pass geometries
        # (the library decides whether fusing pays for this geometry; when it does not, this driver keeps the
        # separate Detection and Fold operations on its own `detected` block; -F N:B never fuses)
        if cfg.fused_fold and (cfg.ndim == 4 or lt.square_law) and lt.sample_delay is None and cfg.convolve_when != "before":
            lt.fused_mode = lt.fb.fold_is_fused(lt.detection_state()) if lt.square_law else lt.fb.fold_is_fused()
        lt.fused_fold = lt.fused_mode != 0      # fused_mode 2: sums re-associated per run of parts (engine.fold_is_fused)
        for name in lt._taps:
            from . import dada
            chbw = info.bandwidth / info.nchan
            sub = lt.subband
            fc = info.centre_frequency if sub is None else info.centre_frequency - 0.5 * info.bandwidth + (sub + 0.5) * chbw
            bw = info.bandwidth if sub is None else chbw
            det = name == "Fold"
            path = os.path.join(dump_dir, "pre_%s%s.dump" % (name, "" if sub is None else ".%d" % sub))
            fold_npol, fold_ndim = lt._fold_dims()        # -4: the input of Fold is the FourthMoment stream
            lt.dumps[name] = dada.Dump(
                path, centre_frequency=fc, bandwidth=bw, nchan=lt.nchan_out, npol=fold_npol if det else 2,
                ndim=fold_ndim if det else 2, nbit=32, rate=lt.out_rate, mjd_day=info.mjd_day,
                mjd_sec=info.mjd_sec + lt.out_start,
                state=lt.state_name() if det else "Analytic",
                source=info.source, telescope=info.telescope)
        if "Fold" in lt.dumps:
            lt.fused_mode, lt.fused_fold = 0, False          # the detected samples must exist in HBM to be dumped

    def process(self, raw, npart, events):
        """One fold call covers the block and the fold is fused: filterbank, detection and fold in one launch group -- the same sums
        in the same order as the chain every other block takes: filterbank+detect -> [SampleDelay of -K, in place (LoadToFold1.C:
        617-618)] -> fold, by piece or by pulsar.  Without -K: no head room, nothing carried, every sample delivered."""
        lt, cfg, nd, sd, ndat = self.lt, self.lt.cfg, self.lt.cfg.ndim, self.lt.sd, npart * self.lt.nkeep
        state = lt.detection_state()
        if lt.twobit is not None:
            return self._process_twobit(raw, npart, events, state)
        if "Detection" in lt.dumps:                          # the filterbank's complex output: one extra pass, taps only
            if lt._dump_cplx is None:
                lt._dump_cplx = _device_empty(lt.ctx, (lt.nchan_out, 2, 2 * cfg.parts_per_block * lt.nkeep))
            lt.fb.perform_raw(raw, lt.layout, lt.scale8, lt._dump_cplx, npart)
            lt.dumps["Detection"].write(lt._dump_cplx, ndat, 2)
        pieces = lt._pieces(ndat) if lt.fused_fold else None
        if pieces is not None and len(pieces) == 1 and pieces[0][:2] == (0, ndat):
            lt._fold_pieces(pieces, lambda: lt._filterbank_op("Filterbank+Detection+Fold", lambda: lt.fb.perform_fold(
                lt.fold, npart, state, raw=raw, layout=lt.layout, scale=lt.scale8), events))
            return ndat
        lt._filterbank_op("Filterbank+Detection", lambda: lt.fb.perform_detect(sd.new(lt.detected, nd), npart, state, nd, raw=raw,
                                                                               layout=lt.layout, scale=lt.scale8), events)
        rows, nout = lt.detected, ndat
        if lt.sample_delay is not None:
            rows = sd.rows(lt.detected, ndat, nd)   # (sub-band rank: the band's total delay, not just this rank's, is given up)
            nuse = rows.shape[2] // nd
            nout = lt._op("SampleDelay", lambda: lt.sample_delay.transform(rows.unflatten(2, (nuse, nd)))) if nuse else 0
        if nout and "Fold" in lt.dumps:
            if lt.moments:
                lt.dumps["Fold"].write(self._moment_stream(rows, nout), nout, 14)
            else:
                lt.dumps["Fold"].write(rows, nout, nd)
        if nout and lt.pulsars:
            self._fold_pulsars(rows, nout)
        elif nout:
            lt._fold_pieces(pieces or lt._pieces(nout), lambda: lt._op("Fold", lambda: self._fold_rows(rows)))
        sd.keep_tail(lt.ctx, lt.detected, ndat, nout, nd)
        return nout

    def _process_twobit(self, raw, npart, events, state):
        """A two-bit block: dsp::TwoBitCorrection into float rows (the per-digitiser weights come back with them), then the
        weights' way to the fold on the host -- mask_weights (ExcisionUnpacker.C:243-247), convolve_weights(nsamp_fft, nsamp_step)
        and scrunch_weights(tres_ratio) (Filterbank.C:279-306) -- and the chain every block takes, on the float entry points.  A
        block without a zero weight folds like any other (fused where the front end fuses); one with a zero weight takes
        Detection + Fold, whose plan drops the samples of a zero weight (Fold.C:686-716,746-763).  Blocks overlap by the
        filterbank's tail, whose windows are unpacked again with the block that follows: the weights of a carried tail are
        those it had."""
        from . import twobit
        lt, cfg, nd, tb, ndat = self.lt, self.lt.cfg, self.lt.cfg.ndim, self.lt.twobit, npart * self.lt.nkeep
        nsamp = npart * lt.nsamp_step + lt.nsamp_overlap
        rows, in_step, wdev = lt._op("TwoBitCorrection", lambda: lt.fb.unpack_twobit(raw, tb.first_sample, npart))
        lt.ctx.synchronize()
        w = twobit.mask_weights(wdev.cpu().numpy().view(np.uint32))
        tb.discarded_weights += int((w[0] == 0).sum())                  # get_nzero of the first row
        row, npw, widat = twobit.convolve_weights(w[0], nsamp, tb.nsample, tb.first_sample, lt.nsamp_step + lt.nsamp_overlap, lt.nsamp_step)
        row, npw, widat = twobit.scrunch_weights(row, npw, widat, (lt.nsamp_step + lt.nsamp_overlap) // lt.response.ndat, ndat=nsamp)
        lt._weights = (row, npw, widat) if not row.all() else None
        try:
            pieces = lt._pieces(ndat) if lt.fused_fold and lt._weights is None else None
            if pieces is not None and len(pieces) == 1 and pieces[0][:2] == (0, ndat):
                lt._fold_pieces(pieces, lambda: lt._filterbank_op("Filterbank+Detection+Fold", lambda: lt.fb.perform_fold(
                    lt.fold, npart, state, inp=rows, in_step=in_step), events))
                tb.blocks_fused += 1
                return ndat
            lt._filterbank_op("Filterbank+Detection", lambda: lt.fb.perform_detect(lt.detected, npart, state, nd, inp=rows, in_step=in_step),
                              events)
            lt._fold_pieces(pieces or lt._pieces(ndat), lambda: lt._op("Fold", lambda: lt.fold.fold(lt.detected)))
            tb.blocks_weighted += lt._weights is not None
            return ndat
        finally:
            lt._weights = None

    def _fold_rows(self, rows):
        """Fold::fold of the pending plan over detected rows.  -4: the Stokes rows go to the moments fold, which forms the products
        in registers; with a pre_Fold tap the 14-float stream dsp::FourthMoment would write exists (`_moment_stream`) and is
        folded as it is -- the same bits either way."""
        lt = self.lt
        if not lt.moments:
            return lt.fold.fold(rows)
        if lt._moment_rows is not None:
            return lt.fold.fold(lt._moment_rows)
        return lt.fold.fold_moments(rows)

    def _moment_stream(self, rows, ndat):
        """dsp::FourthMoment on the first `ndat` samples of the Stokes rows (pre_Fold tap of a -4 run): [nchan][1][ndat*14]"""
        lt = self.lt
        need = lt.nchan_out * 14 * (lt.sd_head + lt.cfg.parts_per_block * lt.nkeep)
        if lt._moment_buf is None or lt._moment_buf.numel() < need:
            lt._moment_buf = _device_empty(lt.ctx, need)
        out = lt._moment_buf[:lt.nchan_out * 14 * ndat].view(lt.nchan_out, 1, 14 * ndat)
        lt._op("FourthMoment", lambda: fourth_moment(lt.ctx, rows, out, ndat))
        lt._moment_rows = out
        return out

    def shape(self, nbin):
        self.lt.fold.set_shape(self.lt.nchan_out, *self.lt._fold_dims(), nbin)
        self.lt.hits = np.zeros(nbin, dtype=np.uint32)


class DetectedFold(_RowFold):
    """Detected input (info.detected, a SIGPROC filterbank file): the first branch of LoadToFold::construct (LoadToFold1.C:126-180)
    -- no filterbank, no convolution, no Detection: dsp::SigProcUnpacker writes the float rows, [dsp::SampleDelay of -K removes the
    inter-channel delay,] Fold folds them, by piece or by pulsar.  A block is a run of whole spectra as they lie in the file: a
    part is one spectrum (lt.nkeep = nsamp_step = 1, no overlap), so the books of every other mode carry over."""

    detects = fuses = fronted = False
    engines = ("fold",)
    no_exchange = "detected input is"

    def state_name(self):
        return self.lt.info.detected

    def vitals(self):
        return ["dspsr: blocksize=%d samples or %g MB" % (self.lt.cfg.parts_per_block, self.lt.block_bytes() / (1024.0 * 1024.0))]

    def plan(self, ntargets, subband, dump_before):
        """No response and no front end; -K: dsp::SampleDelay on the file's own channels, the samples it gives up at the end of a
        block wait in the head room in front of `detected` (DelayCarry: lt.sd), exactly as DetectFold.plan has it."""
        lt, cfg, info = self.lt, self.lt.cfg, self.lt.info
        lt.in_nchan = lt.nchan_out = info.nchan
        lt.npol_out = info.npol
        lt.response = None
        lt.out_rate, lt.out_start, lt.scalefac = info.rate, info.start_seconds, 1.0
        lt.nkeep, lt.nsamp_step, lt.nsamp_overlap = 1, 1, 0
        lt.layout, lt.scale8 = lt.form.layout, 1.0
        if cfg.interchan_dedispersion:
            lt._delays = dedispersion_sample_delays(info.centre_frequency, info.bandwidth, cfg.dispersion_measure, info.nchan, lt.out_rate)
            lt.sd = DelayCarry(lt._delays)
            lt.out_start += lt.sd.zero / lt.out_rate                                 # SampleDelay.C:159

    def open(self, rows, dump_dir):
        lt, cfg = self.lt, self.lt.cfg
        lt.fold = FoldEngine(lt.ctx)
        self.shape(cfg.nbin)
        if cfg.interchan_dedispersion:
            lt.sample_delay = SampleDelay(lt.ctx, lt._delays, lt.npol_out)
            lt.sd.check_block("LoadToFold", rows)
        # every row starts on a 16-byte boundary whatever the head room: float4 stores for whole tiles of a block
        pad = (-lt.sd.head) % 4
        span = pad + lt.sd.head + rows
        self.buffer = _device_empty(lt.ctx, (lt.nchan_out, lt.npol_out, span + (-span) % 4))
        lt.detected = self.buffer[:, :, pad:]

    def shape(self, nbin):
        self.lt.fold.set_shape(self.lt.nchan_out, self.lt.npol_out, 1, nbin)
        self.lt.hits = np.zeros(nbin, dtype=np.uint32)

    def process(self, raw, ndat, events):
        """SigProcUnpacker behind the head room -> [SampleDelay in place over the carried tail and the new samples] -> Fold -> the
        unshifted tail kept in front of the next block.  Without -K: no head room, nothing carried, every sample delivered."""
        lt, info, sd = self.lt, self.lt.info, self.lt.sd
        lt._filterbank_op("SigProcUnpacker", lambda: unpack_sigproc_fpt(lt.ctx, raw, sd.new(lt.detected), info.nbit, info.nchan, info.npol, ndat),
                          events)
        rows, nout = lt.detected[:, :, :ndat], ndat
        if lt.sample_delay is not None:
            rows = sd.rows(lt.detected, ndat)
            nout = lt._op("SampleDelay", lambda: lt.sample_delay.transform(rows)) if rows.shape[2] else 0
        if nout and lt.pulsars:
            self._fold_pulsars(rows, nout)
        elif nout:
            lt._fold_pieces(lt._pieces(nout), lambda: lt._op("Fold", lambda: lt.fold.fold(rows)))
        sd.keep_tail(lt.ctx, lt.detected, ndat, nout)
        return nout


class CyclicFold(_BackEnd):
    """`dspsr -cyclic N`: the convolving filterbank writes its complex rows, dsp::CyclicFold folds their lag products
    (LoadToFold1.C:534-539,999-1044); Detection and Fold are not built.  At a sub-integration the lag data come to the
    host and CyclicFoldEngine::synch turns them into spectra (once per sub-integration: host, as in the reference)."""

    detects = fuses = False
    engines = ("cyclic",)
    no_exchange = "cyclic spectra are"

    def __init__(self, lt):
        self.lt = lt

    def plan(self, ntargets, subband, dump_before):
        self.geometry = cyclic_geometry(self.lt.cfg, self.lt.info)
        self.lt.npol_out = self.geometry["npol"]

    def shape(self, nbin):
        lt, g = self.lt, self.geometry
        lt.cyclic.set_shape(lt.nchan_out, lt.info.npol, g["npol"], g["nlag"], g["mover"], nbin)
        lt.hits = np.zeros(nbin, dtype=np.uint32)

    def open(self, rows, dump_dir):
        lt = self.lt
        lt.cyclic = CyclicFoldEngine(lt.ctx)
        self.shape(lt.cfg.nbin)
        lt.voltages = _device_empty(lt.ctx, (lt.nchan_out, lt.info.npol, 2 * rows * lt.nkeep))

    def process(self, raw, npart, events):
        """Filterbank -> complex rows -> CyclicFold piece by piece (Subint<CyclicFold>).  Lag products never span two fold
        calls (CyclicFold.C:390: idat < ndat_fold - nlag), so the last nlag samples of every piece add nothing."""
        lt, ndat = self.lt, npart * self.lt.nkeep
        lt._filterbank_op("Filterbank", lambda: lt.fb.perform_raw(raw, lt.layout, lt.scale8, lt.voltages, npart), events)
        lt._fold_pieces(lt._pieces(ndat), lambda: lt._op("CyclicFold", lambda: lt.cyclic.fold(lt.voltages)))
        return ndat

    def plan_piece(self, acc, phi, phase_per_sample, ndat_fold, idat_start):
        self.lt.cyclic.set_ndat(ndat_fold, idat_start)
        return self.lt.cyclic.set_bins(phi, phase_per_sample, ndat_fold, idat_start, acc.hits)

    def finish(self, *_exchange):
        """CyclicFoldEngine::synch (CyclicFold.C:450-555): spectra [nchan * nchan_spec / mover][npol][nbin][1] on the host"""
        lt = self.lt
        if not lt.ndat_total:                                # nothing folded since the last one (as the multi-pulsar branch)
            return
        spectra = lt._op("CyclicFold::synch", lambda: lt.cyclic.synch())
        _emit(lt, _books(lt, profile=spectra[..., None]), lt.cyclic.zero)


class PhaseLockedFold(_BackEnd):
    """`dspsr -G nbin`: the convolving filterbank writes its complex rows and dsp::PhaseLockedFilterbank consumes them
    (LoadToFold1.C:386-456); Detection and Fold are not built.  One integration over the whole stream: the windows are those
    of ONE transformation call (PlfbPlan), whatever the block size.  The rows of a block sit behind a head room that holds the
    carried tail -- the samples from the first window that does not fit yet -- so that a window may span two blocks.  It has
    no pieces: no sub-integrations."""

    detects = fuses = False
    engines = ("plfb",)
    no_exchange = "the phase-locked filterbank is"
    shape = None                         # (nothing follows a target's nbin: the phase bins are plfb_nbin; -b plays no part)

    def __init__(self, lt):
        self.lt = lt

    def plan(self, ntargets, subband, dump_before):
        """PhaseLockedFilterbank::prepare (:59-83), all on the host."""
        lt, cfg, info = self.lt, self.lt.cfg, self.lt.info
        period, polyco, reference_phase = lt._ephemeris()
        if period <= 0:
            period = 1.0 / polyco.frequency(info.mjd_day, info.mjd_sec + lt.out_start)
        nmax = plfb_choose_nchan(period, lt.out_rate, cfg.plfb_nbin)
        nchan = cfg.plfb_nchan if cfg.plfb_nchan >= 2 else nmax
        if nchan > nmax:
            import warnings
            warnings.warn("dsp::PhaseLockedFilterbank::prepare warning selected nchan=%d > suggested max=%d" % (nchan, nmax))
        plfb_check_shape(cfg.nchan, info.npol, 2, nchan, cfg.npol, cfg.plfb_nbin)       # the rows are Analytic: ndat_fft = nchan
        state = {1: "Intensity", 2: "PPQQ", 4: "Coherence"}[cfg.npol]                  # :128-133
        lt.plfb_geometry = {"nchan_fft": nchan, "ndat_fft": nchan, "nchan": cfg.nchan * nchan, "npol": cfg.npol, "ndim": 1,
                            "nbin": cfg.plfb_nbin, "state": state, "rate": lt.out_rate / nchan, "nsub_swap": cfg.nchan,
                            "scale": lt.scalefac * nchan}                              # :143-149
        lt.npol_out = cfg.npol
        self.windows = PlfbPlan(lt._turns_divider(*lt._ephemeris(), turns=1.0 / cfg.plfb_nbin), cfg.plfb_nbin, reference_phase, nchan)
        self.carry = DelayCarry(head=nchan)

    def open(self, rows, dump_dir):
        lt, cfg, info = self.lt, self.lt.cfg, self.lt.info
        lt.plfb = PhaseLockedFilterbankEngine(lt.ctx)
        lt.plfb.set_shape(cfg.nchan, info.npol, 2, lt.plfb_geometry["nchan_fft"], cfg.npol, cfg.plfb_nbin)
        lt.voltages = _device_empty(lt.ctx, (lt.nchan_out, info.npol, 2 * (self.carry.head + rows * lt.nkeep)))
        lt.hits = np.zeros(cfg.plfb_nbin, dtype=np.uint32)

    def process(self, raw, npart, events):
        """Filterbank -> complex rows behind the carried tail -> every window of the plan that now lies inside the rows, in one
        accumulate call; then the samples from the next window's start on are carried in front of the next block's rows."""
        lt, carry, ndat = self.lt, self.carry, npart * self.lt.nkeep
        nin = carry.carried + ndat
        lt._filterbank_op("Filterbank", lambda: lt.fb.perform_raw(raw, lt.layout, lt.scale8, carry.new(lt.voltages, 2), npart), events)
        base, avail = lt.ndat_out - carry.carried, lt.ndat_out + ndat     # stream samples of the first row sample / behind the last
        starts, bins = self.windows.take(avail)
        if len(starts):
            rows = carry.rows(lt.voltages, ndim=2)
            rel = (starts.astype(np.int64) - base).astype(np.uint64)
            lt._op("PhaseLockedFilterbank", lambda: lt.plfb.accumulate(rows, nin, rel, bins))
            time_per_fft = float(lt.plfb_geometry["ndat_fft"]) / lt.out_rate
            for b in bins:                                            # PhaseLockedFilterbank.C:233-235, window by window
                lt.hits[b] += 1
                lt.ndat_total += 1
                lt.integration_length += time_per_fft
        nxt = self.windows.next_start()
        keep = avail - nxt if nxt < avail else 0                      # (< ndat_fft: the window at nxt does not fit)
        carry.keep_tail(lt.ctx, lt.voltages, ndat, nin - keep, 2)
        return ndat

    def finish(self, *_exchange):
        """The integration so far: profile [nchan * nchan_fft][npol][nbin][1] on the host, with the members
        PhaseLockedFilterbank.C:123-159 sets on its output"""
        lt = self.lt
        if not lt.ndat_total:
            return
        prof = lt._op("PhaseLockedFilterbank::synch", lambda: lt.plfb.synch())
        _emit(lt, _books(lt, profile=prof[..., None], **{k: lt.plfb_geometry[k] for k in ("state", "rate", "nsub_swap", "scale")}), lt.plfb.zero)


class KurtosisFold(_BackEnd):
    """`dspsr -skz`: the convolving filterbank writes its complex rows, dsp::SpectralKurtosis zeroes what it zaps in place,
    Detection and Fold follow; the fold counts its hits per channel on the device (Fold::Engine::zeroed_samples with
    hits_nchan == nchan, LoadToFold1.C:458-532, Fold.C:853-866).  The rows of a block sit behind a head room that holds the
    carried tail, the < M samples SpectralKurtosis has not consumed yet (InputBuffering, set_next_start(output_ndat):
    SpectralKurtosis.C:211-217)."""

    detects, fuses = True, False
    engines = ("fold", "sk")
    no_exchange = "spectral kurtosis (-skz) is"

    def __init__(self, lt):
        self.lt = lt

    def plan(self, ntargets, subband, dump_before):
        tap_check(self.lt.cfg, dump_before)                  # (chan_range is sk_check's: the driver's plan asks it last)
        self.carry = DelayCarry(head=self.lt.cfg.sk_m - 1)

    def open(self, rows, dump_dir):
        lt, cfg, info = self.lt, self.lt.cfg, self.lt.info
        lt.fold = FoldEngine(lt.ctx)
        self.shape(cfg.nbin)
        lt.sk = SpectralKurtosisEngine(lt.ctx)
        lt.sk.set_shape(lt.nchan_out, info.npol, cfg.sk_m)
        lt.sk.set_options(cfg.sk_std_devs, *self.chan_range, cfg.sk_no_fscr, cfg.sk_no_tscr, cfg.sk_no_ft)
        lt.voltages = _device_empty(lt.ctx, (lt.nchan_out, info.npol, 2 * (self.carry.head + rows * lt.nkeep)))
        lt.detected = _device_empty(lt.ctx, (lt.nchan_out, lt.npol_out, (self.carry.head + rows * lt.nkeep) * cfg.ndim))

    def shape(self, nbin):
        lt = self.lt                   # (hits per channel: uint32 [nchan][nbin] on the device, on the host at a sub-integration)
        lt.fold.set_shape(lt.nchan_out, lt.npol_out, lt.cfg.ndim, nbin)
        self.hits_dev = _device_empty(lt.ctx, (lt.nchan_out, nbin), "int32", zero=True)
        lt.hits = np.zeros((lt.nchan_out, nbin), dtype=np.uint32)

    def process(self, raw, npart, events):
        """Filterbank -> complex rows behind the carried tail -> SpectralKurtosis over the whole parts of M samples (in place: zeros
        over what it zaps) -> Detection -> Fold piece by piece, hits counted where the detected sample is not zero; the remainder is
        carried in front of the next block's rows.  The last < M samples of a run are dropped, as the reference drops them."""
        lt, cfg, carry, ndat = self.lt, self.lt.cfg, self.carry, npart * self.lt.nkeep
        nin = carry.carried + ndat
        lt._filterbank_op("Filterbank", lambda: lt.fb.perform_raw(raw, lt.layout, lt.scale8, carry.new(lt.voltages, 2), npart), events)
        rows = carry.rows(lt.voltages, ndim=2)
        nuse = nin // cfg.sk_m * cfg.sk_m
        if nuse:
            lt._op("SpectralKurtosis", lambda: lt.sk.transform(rows, rows, nin))
            det = lt.detected[:, :, :nuse * cfg.ndim]
            state = _lib.STOKES if cfg.stokes else _lib.COHERENCE
            lt._op("Detection", lambda: DetectionEngine(lt.ctx).polarimetry(cfg.ndim, rows[:, :, :2 * nuse], det, state))
            lt._fold_pieces(lt._pieces(nuse), lambda: lt._op("Fold", lambda: lt.fold.fold_zeroed(det, self.hits_dev)))
        carry.keep_tail(lt.ctx, lt.voltages, ndat, nuse, 2)
        return nuse

    def plan_piece(self, acc, phi, phase_per_sample, ndat_fold, idat_start):
        fold = self.lt.fold                                  # (the hits are the device's: the books get the samples only)
        fold.set_nbin(self.lt.cfg.nbin)
        fold.set_ndat(ndat_fold, idat_start)
        fold.set_bins(phi, phase_per_sample, ndat_fold, idat_start, None)

    def finish(self, *_exchange):
        """The hits come to the host; integration_length = hits.sum() / (rate * nchan), once, from the integer total (Fold.C:893-896)"""
        lt = self.lt
        if not lt.ndat_total:
            return
        lt.hits = self.hits_dev.cpu().numpy().view(np.uint32)
        lt.integration_length = float(int(lt.hits.sum(dtype=np.uint64))) / (lt.out_rate * lt.nchan_out)
        lt.sk_statistics = lt.sk.get_statistics()
        _emit(lt, _books(lt, profile_dev=lt.profiles_tensor().clone()), lambda: (lt.fold.zero(), self.hits_dev.zero_()))


class LoadToFold:
    """One pipeline instance = one GPU = one stream (SingleThread).  `raw` blocks are int8 torch
    tensors already resident on the device (the PCIe copy is the caller's, as TransferCUDA is a
    separate Operation in the reference).

    Construction is `_plan` -- host code: every refusal that needs no device, every derived number -- then `_open`, which only opens
    things; whatever raises in it, close() releases what was opened so far."""

    sd_head, sd_carried, sd_short = _carry_view("head"), _carry_view("carried"), _carry_view("short")

    def __init__(self, cfg: Config, info: InputInfo, device: int = 0, stream: int | None = None,
                 polyco: Polyco | None = None, reference_phase: float = 0.0, subband: int | None = None,
                 dump_before=(), dump_dir=".", targets=None):
        """targets: FoldTarget list, one Fold per pulsar (dspsr -P a -P b / -c p1 -c p2, LoadToFold1.C:917-960).  They replace
        polyco / reference_phase / cfg.folding_period, and cfg.nbin by each target's nbin, or by Fold::choose_nbin for its period
        where the target's nbin is 0 (also with a single target).  One target: the single-pulsar path of this class, unchanged.  Several: `pulsars` holds one fold engine, hits, sub-integration divider and `subints` list per
        target; Detection writes the detected rows and the pulsars fold them with FoldEngine.fold_many (the rows are read once);
        `subints` / `hits` of the instance itself stay empty.  Multi-GPU exchange (subband, communicators) is single-pulsar only.

        subband = g: this instance is rank g of a sub-band sharded run.  `info`/`cfg` still describe the
        WHOLE band (info.nchan input channels, cfg.nchan output channels); the instance processes input channel g only:
        its block holds that channel's bytes alone ([t][pol][dim], what a rank reads from the NCHAN-interleaved file),
        its kernel is the g-th slice of the ONE full-band kernel (Filterbank.C:563, FilterbankCUDA.cu:249-251) with the
        COMMON nfilt_pos/neg, so all ranks stay sample aligned and fold with identical hits."""
        targets = list(targets or [])
        self._defaults()
        self._plan(cfg, info, polyco, reference_phase, subband, tuple(dump_before), targets)
        try:
            self._open(device, stream, dump_dir)
            if targets:
                self._init_targets(targets)
        except BaseException:
            self.close()
            raise

    def _defaults(self):
        """Every field the class reads later; a path overrides only what differs."""
        import torch
        self.torch = torch
        self.pulsars, self.cyclic, self.plfb, self.rfi_filter = [], None, None, None
        self.sk, self.sk_statistics = None, None
        self.square_law = None              # (state name, library state, npol_out) of -d 1 / -d 2 / one polarisation; None: the four products
        self.twobit, self._weights = None, None   # NBIT 2: the TwoBitPlan; the weights of the block in hand (row, ndatperweight, weight_idat)
        self.ctx = self.fb = self.fold = self.response = self.sample_delay = self.detected = self.voltages = None
        self.sd = DelayCarry()               # -K: head room in front of `detected` and the tail carried in it
        self.mode = DetectFold(self)        # the back end; _plan chooses the one of the run
        self.fused_mode, self.fused_fold = 0, False
        self.optime = {}                    # record_time: operation name -> [seconds, calls]
        self.dumps, self._dump_cplx = {}, None
        self._turns, self._moment_rows, self._moment_buf = None, None, None
        self._calibrated, self._delays, self._taps = None, None, ()
        self._closed = False
        # fold bookkeeping (PhaseSeries)
        self.hits = np.zeros(0, dtype=np.uint32)
        self.integration_length, self.ndat_total = 0.0, 0
        self.nsamples_in = 0                # unique input samples consumed (per pol)
        self.ndat_out = 0                   # output samples produced so far
        self.subints = []                   # completed sub-integrations (host copies) on the writer rank

    def _plan(self, cfg, info, polyco, reference_phase, subband, dump_before, targets):
        """The host side of the constructor: what the run refuses, in the order it always has, and every number that needs no device."""
        # the form of the blocks: a sub-band rank reads one channel's runs of a GUPPI block, a two-bit run whole excision windows
        self.form = raw_form(info, channel_sharded=subband is not None, excision_nsample=cfg.excision_nsample)
        detected = self.form.name == "detected"
        if detected:                                     # a SIGPROC filterbank file: nbit counts bits per detected value
            cfg = detected_check(cfg, info, subband, dump_before)
        elif self.form.name == "twobit":
            self.twobit = twobit_check(cfg, info, len(targets), subband, dump_before)
        if cfg.zap_rfi:
            rfi_check(cfg, info, subband)
        self._calibrated = calibrator_response(cfg, info, subband)      # -pac
        if cfg.plfb_nbin > 0:
            plfb_check(cfg, info, len(targets), subband, dump_before)
        self.moments = fourth_moment_active(cfg)         # -4: the fold is (nchan, 1, 14, nbin), fed by FoldEngine.fold_moments
        cfg = fourth_moment_check(cfg, len(targets), subband)
        if cfg.cyclic_nchan > 0:
            cyclic_check(cfg, info, len(targets), subband, dump_before)
        if len(targets) > 1 and subband is not None:
            raise DspsrAmdError("dspsr_amd.LoadToFold: sub-band sharded runs fold one pulsar; %d targets given" % len(targets))
        for t in targets:
            if t.polyco is None and t.folding_period <= 0:
                raise DspsrAmdError("dsp::Fold::fold no polynomial and no period specified (target %r)" % (t.name,))
        if targets:
            t = targets[0]
            cfg = dataclasses.replace(cfg, folding_period=t.folding_period if t.polyco is None else 0.0)
            polyco, reference_phase = t.polyco, t.reference_phase
        self.cfg, self.info, self.polyco = cfg, info, polyco
        self.reference_phase = reference_phase
        self.subband = subband
        if subband is not None and not 0 <= subband < info.nchan:
            raise DspsrAmdError("dspsr_amd.LoadToFold: subband=%d outside the %d input channels" % (subband, info.nchan))
        if cfg.folding_period <= 0 and polyco is None:
            raise DspsrAmdError("dsp::Fold::fold no polynomial and no period specified")   # Fold.C:638-640
        # the back end of the run: every later question about the mode is put to it
        self.mode = (DetectedFold if detected else CyclicFold if cfg.cyclic_nchan > 0 else PhaseLockedFold if cfg.plfb_nbin > 0
                     else KurtosisFold if cfg.sk_zap else DetectFold)(self)
        if not self.mode.fronted:                        # no front end, no response: the back end plans the whole run
            self.square_law = None
            return self.mode.plan(len(targets), subband, dump_before)
        # -d 1, -d 2, one polarisation: Detection::square_law, rows and profile of npol_out x ndim 1 (cfg.ndim, the layout of the
        # four products, then says 1 wherever this class reads it)
        self.square_law = square_law_state(cfg, info)
        if self.square_law:
            square_law_check(cfg, info)
            if info.npol == 1:
                print("Only single polarization detection available", file=sys.stderr)          # LoadToFold1.C:1114
            self.cfg = cfg = dataclasses.replace(cfg, ndim=1)
        if self.mode.detects:                                            # (-cyclic and -G read the complex rows of -F N:D)
            if info.npol != 2 and not self.square_law:
                raise DspsrAmdError("dsp::Detection::polarimetry Cannot detect polarization when npol != 2")
            if cfg.convolve_when not in ("during", "after", "before", "never"):
                raise DspsrAmdError("dspsr_amd.LoadToFold: convolve_when=%r is not one of during / after / before / never" % (cfg.convolve_when,))
        if cfg.nchan % info.nchan:
            raise DspsrAmdError("dsp::Filterbank::make_preparations output nchan=%d not a multiple of input nchan=%d"
                                % (cfg.nchan, info.nchan))
        self.in_nchan = 1 if subband is not None else info.nchan         # input channels in this instance's blocks
        self.nchan_out = (cfg.nchan // info.nchan) * self.in_nchan       # output channels this instance produces
        self.npol_out = self.square_law[2] if self.square_law else 4 // cfg.ndim
        if cfg.convolve_when != "during":
            self._plan_after(subband, dump_before)
        else:
            # -F N:D: the response inside the filterbank (LoadToFold1.C:318-323; -K: the fractional delays with it, :620-621)
            self.response = r = matched_response(info, cfg.dispersion_measure, cfg.freq_res, cfg.nchan, input_nchan=info.nchan,
                                                 ndim=info.ndim, fractional_delay=cfg.interchan_dedispersion)
            self.out_rate, self.out_start, self.scalefac = filterbank_output(info, r, cfg.nchan // info.nchan)
        self.mode.plan(len(targets), subband, dump_before)
        if cfg.sk_zap:                           # after every refusal the run had without -skz (with -cyclic or -G: it refuses)
            self.mode.chan_range = sk_check(cfg, info, len(targets), subband, dump_before)

    def _plan_after(self, subband, dump_before):
        """`dspsr -F N` (Filterbank::Config::After) and the filterbank without coherent dedispersion (Config::Never): the non-convolving
        filterbank (freq_res = 1) followed by dsp::Convolution on its output channels (LoadToFold1.C:296-380).  The response is matched
        to the FILTERBANK'S OUTPUT observation (Convolution.C:105-130 -> Dedispersion::match(input)): cfg.nchan channels, complex,
        dual sideband and DC centred (Filterbank.C:341-348: freq_res = 1), band swapped when the input was single-channel dual
        sideband (:358-364; a multi-channel dual-sideband input sets nsub_swap, which Response::match does not read, Response.C:132-181).
        `dspsr -F N:B` (Config::Before): Convolution::prepare -> Dedispersion::match(input), ONE response per input channel, over
        its whole width."""
        cfg, info = self.cfg, self.info
        if subband is not None:
            raise DspsrAmdError("dspsr_amd.LoadToFold: sub-band sharded runs are built for -F N:D (convolve_when = during)")
        if cfg.interchan_dedispersion or dump_before:
            raise DspsrAmdError("dspsr_amd.LoadToFold: -K and the dump taps are built for -F N:D (convolve_when = during)")
        nsub = cfg.nchan // info.nchan
        if cfg.convolve_when == "before":
            self.response = r = matched_response(info, cfg.dispersion_measure, cfg.freq_res, info.nchan, input_nchan=info.nchan, ndim=info.ndim)
            conv_rate = info.rate * (0.5 if info.ndim == 1 else 1.0)                           # Convolution.C:266-267
            self.out_rate = conv_rate / float(nsub)                                            # Filterbank.C:338-339
            self.out_start = info.start_seconds + r.impulse_pos / conv_rate                   # Convolution.C:300
            nsamp_fft = 2 * r.ndat if info.ndim == 1 else r.ndat
            self.scalefac = float(nsamp_fft) * float(r.ndat) * float(nsub)                    # Convolution.C:305, Filterbank.C:124-125
            return
        r = None
        if cfg.convolve_when == "after":
            r = matched_response(info, cfg.dispersion_measure, cfg.freq_res, cfg.nchan, input_nchan=cfg.nchan, ndim=2, dual_sideband=1,
                                 dc_centred=True, swap=(info.ndim == 2 and info.nchan == 1))
        self.response = r
        nsamp_fft_front = 2 * nsub if info.ndim == 1 else nsub                           # input samples per filterbank output sample
        self.out_rate = info.rate / float(nsamp_fft_front)                               # Filterbank.C:338-339: freq_res / nsamp_fft
        ndat = r.ndat if r is not None else 1
        self.out_start = info.start_seconds + (r.impulse_pos if r is not None else 0) / self.out_rate   # Convolution.C:300
        self.scalefac = float(nsub) * (float(ndat) * float(ndat) if r is not None else 1.0)            # Filterbank.C:124-125, Convolution.C:305

    def _open(self, device, stream, dump_dir):
        """The device side of the constructor: the context, the front end, then what the back end opens -- the fold of the mode,
        the block the two share."""
        cfg, info, r = self.cfg, self.info, self.response
        self.ctx = Context(device, stream)
        if not self.mode.fronted:                        # detected input: self.fb stays None
            return self.mode.open(cfg.parts_per_block, dump_dir)
        nsub, rows = cfg.nchan // info.nchan, cfg.parts_per_block
        setup = dict(max_parts=cfg.max_parts, force_four_pass=0 if cfg.two_pass else 2, fuse_heaps=cfg.fuse_heaps)
        fused = _lib.FUSED_NEVER if not (cfg.fused_fold and self.mode.fuses) else _lib.FUSED_ALWAYS if cfg.force_fused else _lib.FUSED_AUTO
        if cfg.convolve_when == "during":
            # -pac: chirp x Jones per bin as a matrix response instead of the chirp (calibrator_response)
            matrix = self._calibrated[1] if self._calibrated else None
            kernel = None if matrix is not None else r.kernel
            if self.subband is not None:
                kernel = kernel[self.subband * nsub * r.ndat:(self.subband + 1) * nsub * r.ndat]
            _open_convolving_front(self, r, nsub, self.in_nchan, kernel, fused_fold=fused, response_matrix=matrix, **setup)
            if self.twobit is not None:
                tb = self.twobit
                self.fb.set_twobit(tb.nsample, tb.nlow_min, tb.nlow_max, tb.levels, tb.table_type)
        elif cfg.convolve_when == "before":
            _adopt_front(self, ConvolutionThenFilterbank(self.ctx, nsub, info.nchan, info.npol, info.ndim == 1, r, max_parts=cfg.max_parts,
                                                         parts_per_block=rows))
        else:
            _adopt_front(self, FilterbankThenConvolution(self.ctx, nsub, info.nchan, info.npol, info.ndim == 1, r, max_parts=cfg.max_parts,
                                                         parts_per_block=rows, fused_fold=fused))
        self.mode.open(rows, dump_dir)

    def _filterbank_op(self, name, fn, events):
        """The filterbank step of a block as an operation, between the caller's two HIP events (bench.py's roofline brackets the
        FFT + chirp launch group with them)."""
        if events is not None:
            events[0].record()
        self._op(name, fn)
        if events is not None:
            events[1].record()

    def _init_targets(self, targets):
        """nbin per target (Fold::choose_nbin for its period where the target gives none); several targets: one FoldEngine each,
        the fused fold off (the detected rows are shared)."""
        if self.mode.shape is None:
            return
        nbins = []
        for t in targets:
            p = t.folding_period if t.polyco is None else 1.0 / t.polyco.frequency(self.info.mjd_day, self.info.mjd_sec + self.out_start)
            nbins.append(t.nbin or choose_nbin(p, self.out_rate))
        if len(targets) == 1:
            if nbins[0] != self.cfg.nbin:
                self.cfg = dataclasses.replace(self.cfg, nbin=nbins[0])
                self.mode.shape(nbins[0])
            return
        self.fused_mode, self.fused_fold = 0, False
        self.fold.close()
        self.fold = None
        for t, nbin in zip(targets, nbins):
            self.pulsars.append(_PulsarFold(t, nbin, FoldEngine(self.ctx)))      # (listed first: close() finds it if set_shape raises)
            self.pulsars[-1].fold.set_shape(self.nchan_out, self.npol_out, self.cfg.ndim, nbin)

    def set_rfi_filter(self, filt):
        """`dspsr -R`: multiply the filter's mask into the dedispersion kernel (ResponseProduct, LoadToFold1.C:248-266) and hand the
        product to the engine through set_kernel -- between blocks: the stream is drained first.  filt: dspsr_amd.rfi.RfiFilter
        (calculated here if it has not been), or None to restore the dedispersion kernel alone.  The reference matches the
        response once (Filterbank.C:84, Convolution.C:115): call this once, before the first block."""
        rfi_check(self.cfg, self.info, self.subband)
        # the engine that holds the response: the convolving filterbank (-F N:D, every back end), or the Convolution of -F N / -F N:B
        r, eng = self.response, self.fb if self.cfg.convolve_when == "during" else self.fb.conv
        if r is None or eng is None:
            raise DspsrAmdError("dspsr_amd.LoadToFold: the RFI filter (-R) needs a dedispersion kernel to multiply into")
        kernel = r.kernel if filt is None else filt.product(r.kernel, r.kernel.size // r.ndat, r.ndat)
        self.ctx.synchronize()
        eng.set_kernel(kernel)
        self.rfi_filter = filt

    def detection_state(self):
        """the library's state of the detected rows: INTENSITY (also PP of one polarisation) / PPQQ for -d 1 / -d 2, else STOKES or COHERENCE"""
        return self.square_law[1] if self.square_law else _lib.STOKES if self.cfg.stokes else _lib.COHERENCE

    def state_name(self):
        """Observation::get_state of the folded PhaseSeries (the STATE of its files and of the pre_Fold tap)"""
        own = self.mode.state_name()                       # (detected input: the file's)
        if own is not None:
            return own
        return "FourthMoment" if self.moments else self.square_law[0] if self.square_law else "Stokes" if self.cfg.stokes else "Coherence"

    def _fold_dims(self):
        """(npol, ndim) of the folded PhaseSeries: those of the detected rows, or 1 x 14 for -4 (FourthMoment.C:39-42)"""
        return (1, 14) if self.moments else (self.npol_out, self.cfg.ndim)

    def _op(self, name, fn):
        """Operation::operate with record_time (Operation.C:90-113): wall time of the operation including its stream
        synchronisation, accumulated per name."""
        if not self.cfg.record_time:
            return fn()
        import time as _time
        self.ctx.synchronize()
        t0 = _time.perf_counter()
        r = fn()
        self.ctx.synchronize()
        e = self.optime.setdefault(name, [0.0, 0])
        e[0] += _time.perf_counter() - t0
        e[1] += 1
        return r

    def vitals(self):
        """The lines `dspsr` prints while it prepares (report_vitals, LoadToFold1.C:773-792,874-879): dedispersion filter
        length, what the filterbank requires, the block size."""
        r, cfg = self.response, self.cfg
        own = self.mode.vitals()                          # (detected input: no filter and no filterbank, the block alone)
        if own is not None:
            return own
        if r is None:                                     # Config::Never: no response
            from types import SimpleNamespace
            r = SimpleNamespace(ndat=1, minimum_ndat=0)
        nsamp_fft = self.nsamp_step + self.nsamp_overlap
        nblock = cfg.parts_per_block * self.nsamp_step + self.nsamp_overlap
        return ["dspsr: dedispersion filter length=%d (minimum=%d) complex samples" % (r.ndat, r.minimum_ndat),
                "dspsr: %d channel dedispersing filterbank requires %d samples" % (cfg.nchan, nsamp_fft),
                "dspsr: blocksize=%d samples or %g MB" % (nblock, self.block_bytes() / (1024.0 * 1024.0))]

    def report(self, file=None):
        """Operation::report (Operation.C:168-190): the table `dspsr -r` prints -- name, time spent, discarded weights."""
        import sys
        file = file or sys.stderr
        if not self.optime:
            return
        pad = lambda t: ("%-25s" % t)
        print(pad("Operation") + pad("Time Spent") + pad("Discarded"), file=file)
        for name, (t, _n) in self.optime.items():
            discarded = self.twobit.discarded_weights if self.twobit is not None and name == "TwoBitCorrection" else 0
            print(pad(name) + pad("%g" % t) + pad("%d" % discarded), file=file)

    # bytes of one block of `npart` parts
    def block_bytes(self, npart=None, first_sample=0):
        """first_sample: where in its first heap, GUPPI raw block or excision window the block begins (0 for every other form)."""
        nsamp = (npart or self.cfg.parts_per_block) * self.nsamp_step + self.nsamp_overlap
        return self.form.block_bytes(nsamp, self.in_nchan, self.info.npol, self.info.ndim, first_sample)

    def seek_block(self, k):
        """Time-slice replicas: the next block is block k of the stream (blocks of parts_per_block parts), not the one
        following the last (MultiThread.C:120-148 hands whole blocks to the threads in turn)."""
        self.ndat_out = k * self.cfg.parts_per_block * self.nkeep

    def _ephemeris(self, pulsar=None):
        """(folding_period, polyco, reference_phase) of the single pulsar, or of `pulsar` of a multi-target run"""
        if pulsar is None:
            return self.cfg.folding_period, self.polyco, self.reference_phase
        t = pulsar.target
        return (t.folding_period if t.polyco is None else 0.0), t.polyco, t.reference_phase

    def _phase(self, t_seconds, pulsar=None):
        """Fold::get_phi / get_pfold (Fold.C:943-958)."""
        period, polyco, reference_phase = self._ephemeris(pulsar)
        if period > 0:
            p = period
            return math.fmod(t_seconds, p) / p - reference_phase, p
        day, sec = self.info.mjd_day, self.info.mjd_sec + t_seconds
        return polyco.phase_frac(day, sec) - reference_phase, 1.0 / polyco.frequency(day, sec)

    def process_block(self, raw, npart=None, events=None, first_sample=0):
        """raw: device int8 tensor holding npart*nsamp_step + nsamp_overlap samples (the InputBuffering
        tail of the previous block already prepended, Filterbank.C:443-444).  A block of MeerKAT heaps holds the whole heaps
        around those samples; first_sample: where in its first heap the block's first sample lies.  A block of a GUPPI raw file
        (info.guppi) holds the whole data sections around them; first_sample: where in the first one's runs that sample lies."""
        cfg = self.cfg
        npart = npart or cfg.parts_per_block
        if raw.numel() < self.block_bytes(npart, first_sample):
            raise DspsrAmdError("dspsr_amd.LoadToFold.process_block: block holds %d bytes, %d needed"
                                % (raw.numel(), self.block_bytes(npart, first_sample)))
        _block_layout(self, first_sample)
        if cfg.zap_rfi and self.rfi_filter is None:
            raise DspsrAmdError("dspsr_amd.LoadToFold.process_block: zap_rfi (-R) is set and no filter has been given: "
                                "call set_rfi_filter before the first block")
        if self.twobit is not None:
            self.twobit.first_sample = first_sample
        nout = self.mode.process(raw, npart, events)              # (the pieces were planned from ndat_out as it was)
        self.ndat_out += nout
        self.nsamples_in += npart * self.nsamp_step

    def _plan_piece(self, piece, pulsar=None):
        """The host plan of Fold::fold (Fold.C:650-657,718-787) for one piece: the phase of its first sample, then the back end's
        bins.  Returns the samples the plan folds (None where the device counts them)."""
        idat_start, ndat_fold = piece[:2]
        t0 = self.out_start + (self.ndat_out + idat_start + 0.5) / self.out_rate     # midpoint of first sample
        phi, pfold = self._phase(t0, pulsar)
        return self.mode.plan_piece(pulsar or self, phi, (1.0 / self.out_rate) / pfold, ndat_fold, idat_start)

    def _book_piece(self, piece, folded, pulsar=None):
        """The books of a folded piece, on the driver or on `pulsar` (hits[] were counted by the plan, Fold.C:744-803); where the
        piece completes its division, the sub-integration"""
        acc = pulsar or self
        if folded is not None:                     # (None: the device counts the hits, the length comes from them)
            acc.integration_length += folded / self.out_rate
        acc.ndat_total += piece[1]
        if piece[3] and pulsar is None:
            self.finish_subint(*self._subint_comm)
        elif piece[3]:
            self._finish_pulsar_subint(pulsar)

    def _fold_pieces(self, pieces, fold, pulsar=None):
        """Subint<Fold>::transformation (Subint.h:234-309): plan, fold (the back end's call over its rows) and book piece by piece,
        emitting a sub-integration at every boundary"""
        for piece in pieces:
            folded = self._plan_piece(piece, pulsar)
            fold()
            self._book_piece(piece, folded, pulsar)

    def _pieces(self, ndat, pulsar=None):
        """Subint<Fold>::transformation (Subint.h:234-309): the pieces of the next `ndat` output samples, one per
        sub-integration they touch -- seconds mode (-L), turns mode (-s / -turns; per pulsar) or one piece."""
        cfg = self.cfg
        if cfg.subint_seconds > 0:
            return subint_pieces(self.ndat_out, ndat, cfg.subint_seconds, self.out_rate)
        if cfg.subint_turns > 0:
            if pulsar is not None:
                if pulsar.turns is None:
                    pulsar.turns = self._turns_divider(*self._ephemeris(pulsar))
                return pulsar.turns.pieces(self.ndat_out, ndat)
            if self._turns is None:
                self._turns = self._turns_divider(*self._ephemeris())
            return self._turns.pieces(self.ndat_out, ndat)
        return [(0, ndat, 0, False)]

    def _turns_divider(self, folding_period, polyco, reference_phase, turns=None):
        """TimeDivide in turns mode for one pulsar's ephemeris (turns: the division length when it is not -s / -turns)"""
        cfg = self.cfg
        if folding_period > 0:
            p = folding_period
            phase = lambda t: (int(math.floor(t / p)), t / p - math.floor(t / p))
            iphase = lambda ph, guess: (ph[0] + ph[1]) * p
            pg = p
        else:
            day, s0 = self.info.mjd_day, self.info.mjd_sec
            phase = lambda t: polyco.phase(day, s0 + t)
            iphase = lambda ph, guess: polyco.iphase(ph, day, s0 + guess) - s0
            pg = 1.0 / polyco.frequency(day, s0 + self.out_start)
        return TurnsDivider(phase, iphase, pg, self.out_start, self.out_rate, cfg.subint_turns if turns is None else turns,
                            reference_phase, cfg.fractional_pulses)

    _subint_comm = (None, 0, 1, None)     # (dist, rank, world, gather_buffer[, replicas]) used at sub-integration dumps

    def set_communicator(self, dist, rank, world, gather_buffer=None, replicas=False):
        self._refuse_exchange("set_communicator")
        self._subint_comm = (dist, rank, world, gather_buffer, replicas)

    def _refuse_exchange(self, what):
        """what a multi-GPU exchange refuses: several pulsars first (asked of a bare instance too), then the back end's own words"""
        if self.pulsars:
            raise DspsrAmdError("dspsr_amd.LoadToFold.%s: the multi-GPU exchange folds one pulsar; this run has %d targets"
                                % (what, len(self.pulsars)))
        if self.mode.no_exchange:
            raise DspsrAmdError("dspsr_amd.LoadToFold.%s: %s not built for a multi-GPU exchange" % (what, self.mode.no_exchange))

    def _finish_pulsar_subint(self, p):
        """Subint<Fold> of one pulsar of a multi-target run: emit its sub-integration and zero its profile."""
        _emit(p, _books(p, profile_dev=self.profiles_tensor(p).clone()), p.fold.zero)

    def profiles_tensor(self, pulsar=None):
        """Zero-copy torch view of the device-resident PhaseSeries (Fold::Engine::get_profiles); `pulsar`: one of a multi-target run."""
        torch = self.torch
        fold, nbin = (self.fold, self.cfg.nbin) if pulsar is None else (pulsar.fold, pulsar.nbin)
        npol, ndim = self._fold_dims()
        n = self.nchan_out * npol * nbin * ndim
        ptr = fold.get_profiles_ptr()

        class _Holder:
            pass
        h = _Holder()
        h.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (int(ptr), False), "version": 2,
                                      "strides": None}
        return torch.as_tensor(h, device=_device(self.ctx))

    comm = None                 # dspsr_amd.Communicator (RCCL behind the C-ABI): the product's exchange
    _comm_pending = None
    copy_subints = True          # False: `subints` profiles stay views of the communicator's pinned buffer (see collect_subint)

    def set_rccl_communicator(self, comm):
        """The exchange of a multi-GPU run: a dspsr_amd.Communicator (dspsr_amd_comm_*, csrc/comm.hip -- the same C entry
        points DSPSR's host calls).  Without one, finish_subint falls back to the torch.distributed calls below, which
        exist for the gloo CPU tests and for rehearsing several ranks on one device (RCCL needs one GPU per rank)."""
        self._refuse_exchange("set_rccl_communicator")
        self.comm = comm

    def collect_subint(self, copy=None):
        """Wait for the exchange finish_subint(wait=False) started and append its result to `subints` (root only).
        copy=False (default: self.copy_subints, True): the entry's profile is a VIEW of the communicator's pinned buffer, valid
        until the next dump starts -- for a writer that consumes each sub-integration as it arrives."""
        if self._comm_pending is None:
            return
        if copy is None:
            copy = self.copy_subints
        check = self._comm_pending
        self._comm_pending = None
        prof, hits, length, ndat_total, same = self.comm.finish(copy=copy)
        if check and not same:
            raise DspsrAmdError("sub-band ranks disagree on hits[]: the shards are not sample aligned "
                                "(different nfilt_pos/neg, start time or rate)")
        if prof is not None:
            self.subints.append({"hits": hits, "integration_length": length, "ndat_total": ndat_total, "profile": prof})

    def finish_subint(self, dist=None, rank=0, world=1, gather_buffer=None, replicas=False, check_hits=True, wait=True):
        """Subint<Fold>: emit the finished sub-integration and zero the profile (Subint.h:291-303).  With world > 1 this
        is the one exchange of the path: sub-band shards deliver their slice of the full band to rank 0, hits /
        integration_length taken from rank 0 (identical everywhere; check_hits asserts it); time-slice replicas
        (replicas=True) SUM profiles, hits, integration_length and ndat_total.
        With an RCCL communicator (set_rccl_communicator) the exchange is dspsr_amd_reduce_profiles_start/finish: a
        snapshot on the compute stream, the collective on the communicator's stream -- the next block's kernels overlap
        it; wait=False leaves it in flight until collect_subint() or the next dump.
        check_hits (default True) adds a MIN/MAX all-reduce of hits[] to the sub-band exchange (two small collectives in the
        same group; nothing for replicas): pass False inside a timed loop that has checked once.
        A multi-target run (one GPU) emits the open sub-integration of every pulsar that has folded samples since its last one."""
        self.mode.finish(dist, rank, world, gather_buffer, replicas, check_hits, wait)

    def _exchange_subint(self, dist, rank, world, gather_buffer, replicas, check_hits, wait):
        """finish_subint of a single pulsar's Detection + Fold: the sub-integration goes through the exchange of the run"""
        if self.comm is not None:
            # (one exchange in flight per communicator.  The result of the previous one is COPIED here even with
            #  copy_subints False: start() below may grow the pinned buffer a view would point into -- a view is only handed
            #  out when the caller collects the sub-integration itself)
            self.collect_subint(copy=True)
            n = self.npol_out * self.cfg.nbin * self.cfg.ndim           # floats per channel: rows are packed
            self.comm.start(self.comm.SUM if replicas else self.comm.GATHER, self.fold.get_profiles_ptr(), n, self.nchan_out, n,
                            self.hits, self.integration_length, self.ndat_total, root=0,
                            check_hits=check_hits and not replicas)
            self._comm_pending = bool(check_hits and not replicas)
            _emit(self, None, self.fold.zero)                           # (the zero is stream ordered behind the snapshot)
            if wait:
                self.collect_subint()
            return
        prof, entry = self.profiles_tensor(), None
        if replicas:
            res = reduce_replicas(prof, self.hits, self.integration_length, self.ndat_total, dist, rank, world)
            if rank == 0:
                entry = {"hits": res[1].copy(), "integration_length": res[2], "ndat_total": res[3], "profile_dev": res[0].clone()}
        else:
            if check_hits:
                check_identical_hits(self.hits, dist, rank, world)
            result = reduce_subbands(prof, dist, rank, world, gather_buffer)
            if rank == 0:
                entry = _books(self, profile_dev=result.clone())
        _emit(self, entry, self.fold.zero)

    def process_host_blocks(self, blocks, npart=None):
        """Host hand-over (the role of dsp::TransferCUDA / TransferBitSeriesCUDA, Signal/General/TransferCUDA.C:24-85):
        `blocks` yields one block each -- a pinned host int8 tensor (copied from where it lies; the caller must not touch
        it again before the call returns), or any other host int8 tensor / numpy array (staged through two pinned buffers
        owned by this call), optionally as a pair (block, npart) for a ragged last block or, for a file of heaps, a triple
        (block, npart, first_sample).  Block i+1 is copied to the
        device on a second stream while block i is processed (two device buffers, events both ways).  With the data
        coming over PCIe Gen5 x16 the link, not the GPU, sets the rate.  Returns the number of
        blocks processed."""
        torch = self.torch
        main = torch.cuda.current_stream()
        copy = torch.cuda.Stream()
        bufs, pins = [None, None], [None, None]
        ready, done = [torch.cuda.Event(), torch.cuda.Event()], [torch.cuda.Event(), torch.cuda.Event()]
        used = [False, False]
        it = iter(blocks)

        def split(item):
            if item is None:
                return None, None
            if isinstance(item, tuple):
                return item[0], item[1:]                     # (npart,) or, for heaps and GUPPI raw blocks, (npart, first_sample)
            return item, (npart,)

        def upload(k, host):
            if not (torch.is_tensor(host) and host.is_pinned()):
                src = (host.numpy() if torch.is_tensor(host) else np.asarray(host)).reshape(-1).view(np.int8)
                if used[k]:
                    ready[k].synchronize()                   # host wait: the previous copy out of this pinned buffer is over
                if pins[k] is None or pins[k].numel() < src.size:
                    pins[k] = torch.empty(src.size, dtype=torch.int8).pin_memory()
                host = pins[k][:src.size]
                host.numpy()[:] = src                        # (a read-only memory map is fine as a source)
            with torch.cuda.stream(copy):
                if bufs[k] is None or bufs[k].numel() < host.numel():
                    if bufs[k] is not None:
                        bufs[k].record_stream(main)          # still being read by kernels on the main stream
                    bufs[k] = _device_empty(self.ctx, host.numel(), "int8")
                    bufs[k].record_stream(main)
                elif used[k]:
                    copy.wait_event(done[k])                 # the kernels that read this buffer have finished
                bufs[k][:host.numel()].copy_(host, non_blocking=True)
                ready[k].record(copy)
            used[k] = True
            return host.numel()
        nxt, nxt_parts = split(next(it, None))
        if nxt is None:
            return 0
        sizes = [upload(0, nxt), 0]
        parts = [nxt_parts, None]
        n = 0
        while True:
            k = n & 1
            nxt, nxt_parts = split(next(it, None))
            if nxt is not None:
                sizes[k ^ 1], parts[k ^ 1] = upload(k ^ 1, nxt), nxt_parts
            main.wait_event(ready[k])
            self.process_block(bufs[k][:sizes[k]], parts[k][0], None, *parts[k][1:])
            done[k].record(main)
            n += 1
            if nxt is None:
                break
        main.synchronize()                                   # the staging buffers go out of scope with this call
        return n

    def synchronize(self):
        self.ctx.synchronize()

    def close(self):
        """Release everything opened, the context last; also on an instance whose construction stopped half-way, and once only."""
        if self._closed:
            return
        self._closed = True
        if self._comm_pending is not None:
            self.collect_subint()
        _close_all(*self.dumps.values(), self.sample_delay, self.fb, *(getattr(self, e) for e in self.mode.engines), *(p.fold for p in self.pulsars), self.ctx)


# ---- search mode: digifil (Signal/General/LoadToFil.C) ------------------------------------------------------------

@dataclass
class SearchConfig:
    """The digifil options on this path (LoadToFil.C:60-100 defaults, digifil.C)."""
    nchan: int = 4096                 # -F nchan  (non-convolving TFPFilterbank)
    tscrunch: int = 16                # -t
    nbit: int = 2                     # -b  (digifil default 2; 1, 2, 4, 8, 16, -32)
    rescale_seconds: float = 10.0     # -I  (0 disables Rescale and the digitizer's own scales, LoadToFil.C:318,360)
    rescale_constant: bool = False    # -c
    scale_fac: float = 1.0            # -s
    parts_per_block: int = 4096       # FFT blocks (2*nchan samples each) per call; a multiple of tscrunch
    # the convolving branch, `-F nchan:D` (LoadToFil.C:176-222): LoadToFilCoherent
    dispersion_measure: float = 0.0   # -D  (with -F N:D: coherent dedispersion inside the filterbank)
    freq_res: int = 0                 # -x  (0 => optimal, as dsp::Dedispersion chooses)
    fscrunch: int = 0                 # -f
    npol: int = 1                     # -d  output polarisations: 1 Intensity, 2 PPQQ, 4 Coherence (LoadToFil.C:262-277)
    dedisperse: bool = False          # -K  remove the inter-channel dispersion delays (dsp::SampleDelay, LoadToFil.C:236-247)
    max_parts: int = 32               # parts per launch group
    fused: bool = True                # detection + time scrunch inside the inverse pass where the geometry allows it
    fuse_coherence: bool = False      # ... also for the four Coherence products (npol 4): one perform_search per block in place of
                                      #     perform_detect + TScrunch, the same bytes (not a reference option; off by default)


def write_sigproc_header(f, *, source_name="unknown", rawdatafile="unknown", machine_id=0, telescope_id=0, src_raj=0.0, src_dej=0.0,
                         fch1, foff, nchans, nbits, tstart_mjd, tsamp, nifs=1):
    """The SIGPROC filterbank header digifil writes (Kernel/Formats/sigproc/filterbank_header.c:42-105, send_stuff.c,
    values as SigProcObservation::unload fills them, SigProcObservation.C:228-270): length-prefixed keywords, native
    (little-endian) int32 / float64 values."""
    import struct

    def send_string(sv):
        b = sv.encode("ascii")
        f.write(struct.pack("<i", len(b)) + b)

    def send_int(name, v):
        send_string(name)
        f.write(struct.pack("<i", int(v)))

    def send_double(name, v):
        send_string(name)
        f.write(struct.pack("<d", float(v)))

    send_string("HEADER_START")
    if rawdatafile:
        send_string("rawdatafile")
        send_string(rawdatafile)
    if source_name:
        send_string("source_name")
        send_string(source_name)
    send_int("machine_id", machine_id)
    send_int("telescope_id", telescope_id)
    for name, v in (("src_raj", src_raj), ("src_dej", src_dej), ("az_start", 0.0), ("za_start", 0.0)):   # send_coords
        send_double(name, v)
    send_int("data_type", 1)
    send_double("fch1", fch1)
    send_double("foff", foff)
    send_int("nchans", nchans)
    send_int("nbeams", 0)
    send_int("ibeam", 0)
    send_int("nbits", nbits)
    send_double("tstart", tstart_mjd)
    send_double("tsamp", tsamp)
    send_int("nifs", nifs)
    send_string("HEADER_END")


def sigproc_header_values(info, nbit, nchan, tsamp, start_seconds, nifs):
    """fch1/foff/tsamp/tstart as SigProcObservation::unload derives them from the digitizer's output observation
    (bandwidth forced negative, SigProcDigitizer.C:83-85; channel 0 centred half a channel inside the band edge)."""
    bw = -abs(info.bandwidth)
    fch1 = info.centre_frequency - 0.5 * bw + 0.5 * bw / nchan
    return dict(fch1=fch1, foff=bw / nchan, nchans=nchan, nbits=_nbits(nbit), tsamp=tsamp,
                tstart_mjd=info.mjd_day + (info.mjd_sec + start_seconds) / 86400.0, nifs=nifs)


def _nbits(nbit):
    """bits per output sample of -b (-32: floats)"""
    return 32 if nbit == -32 else nbit


def _rescale_interval(cfg, out_rate):
    """Rescale::init (Rescale.C:102-103): samples per interval of -I, 0 without Rescale"""
    if not cfg.rescale_seconds:
        return 0
    interval = int(cfg.rescale_seconds * out_rate)
    if not interval:
        raise DspsrAmdError("dsp::Rescale::init nsample == 0")
    return interval


def _of(part, name):
    """A driver's view of a value that lives on one of its parts"""
    return property(lambda self: getattr(getattr(self, part), name))


# ---- the parts of the search drivers: one front end per input, one output stage per format ---------------------------------------
# A front end turns a call's 8-bit block into scrunched rows [nchan_out][npol][nout]: it plans on the host when it is made (every
# refusal, no device), opens on the context its owner gives it, and writes its rows into a buffer of its own or, where the owner
# hands a destination in, there.  An output stage turns those rows into what a format takes.  A driver is one of each on one shell.

FRONT_OPTIONS = ("nchan", "tscrunch", "fscrunch", "npol", "dedisperse", "dispersion_measure", "freq_res", "parts_per_block", "max_parts", "fused",
                 "fuse_coherence")


class SearchFront:
    """What the two front ends share: the plan behind their geometry (state, scrunch factors, the -K delays and their head room,
    whether the one-pass form applies), the buffers, and the chain behind detection: [SampleDelay, in place (LoadToFil.C:240-241)]
    -> [FScrunch] -> TScrunch.  `cfg` holds the options that concern a front end (FRONT_OPTIONS) and no others."""

    ctx = fb = sample_delay = scrunched = detected = fscr = None
    tsamp = property(lambda self: 1.0 / self.out_rate)

    def __init__(self, info, **options):
        from types import SimpleNamespace
        self.info, self.cfg = info, SimpleNamespace(**options)
        cfg = self.cfg
        # the subclass: its refusals; the channels, rate, start and scale of the detected rows; the samples of a full call, where
        # the host knows them
        self.nchan, self.rate, self.out_start, scale, self.block = self._geometry()
        if cfg.fscrunch and self.nchan % cfg.fscrunch:
            raise DspsrAmdError("%s: nchan=%d is not a multiple of fscrunch=%d" % (self.who, self.nchan, cfg.fscrunch))
        self.ts = ts = max(1, cfg.tscrunch)
        self.nchan_out = self.nchan // cfg.fscrunch if cfg.fscrunch else self.nchan
        self.out_rate = self.rate / ts
        # FScrunch / TScrunch multiply the scale by their factors (TimeSeries::rescale, TScrunch.C:126, FScrunch.C:103); without
        # Rescale the digitiser divides by it (SigProcDigitizer.C:158)
        self.input_scale = scale * ts * (cfg.fscrunch or 1)
        self.state = {1: _lib.INTENSITY, 2: _lib.PPQQ, 4: _lib.COHERENCE}[cfg.npol]
        self.scale8 = eight_bit_scale()
        # -K: dsp::SampleDelay sits in front of Detection (LoadToFil.C:236-247).  Detection acts sample by sample, so delaying the
        # detected rows gives the reference's numbers; the last total_delay samples of a block are re-presented in front of the
        # next one (InputBuffering, SampleDelay.C:117,146): they live in the head room in front of `detected`.
        self.sd = DelayCarry()
        if cfg.dedisperse:
            self.sd = DelayCarry(self.channel_delays(cfg.dispersion_measure, self.nchan, self.rate))
            if self.block is not None:
                self.sd.check_block(self.name, self.block)
            self.out_start += self.sd.zero / self.rate                                   # SampleDelay.C:159
        # FScrunch sits between Detection and TScrunch and SampleDelay in front of Detection: the one-pass form holds neither, so
        # with -f or -K detection runs at tscrunch 1 into `detected` and the operations follow one after the other
        self.fused = self._one_pass() and not cfg.fscrunch and not cfg.dedisperse
        self.carry_count = 0

    def open(self, ctx, own_rows=True):
        """The engine and the buffers on `ctx`.  own_rows False: every call brings the destination of its scrunched rows."""
        cfg, shape = self.cfg, (self.nchan_out, self.cfg.npol)
        self.ctx = ctx
        self._open_engine()
        if cfg.dedisperse:
            self.sample_delay = SampleDelay(ctx, self.sd.delays, cfg.npol)
            self.sd.check_block(self.name, self.block)       # (-F: the block is known with the engine's nkeep)
        nd = self.sd.head + self.block
        self.nmax = max(1, (self.ts - 1 + nd) // self.ts)    # the most scrunched samples one call delivers
        if own_rows:
            self.scrunched = _device_empty(ctx, shape + (self.nmax,))
        self.carry = _device_empty(ctx, shape, zero=True)
        if not self.fused:
            self.detected = _device_empty(ctx, (self.nchan, cfg.npol, nd))
            if cfg.fscrunch:
                self.fscr = _device_empty(ctx, shape + (nd,))

    def detect_scrunch(self, raw, n=None, first_sample=0, out=None):
        """Detection -> [SampleDelay] -> [FScrunch] -> TScrunch of one call of `n` parts (-F) or time samples (no -F): the scrunched
        rows [nchan_out][npol][nout], a view of `out` (default: the front end's own buffer).  first_sample: a block of MeerKAT heaps
        begins at that sample of its first heap (LoadToFold.process_block)."""
        n = self._count(n)
        need = self.block_bytes(n, first_sample)
        if raw.numel() < need:
            raise DspsrAmdError("%s.process_block: block holds %d bytes, %d needed" % (self.who, raw.numel(), need))
        out = self.scrunched if out is None else out
        if self.fused:
            nout, self.carry_count = self._detect(raw, n, first_sample, out, self.ts)
            return out[:, :, :nout]
        nd, head = n * self.samples_per_count, self.sd.head
        det = self.detected[:, :, head:head + nd]
        self._detect(raw, n, first_sample, det, 1)
        if self.sample_delay is None:
            return out[:, :, :self._scrunch(det, out)]
        return out[:, :, :self.sd.delayed(self.ctx, self.sample_delay, self.detected, nd, lambda rows: self._scrunch(rows, out))]

    def _scrunch(self, det, out):
        """[FScrunch] -> TScrunch of the detected rows into `out`: how many samples that completes"""
        nd, nout = det.shape[2], 0
        if nd:
            if self.cfg.fscrunch:
                det = fscrunch_fpt(self.ctx, det, self.fscr[:, :, :nd], self.cfg.fscrunch)
            nout, self.carry_count = tscrunch_fpt(self.ctx, det, out, self.ts, self.carry, self.carry_count)
        return nout

    def close(self):
        _close_all(self.sample_delay, self.fb)


class ConvolvingFront(SearchFront):
    """`-F N[:D] [-x M]`, MeerKAT heaps included (LoadToFil.C:176-222,250-304): dsp::Filterbank with the Dedispersion response ->
    Detection::square_law -> [FScrunch] -> TScrunch.  One launch group runs filterbank, detection and time scrunch
    (FilterbankEngine.perform_search): the detected rows never exist at the filterbank's output rate.  A call takes the 8-bit block
    of LoadToFold: n * nsamp_step + nsamp_overlap samples, the overlap re-presented by the caller; no n (or 0): parts_per_block."""

    name, who = "LoadToFilCoherent", "dspsr_amd.LoadToFilCoherent"           # (the driver its refusals have always named)
    samples_per_count = property(lambda self: self.nkeep)

    def _geometry(self):
        cfg, info, who = self.cfg, self.info, self.who
        self.form = refuse_forms(who, info, VOLTAGES)
        if cfg.npol not in (1, 2, 4):
            raise DspsrAmdError("%s: npol=%d (Intensity 1 / PPQQ 2 / Coherence 4 are built; NthPower 3 is not)" % (who, cfg.npol))
        if cfg.npol >= 2 and info.npol != 2:
            raise DspsrAmdError("%s: PPQQ / Coherence need two input polarisations" % who)
        if cfg.nchan % info.nchan:
            raise DspsrAmdError("dsp::Filterbank::make_preparations output nchan=%d not a multiple of input nchan=%d" % (cfg.nchan, info.nchan))
        if cfg.dispersion_measure == 0.0 and not cfg.freq_res and cfg.npol <= 2:
            raise DspsrAmdError("%s: -F N:D with a dispersion measure, -F N -x M, or -d 4 (with none of them "
                                "digifil takes the TFPFilterbank: dspsr_amd.LoadToFil)" % who)
        if cfg.dispersion_measure != 0.0:
            r = matched_response(info, cfg.dispersion_measure, cfg.freq_res, cfg.nchan, input_nchan=info.nchan, ndim=info.ndim)   # LoadToFil.C:190-191
        else:
            # -F N -x M without :D (LoadToFil.C:199-216): the convolving filterbank with no response -- nothing is discarded
            # (Filterbank.C:139-155: freq_res as set, nfilt 0)
            # -F N -d 4 with neither (LoadToFil.C:205-207: `npol > 2` takes the Filterbank too): its default freq_res = 1, the
            # non-convolving filterbank (Filterbank.C:614-623)
            from types import SimpleNamespace
            r = SimpleNamespace(ndat=cfg.freq_res or 1, impulse_pos=0, impulse_neg=0, kernel=None)
        self.response = r
        # Filterbank.C:124-128 leaves scale = n_fft * freq_res on its output
        self.fb_rate, start, scale = filterbank_output(info, r, cfg.nchan // info.nchan)
        return cfg.nchan, self.fb_rate, start, scale, None

    def _one_pass(self):
        """the fused launch group holds the two square-law states; the four Coherence products only where the caller asks for it
        (fuse_coherence: perform_search with COHERENCE -- the engine fuses where the staged tile fits and runs the operations one after
        the other elsewhere, the same numbers), else perform_detect with ndim 1"""
        return self.cfg.fused and (self.cfg.npol != 4 or self.cfg.fuse_coherence)

    def channel_delays(self, dispersion_measure, nchan, rate):
        """the -K delays of `nchan` channels of this filterbank's output at `rate` (Observation.C:80-87; Filterbank.C:358-364)"""
        info, dual = self.info, self.info.ndim == 2
        return dedispersion_sample_delays(info.centre_frequency, info.bandwidth, dispersion_measure, nchan, rate,
                                          swap=dual and info.nchan == 1, nsub_swap=info.nchan if dual and info.nchan > 1 else 0)

    def _open_engine(self):
        cfg, info, r = self.cfg, self.info, self.response
        _open_convolving_front(self, r, cfg.nchan // info.nchan, info.nchan, r.kernel, max_parts=cfg.max_parts)
        self.block = cfg.parts_per_block * self.nkeep
        if not self.fused and cfg.npol != 4:
            self.det_carry = _device_empty(self.ctx, (cfg.nchan, cfg.npol), zero=True)

    def _count(self, npart):
        return npart or self.cfg.parts_per_block

    def block_bytes(self, npart=None, first_sample=0):
        nsamp = (npart or self.cfg.parts_per_block) * self.nsamp_step + self.nsamp_overlap
        return self.form.block_bytes(nsamp, self.info.nchan, self.info.npol, self.info.ndim, first_sample)

    def _detect(self, raw, npart, first_sample, out, ts):
        _block_layout(self, first_sample)
        block = dict(raw=raw, layout=self.layout, scale=self.scale8)
        if self.fused:
            return self.fb.perform_search(out, self.carry, self.carry_count, npart, ts, self.state, **block)
        if self.cfg.npol == 4:
            return self.fb.perform_detect(out, npart, self.state, 1, **block)
        return self.fb.perform_search(out, self.det_carry, 0, npart, 1, self.state, **block)

    def file_calls(self, f):
        """DadaFile `f` cut into this front end's calls: parts with their overlap (DadaFile.blocks)"""
        return f.blocks(self)


class ChannelisedFront(SearchFront):
    """No -F, on an already channelised complex 8-bit file (LoadToFil.C:233-304): Detection (Intensity / PPQQ / Coherence with
    ndim 1) -> [FScrunch] -> [TScrunch].  The block is detected and time-scrunched in ONE pass (dspsr_amd.detect_raw): the float
    voltages are never written.  The channels are those of the file: nchan, freq_res, max_parts, fused and fuse_coherence are IGNORED;
    parts_per_block is the largest number of time samples one call may bring.  A call takes n time samples in DADA order
    [n][nchan][npol][2] int8: any n up to parts_per_block, 0 included; no n: parts_per_block."""

    name, who = "LoadToFilDirect", "dspsr_amd.LoadToFilDirect"
    samples_per_count = 1
    tsamp = property(lambda self: self.ts / self.info.rate)                    # (not always the double that 1 / out_rate is)

    def _geometry(self):
        cfg, info, who = self.cfg, self.info, self.who
        refuse_forms(who, info, VOLTAGES)                # (the voltages it does not read are refused behind NDIM and NBIT, as they always were)
        if info.ndim != 2:
            raise DspsrAmdError("%s: NDIM=%d; complex (NDIM 2) channelised voltages only" % (who, info.ndim))
        if info.nbit != 8:
            raise DspsrAmdError("%s: NBIT=%d; this path reads 8-bit samples" % (who, info.nbit))
        self.form = refuse_forms(who, info, {"generic"}, {
            "heaps": "dspsr_amd.unpack_heaps_fpt gives the float rows, and -F N:D (dspsr_amd.LoadToFilCoherent) reads the heaps",
            "guppi": "dspsr_amd.unpack_guppi_fpt gives the float rows, and -F N:D (dspsr_amd.LoadToFilCoherent) reads the blocks"})
        if cfg.npol not in (1, 2, 4):
            raise DspsrAmdError("%s: npol=%d (Intensity 1 / PPQQ 2 / Coherence 4 are built; NthPower 3 is not)" % (who, cfg.npol))
        if info.npol not in (1, 2):
            raise DspsrAmdError("%s: NPOL=%d; one or two input polarisations" % (who, info.npol))
        if cfg.npol >= 2 and info.npol != 2:
            raise DspsrAmdError("dsp::Detection::checks invalid npol=%d for %s formation" % (info.npol, "PPQQ" if cfg.npol == 2 else "Coherence"))
        if info.nchan < 1 or cfg.parts_per_block < 1:
            raise DspsrAmdError("%s: nchan=%d, parts_per_block=%d" % (who, info.nchan, cfg.parts_per_block))
        return info.nchan, info.rate, info.start_seconds, 1.0, cfg.parts_per_block       # (no filterbank factor in the scale)

    def _one_pass(self):
        return True

    def channel_delays(self, dispersion_measure, nchan, rate):
        """the -K delays: the input comes from a file, not from a filterbank -- no swapped halves (Observation.C:420-451)"""
        return dedispersion_sample_delays(self.info.centre_frequency, self.info.bandwidth, dispersion_measure, nchan, rate, swap=False, nsub_swap=0)

    def _open_engine(self):
        pass

    def _count(self, ndat):
        ndat = self.cfg.parts_per_block if ndat is None else ndat
        if ndat > self.cfg.parts_per_block:
            raise DspsrAmdError("%s.process_block: ndat=%d exceeds parts_per_block=%d" % (self.who, ndat, self.cfg.parts_per_block))
        return ndat

    def block_bytes(self, ndat=None, first_sample=0):
        ndat = self.cfg.parts_per_block if ndat is None else ndat
        return self.form.block_bytes(ndat, self.info.nchan, self.info.npol, 2, first_sample)

    def _detect(self, raw, ndat, first_sample, out, ts):
        carry, count = (self.carry, self.carry_count) if self.fused else (None, None)
        return detect_raw(self.ctx, raw, out, carry, count, self.info.nchan, self.info.npol, ts, self.state, self.scale8, ndat=ndat)

    def file_calls(self, f):
        """DadaFile `f` cut into this front end's calls: runs of parts_per_block time samples, the last one shorter"""
        step = self.cfg.parts_per_block
        for s0 in range(0, f.ndat, step):
            ndat = min(step, f.ndat - s0)
            yield f.samples(s0, ndat), ndat


class SigprocOutput:
    """[Rescale] -> SigProcDigitizer of scrunched FPT rows (LoadToFil.C:306-362) and the SIGPROC header that goes with the bytes"""

    ctx = rescale = None

    def __init__(self, cfg, info, nchan, out_rate):
        self.cfg, self.info, self.nchan = cfg, info, nchan
        self.rescale_interval = _rescale_interval(cfg, out_rate)
        self.bytes_per_sample = nchan * cfg.npol * _nbits(cfg.nbit) // 8
        self.ndat_out = 0

    def open(self, ctx, nmax):
        """for calls of at most `nmax` samples"""
        cfg = self.cfg
        self.ctx = ctx
        if self.rescale_interval:
            self.rescale = Rescale(ctx, self.nchan, cfg.npol, self.rescale_interval, cfg.rescale_constant)
        self.packed = _device_empty(ctx, nmax * self.bytes_per_sample, "uint8")

    def digitize(self, scr, input_scale):
        """the packed bytes [time][pol][chan] of the rows `scr` [nchan][npol][nout], which carry the scale `input_scale`"""
        cfg, nout = self.cfg, scr.shape[2]
        packed = self.packed[:nout * self.bytes_per_sample]
        flip = self.info.bandwidth > 0
        if nout:
            if self.rescale is not None and cfg.nbit != -32:
                self.rescale.digitize_fpt(scr, packed, cfg.nbit, cfg.scale_fac, flip_band=flip)        # Rescale + digitiser, one pass
            else:
                if self.rescale is not None:
                    self.rescale.transform_fpt(scr)                                                     # in place, LoadToFil.C:312-313
                sigproc_digitize_fpt(self.ctx, scr, packed, cfg.nbit, use_digi_scales=self.rescale is not None,
                                     input_scale=1.0 if self.rescale is not None else input_scale, scale_fac=cfg.scale_fac,
                                     flip_band=flip)
        self.ndat_out += nout
        return packed

    def header_values(self, tsamp, start_seconds):
        return sigproc_header_values(self.info, self.cfg.nbit, self.nchan, tsamp, start_seconds, self.cfg.npol)

    def close(self):
        _close_all(self.rescale)


class _SearchDriver:
    """The shell of the search drivers: the host plan first (every refusal comes from there, before a device is touched), then the
    device under try/close; close() releases the parts and then the context, once, also after a construction that stopped half-way.
    device None: the host plan alone."""

    ctx = None
    _closed = False

    def __init__(self, cfg, info, device: int | None = 0, stream: int | None = None):
        self.cfg, self.info = cfg, info
        self._plan()
        if device is None:
            return
        try:
            self.ctx = Context(device, stream)
            self._open()
        except BaseException:
            self.close()
            raise

    def synchronize(self):
        self.ctx.synchronize()

    def close(self):
        if not self._closed:
            self._closed = True
            _close_all(*self._parts(), self.ctx)


class LoadToFil(_SearchDriver):
    """digifil's chain for 8-bit real dual-polarisation input and one output polarisation, every stage on the device
    (LoadToFil.C:196-362): TFPFilterbank (PPQQ) + TScrunch [one kernel] -> Rescale (per pol and channel, in place)
    -> PScrunch -> SigProcDigitizer.  process_block returns the packed block (device uint8, [time][chan] n-bit)."""

    fused_output = True          # Rescale + PScrunch + digitiser as one pass (False: the three operations one after the other)
    rescale = None

    def _plan(self):
        cfg, info = self.cfg, self.info
        form = refuse_forms("dspsr_amd.LoadToFil", info, {"generic", "caspsr"}, "channelised complex voltages take -F N:D (dspsr_amd.LoadToFilCoherent)")
        if info.npol != 2 or info.ndim != 1 or info.nchan != 1:
            raise DspsrAmdError("dspsr_amd.LoadToFil: 8-bit real dual-polarisation single-channel input only")
        if cfg.parts_per_block % cfg.tscrunch:
            raise DspsrAmdError("dspsr_amd.LoadToFil: parts_per_block=%d is not a multiple of tscrunch=%d"
                                % (cfg.parts_per_block, cfg.tscrunch))
        self.scale8 = eight_bit_scale()
        self.layout = form.layout
        self.out_rate = info.rate / (2.0 * cfg.nchan) / cfg.tscrunch           # TFPFilterbank + TScrunch
        self.bytes_per_sample = cfg.nchan * _nbits(cfg.nbit) // 8
        self.ndat_out = 0
        self.rescale_interval = _rescale_interval(cfg, self.out_rate)

    def _open(self):
        cfg, nout = self.cfg, self.cfg.parts_per_block // self.cfg.tscrunch
        self.detected = _device_empty(self.ctx, (nout, cfg.nchan, 2))      # PPQQ, TFP order
        self.intensity = _device_empty(self.ctx, (nout, cfg.nchan, 1))
        if self.rescale_interval:
            self.rescale = Rescale(self.ctx, cfg.nchan, 2, self.rescale_interval, cfg.rescale_constant)
        self.packed = _device_empty(self.ctx, nout * self.bytes_per_sample, "uint8")

    def _parts(self):
        return (self.rescale,)

    def block_bytes(self, npart=None):
        return (npart or self.cfg.parts_per_block) * 2 * self.cfg.nchan * 2

    def process_block(self, raw, npart=None):
        cfg = self.cfg
        npart = npart or cfg.parts_per_block
        if npart % cfg.tscrunch or npart > cfg.parts_per_block:
            raise DspsrAmdError("dspsr_amd.LoadToFil.process_block: npart=%d must be a multiple of tscrunch=%d and <= %d"
                                % (npart, cfg.tscrunch, cfg.parts_per_block))
        if raw.numel() < self.block_bytes(npart):
            raise DspsrAmdError("dspsr_amd.LoadToFil.process_block: block holds %d bytes, %d needed"
                                % (raw.numel(), self.block_bytes(npart)))
        nout = npart // cfg.tscrunch
        det = self.detected[:nout]
        tfp_filterbank(self.ctx, raw, cfg.nchan, npart, det, False, cfg.tscrunch, self.layout, self.scale8)
        packed = self.packed[:nout * self.bytes_per_sample]
        if self.rescale is not None and self.fused_output and cfg.nbit in (1, 2, 4, 8, 16):
            # Rescale -> PScrunch -> digitiser in one pass over the PPQQ block (identical bytes, LoadToFil.C:318-362)
            self.rescale.pscrunch_digitize(det, packed, cfg.nbit, cfg.scale_fac, flip_band=self.info.bandwidth > 0, swap_band=False)
            self.ndat_out += nout
            return packed
        if self.rescale is not None:
            self.rescale.transform(det)                                            # in place, LoadToFil.C:325-326
        inten = self.intensity[:nout]
        pscrunch_tfp(self.ctx, det, inten, cfg.nchan, 2)                            # LoadToFil.C:333-343
        # after Rescale the input scale is 1 (Rescale.C:204); without it the TFP filterbank leaves scale 1 as well
        sigproc_digitize(self.ctx, inten, packed, cfg.nchan, 1, cfg.nbit, use_digi_scales=self.rescale is not None,
                         input_scale=1.0, scale_fac=cfg.scale_fac, flip_band=self.info.bandwidth > 0, swap_band=False)
        self.ndat_out += nout
        return packed

    def header_values(self):
        return sigproc_header_values(self.info, self.cfg.nbit, self.cfg.nchan, 1.0 / self.out_rate, self.info.start_seconds, 1)


class _FrontToFil(_SearchDriver):
    """digifil in FPT order, every stage on the device: a front end (`front_end`) and the SIGPROC output stage.  process_block takes
    what the front end's detect_scrunch takes and returns the packed bytes [time][pol][chan] of the output samples it completes."""

    front = out = None

    def _plan(self):
        cfg = self.cfg
        self.front = self.front_end(self.info, **{k: getattr(cfg, k) for k in FRONT_OPTIONS})
        self.out = SigprocOutput(cfg, self.info, self.front.nchan_out, self.front.out_rate)

    def _open(self):
        self.front.open(self.ctx)
        self.out.open(self.ctx, self.front.nmax)

    def _parts(self):
        return self.out, self.front

    def process_block(self, raw, n=None, first_sample=0):
        return self.out.digitize(self.front.detect_scrunch(raw, n, first_sample), self.front.input_scale)

    def header_values(self):
        return self.out.header_values(self.front.tsamp, self.front.out_start)


for _name in ("response", "fb", "nkeep", "nsamp_step", "nsamp_overlap", "form", "layout", "scale8", "fb_rate", "fused", "ts", "nchan_out", "out_rate",
              "out_start", "input_scale", "sd", "sample_delay", "carry_count", "block_bytes", "detect_scrunch", "file_calls"):
    setattr(_FrontToFil, _name, _of("front", _name))
for _name in ("bytes_per_sample", "ndat_out", "rescale", "rescale_interval"):
    setattr(_FrontToFil, _name, _of("out", _name))
_FrontToFil.sd_head, _FrontToFil.sd_carried = _carry_view("head"), _carry_view("carried")


class LoadToFilCoherent(_FrontToFil):
    """digifil with the convolving filterbank, `digifil -F N:D [-x M] [-f F] [-K] -t T -b nbit` (Signal/General/LoadToFil.C:176-222,
    250-362): ConvolvingFront -> [Rescale] -> SigProcDigitizer.  process_block(raw, npart, first_sample)."""
    front_end = ConvolvingFront


class LoadToFilDirect(_FrontToFil):
    """digifil on an already channelised voltage file with NO -F, `digifil file.dada [-K] [-d npol] [-f F] [-t T] [-I s] -b nbit`
    (Signal/General/LoadToFil.C:233-362): ChannelisedFront -> [Rescale] -> SigProcDigitizer.  process_block(raw, ndat)."""
    front_end = ChannelisedFront


# ---- search mode: digifits (Signal/General/digifits.C, LoadToFITS.C) -----------------------------------------------------------------

@dataclass
class FitsConfig:
    """The digifits options (digifits.C) with LoadToFITS::Config's defaults (LoadToFITS.C:65-100)."""
    nchan: int = 0                    # -F nchan  (0: the channels of the file)
    convolve: bool = False            # -F nchan:D  (Filterbank::Config::During)
    freq_res: int = 0                 # -x  (with the response: times the minimum transform length, LoadToFITS.C:272)
    dispersion_measure: float = 0.0   # -D
    coherent_dedisp: bool = False     # -do_dedisp
    tsamp: float = 64e-6              # -t  seconds
    npol: int = 4                     # -p  1 Intensity, 2 PPQQ, 4 Coherence
    nbit: int = 2                     # -b  1, 2, 4, 8
    nsblk: int = 2048                 # -nsblk  samples per output block
    rescale_seconds: float = -1.0     # -I  (<= 0: the spectrum of each block alone)
    rescale_constant: bool = False    # -c
    dedisperse: bool = False          # -K  remove the inter-channel dispersion delays, behind TScrunch (LoadToFITS.C:486-498)
    integration_length: float = 0.0   # -L  (file splitting: refused)
    parts_per_block: int = 64         # -F: parts (FFT blocks) per call; no -F: the most time samples per call
    max_parts: int = 32               # parts per launch group
    fused: bool = True                # detection + time scrunch inside the inverse pass where the geometry allows it
    fuse_coherence: bool = False      # ... also for the four Coherence products (npol 4): one perform_search per block in place of
                                      #     perform_detect + TScrunch, the same bytes (not a reference option; off by default)


def _c_round(x):
    """round() of <cmath> for the non-negative values of LoadToFITS.C:192,201: halves go away from zero"""
    return int(math.floor(x + 0.5))


def fits_plan(cfg: FitsConfig, info: InputInfo):
    """LoadToFITS.C:178-204 and :539-551 restated: (tres_factor, tsamp the reference prints, nblock).  With multi-channel input and -F
    the factor counts the file's per-channel rate against ALL output channels, as the reference does: the time resolution of the
    output is what the chain delivers (LoadToFITS.out_rate -> TBIN), not this tsamp."""
    rate = info.rate
    factor = 0.5 if info.ndim == 1 else 1.0                  # Signal::Nyquist
    if cfg.nchan > 0:
        samp_per_fb = cfg.tsamp * rate
        tres_factor = _c_round(factor * samp_per_fb / cfg.nchan)
        tsamp = tres_factor / factor * cfg.nchan / rate
    else:
        tres_factor = _c_round(rate * cfg.tsamp)
        tsamp = tres_factor / factor * 1 / rate
    nblock = 1
    if not cfg.rescale_constant and cfg.rescale_seconds > 0:
        tblock = cfg.tsamp * cfg.nsblk
        nblock = max(1, int(cfg.rescale_seconds / tblock + 0.5))
    return tres_factor, tsamp, nblock


SEARCH_BLOCKS_MAGIC = "DSPSR_AMD_SEARCH_BLOCKS"
SEARCH_BLOCKS_HDR_SIZE = 4096
POL_TYPES = {1: "AA+BB", 2: "AABB", 4: "AABBCRCI"}           # PSRFITS POL_TYPE of Intensity, PPQQ, Coherence


class FitsOutput:
    """The PSRFITS output stage (LoadToFITS.C:486-553): [SampleDelay at the scrunched rate, -K] -> the rows collect until nsblk of
    them are there -> FITSDigitizer, block by block.  The front end writes a call's rows where destination() says: straight behind
    the rows that wait for a block, or with -K behind the head room that holds the tail SampleDelay gave up."""

    ctx = digitizer = sample_delay = kbuf = None

    def __init__(self, cfg, info, front, nblock):
        who = "dspsr_amd.LoadToFITS"
        self.cfg, self.info, self.nblock = cfg, info, nblock
        self.nchan, self.out_start = front.nchan_out, front.out_start
        if self.nchan % (8 // cfg.nbit):
            raise DspsrAmdError("%s: nchan=%d not a multiple of %d samples per byte" % (who, self.nchan, 8 // cfg.nbit))
        if self.nchan * cfg.npol > 65535:
            raise DspsrAmdError("%s: nchan*npol=%d exceeds the grid limit" % (who, self.nchan * cfg.npol))
        self.sd = DelayCarry()
        if cfg.dedisperse:
            self.sd = DelayCarry(front.channel_delays(cfg.dispersion_measure, self.nchan, front.out_rate))
            self.out_start += self.sd.zero / front.out_rate                                 # SampleDelay.C:159
        self.block_bytes = cfg.nsblk * cfg.npol * self.nchan * cfg.nbit // 8
        self.fill = self.nblocks_out = 0

    def open(self, ctx, nmax):
        """for calls of at most `nmax` scrunched samples"""
        cfg, ncol = self.cfg, self.nchan * self.cfg.npol
        self.ctx, self.nmax = ctx, nmax
        if cfg.dedisperse:
            self.sd.check_block("LoadToFITS", nmax)
            self.sample_delay = SampleDelay(ctx, self.sd.delays, cfg.npol)
            self.kbuf = _device_empty(ctx, (self.nchan, cfg.npol, self.sd.head + nmax))
        self.rows = _device_empty(ctx, (self.nchan, cfg.npol, cfg.nsblk - 1 + nmax + self.sd.head))
        self.digitizer = FITSDigitizer(ctx, self.nchan, cfg.npol, cfg.nbit, cfg.nsblk, self.nblock, cfg.rescale_constant,
                                       flip_band=self.info.bandwidth > 0)
        maxblk = max(1, self.rows.shape[2] // cfg.nsblk)
        self.packed = _device_empty(ctx, (maxblk, self.block_bytes), "uint8")
        self.dat_scl = _device_empty(ctx, (maxblk, ncol))
        self.dat_offs = _device_empty(ctx, (maxblk, ncol))

    def destination(self):
        """where the front end writes the scrunched rows of the next call"""
        if self.sample_delay is not None:
            return self.sd.new(self.kbuf)
        return self.rows[:, :, self.fill:self.fill + self.nmax]

    def _place(self, rows):
        """the delayed rows of a call, behind the rows that wait"""
        nd = rows.shape[2]
        if nd:
            copy_data_fpt(self.ctx, self.rows[:, :, self.fill:self.fill + nd], rows)
        return nd

    def blocks(self, nnew):
        """`nnew` rows have arrived at destination(): the blocks they complete, [(bytes, DAT_SCL, DAT_OFFS), ...]"""
        nsblk = self.cfg.nsblk
        if self.sample_delay is not None:                    # in place, LoadToFITS.C:493-494
            nnew = self.sd.delayed(self.ctx, self.sample_delay, self.kbuf, nnew, self._place)
        self.fill += nnew
        out, k = [], 0
        while self.fill - k * nsblk >= nsblk:                # every complete run of nsblk samples is one pack
            self.digitizer.pack(self.rows[:, :, k * nsblk:(k + 1) * nsblk], self.packed[k], self.dat_scl[k], self.dat_offs[k])
            out.append((self.packed[k], self.dat_scl[k], self.dat_offs[k]))
            k += 1
        if k:
            rest = self.fill - k * nsblk
            if rest:
                move_tail_fpt(self.ctx, self.rows, 0, k * nsblk, rest)
            self.fill = rest
            self.nblocks_out += k
        return out

    def close(self):
        _close_all(self.digitizer, self.sample_delay)


class LoadToFITS(_SearchDriver):
    """digifits' chain, CPU branch (Signal/General/LoadToFITS.C:249-553): [Filterbank -F N[:D]] -> Detection straight to the state -p
    names -> TScrunch(tres_factor) -> [SampleDelay at the scrunched rate, -K] -> FITSDigitizer over blocks of nsblk samples, every
    stage on the device: the front end of digifil's drivers (ConvolvingFront with -F, ChannelisedFront on channelised complex
    voltages without) and FitsOutput, in whose collecting buffer the front end's rows land.  process_block(raw, n, first_sample)
    takes the block its front end takes and returns the blocks it completes, a list of (bytes uint8 [nsblk*npol*nchan*nbit/8],
    DAT_SCL float32 [npol*nchan], DAT_OFFS float32 [npol*nchan]) device tensors that stay valid until the next call.  Samples
    short of a block at the end of the data are dropped (InputBuffering)."""

    front = out = None

    def _plan(self):
        who, cfg, info = "dspsr_amd.LoadToFITS", self.cfg, self.info
        refuse_forms(who, info, VOLTAGES, own={"detected": "detected input (the PScrunch branch, LoadToFITS.C:501-514) is not built"})
        if cfg.integration_length:
            raise DspsrAmdError("%s: -L (splitting the output into files of integration_length seconds) is not built" % who)
        if cfg.npol not in (1, 2, 4):
            raise DspsrAmdError("dsp::LoadToFITS::construct invalid polarization specified (npol=%d)" % cfg.npol)
        if cfg.nbit not in (1, 2, 4, 8):
            raise DspsrAmdError("dsp::FITSDigitizer::set_nbit nbit=%i not understood" % cfg.nbit)
        if cfg.nsblk < 1:
            raise DspsrAmdError("%s: nsblk=%d" % (who, cfg.nsblk))
        if cfg.nchan == 0 and info.nchan == 1:
            raise DspsrAmdError("dsp::LoadToFITS::construct must specify filterbank scheme if single channel data")      # :254-258
        if cfg.nchan == 1 or cfg.nchan < 0:
            raise DspsrAmdError("%s: -F %d (a filterbank of at least two channels, or none)" % (who, cfg.nchan))
        response = cfg.coherent_dedisp and cfg.dispersion_measure != 0.0                                               # :260
        if response and not (cfg.nchan > 1 and cfg.convolve):
            raise DspsrAmdError("%s: -do_dedisp without -F N:D is not built (dsp::Convolution behind the filterbank or on the file's "
                                "channels, LoadToFITS.C:329-362)" % who)
        self.tres_factor, self.tsamp, self.nblock = fits_plan(cfg, info)
        if self.tres_factor < 1:
            raise DspsrAmdError("dsp::TScrunch::get_factor scrunch factor not set (tsamp=%g s is below the resolution of the chain)" % cfg.tsamp)
        # the front end: TScrunch by tres_factor, neither -f nor -K (this chain delays the SCRUNCHED rows: FitsOutput)
        front_end, dm, freq_res = ChannelisedFront, 0.0, 0
        if cfg.nchan:
            front_end, freq_res = ConvolvingFront, cfg.freq_res if cfg.freq_res > 1 else 1                              # :318-323
            if response:
                # -x with the response: Dedispersion::set_times_minimum_nfft (:272), not a transform length
                dm, freq_res = cfg.dispersion_measure, 0
                if cfg.freq_res:
                    freq_res = cfg.freq_res * matched_response(info, dm, 0, cfg.nchan, input_nchan=info.nchan, ndim=info.ndim).minimum_ndat
        self.front = front_end(info, nchan=cfg.nchan, dispersion_measure=dm, freq_res=freq_res, tscrunch=self.tres_factor, fscrunch=0,
                               npol=cfg.npol, dedisperse=False, parts_per_block=cfg.parts_per_block, max_parts=cfg.max_parts, fused=cfg.fused,
                               fuse_coherence=cfg.fuse_coherence)
        self.out = FitsOutput(cfg, info, self.front, self.nblock)

    def _open(self):
        self.front.open(self.ctx, own_rows=False)
        self.out.open(self.ctx, self.front.nmax)

    def _parts(self):
        return self.out, self.front

    def process_block(self, raw, n=None, first_sample=0):
        return self.out.blocks(self.front.detect_scrunch(raw, n, first_sample, out=self.out.destination()).shape[2])

    def header_values(self):
        """What the SUBINT header of the PSRFITS file takes (FITSOutputFile.C:247-250,428-431), keyed by its names."""
        cfg, info, bw = self.cfg, self.info, -abs(self.info.bandwidth)
        return dict(NSBLK=cfg.nsblk, TBIN=1.0 / self.out_rate, NBITS=cfg.nbit, ZERO_OFF=2.0 ** (cfg.nbit - 1) - 0.5, NCHAN=self.nchan_out,
                    NPOL=cfg.npol, POL_TYPE=POL_TYPES[cfg.npol], OBSFREQ=info.centre_frequency, OBSBW=bw, CHAN_BW=bw / self.nchan_out,
                    STT_IMJD=info.mjd_day, STT_SECONDS=info.mjd_sec + self.out_start, SRC_NAME=info.source)


for _name in ("nchan_out", "out_rate", "block_bytes", "file_calls"):
    setattr(LoadToFITS, _name, _of("front", _name))
for _name in ("out_start", "sd", "sample_delay", "fill", "nblocks_out"):
    setattr(LoadToFITS, _name, _of("out", _name))
LoadToFITS.block_bytes_out = _of("out", "block_bytes")


def write_search_blocks(path, header, blocks):
    """The hand-off file of a digifits run: a fixed-size ASCII header keyed by the PSRFITS names (LoadToFITS.header_values), then one
    record per block: DAT_OFFS[npol*nchan] float32, DAT_SCL[npol*nchan] float32, DATA[nsblk*npol*nchan*nbit/8].
    blocks: (bytes, dat_scl, dat_offs) as process_block returns them, on the host (numpy)."""
    keys = [("HDR_MAGIC", SEARCH_BLOCKS_MAGIC), ("HDR_VERSION", "1.0"), ("HDR_SIZE", SEARCH_BLOCKS_HDR_SIZE)]
    keys += [(k, repr(float(v)) if isinstance(v, float) else v) for k, v in header.items()]
    keys.append(("NROWS", len(blocks)))
    text = "".join("%-20s %s\n" % (k, v) for k, v in keys)
    if len(text) >= SEARCH_BLOCKS_HDR_SIZE:
        raise DspsrAmdError("write_search_blocks: header does not fit %d bytes" % SEARCH_BLOCKS_HDR_SIZE)
    ncol = int(header["NCHAN"]) * int(header["NPOL"])
    nbytes = int(header["NSBLK"]) * ncol * int(header["NBITS"]) // 8
    with open(path, "wb") as f:
        f.write(text.encode("ascii").ljust(SEARCH_BLOCKS_HDR_SIZE, b"\0"))
        for data, scl, offs in blocks:
            data, scl, offs = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(scl, "<f4"), np.ascontiguousarray(offs, "<f4")
            if data.size != nbytes or scl.size != ncol or offs.size != ncol:
                raise DspsrAmdError("write_search_blocks: a block of %d bytes and %d / %d scales; the header says %d and %d"
                                    % (data.size, scl.size, offs.size, nbytes, ncol))
            f.write(offs.tobytes())
            f.write(scl.tobytes())
            f.write(data.tobytes())


def read_search_blocks(path):
    """Returns (header dict of strings, [(bytes uint8, dat_scl float32, dat_offs float32), ...])."""
    with open(path, "rb") as f:
        raw = f.read(SEARCH_BLOCKS_HDR_SIZE)
        hdr = {}
        for line in raw.split(b"\0", 1)[0].decode("ascii").splitlines():
            parts = line.split(None, 1)
            if len(parts) == 2:
                hdr[parts[0]] = parts[1].strip()
        if hdr.get("HDR_MAGIC") != SEARCH_BLOCKS_MAGIC:
            raise DspsrAmdError("read_search_blocks: %s is not a %s file" % (path, SEARCH_BLOCKS_MAGIC))
        ncol = int(hdr["NCHAN"]) * int(hdr["NPOL"])
        nbytes = int(hdr["NSBLK"]) * ncol * int(hdr["NBITS"]) // 8
        blocks = []
        for _ in range(int(hdr["NROWS"])):
            rec = f.read(8 * ncol + nbytes)
            if len(rec) != 8 * ncol + nbytes:
                raise DspsrAmdError("read_search_blocks: %s is truncated" % path)
            offs = np.frombuffer(rec, "<f4", ncol).copy()
            scl = np.frombuffer(rec, "<f4", ncol, 4 * ncol).copy()
            blocks.append((np.frombuffer(rec, np.uint8, nbytes, 8 * ncol).copy(), scl, offs))
    return hdr, blocks
