"""Reference restatements for the phase-locked filterbank (dspsr -G nbin); no device, numpy only.

  plfb_loop        the loop body of dsp::PhaseLockedFilterbank::transformation (Signal/Pulsar/PhaseLockedFilterbank.C:254-297)
                   with numpy.fft, windows in strict time order, in float64 or float32 (numpy >= 2 keeps complex64 / float32
                   transforms in single precision)
  divider_windows  dsp::TimeDivide in turns mode with D = 1 / nbin, walked as ONE PhaseLockedFilterbank::transformation call
                   walks it (PhaseLockedFilterbank.C:208-235): set_bounds (TimeDivide.C:132-346), set_boundaries
                   (:354-501, the phase bin at :486-492) and the sample snapping (:503-540), written from those lines and
                   not from pipeline.TurnsDivider; times are seconds of the stream, phases (integer turns, fraction)
"""
import math

import numpy as np


def plfb_loop(rows, ndim, nchan, npol_out, nbin, starts, bins, dtype=np.float64, out=None):
    """rows: [nchan_in][npol_in][ndat * ndim] real array (any float type; converted to dtype).  Returns
    [nchan_in * nchan][npol_out][nbin] of dtype (added to `out` when given)."""
    dtype = np.dtype(dtype)
    cdtype = np.complex128 if dtype == np.float64 else np.complex64
    rows = np.asarray(rows).astype(dtype)
    nchan_in, npol_in = rows.shape[:2]
    ndat_fft = nchan if ndim == 2 else 2 * nchan                                  # :100-110
    if npol_in < 2 and npol_out > 1:
        raise ValueError("Not enough input polns")                                # :138-141
    prof = np.zeros((nchan_in * nchan, npol_out, nbin), dtype=dtype) if out is None else out
    for s, b in zip(starts, bins):
        s, b = int(s), int(b)
        for c in range(nchan_in):
            spec = []
            for p in range(npol_in):
                seg = rows[c, p, s * ndim:(s + ndat_fft) * ndim]
                assert seg.size == ndat_fft * ndim, "window past the rows"
                if ndim == 1:
                    x = np.fft.rfft(seg)[:nchan]                                  # frc1d: bins 0 .. nchan-1 of the 2 nchan transform
                else:
                    x = np.fft.fft(np.ascontiguousarray(seg).view(cdtype))        # fcc1d
                assert x.dtype == cdtype
                spec.append(x)
                amps = prof[c * nchan:(c + 1) * nchan, 0 if npol_out == 1 else p, b]
                amps += x.real * x.real                                           # :275
                amps += x.imag * x.imag                                           # :276
            if npol_out > 2:
                x0, x1 = spec
                prof[c * nchan:(c + 1) * nchan, 2, b] += x0.real * x1.real + x0.imag * x1.imag      # :288-290
                prof[c * nchan:(c + 1) * nchan, 3, b] += x0.real * x1.imag - x0.imag * x1.real      # :291-293
    return prof


def reference_nchan(period, rate, nbin):
    """PhaseLockedFilterbank::prepare, :65-73: the largest power of two <= the samples per phase bin."""
    samples_per_bin = period * rate / nbin
    return int(math.pow(2.0, math.floor(math.log(samples_per_bin) / math.log(2.0))))


def _padd(ph, turns):
    """Pulsar::Phase + double: (integer turns, fraction in [0, 1))"""
    f = ph[1] + turns
    fl = math.floor(f)
    return (ph[0] + int(fl), f - fl)


def divider_windows(phase, iphase, t_start, rate, nbin, reference_phase, ndat, ndat_fft):
    """One transformation call over `ndat` samples that start at t_start (seconds): the (idat_start, phase_bin) of every window
    the loop at PhaseLockedFilterbank.C:208-235 transforms.  phase(t) -> (int, frac); iphase((int, frac), t_guess) -> t."""
    D = 1.0 / float(nbin)                                                         # PhaseLockedFilterbank.C:36-40
    input_start, input_end = t_start, t_start + ndat / rate
    st = {"start_phase": None, "start_time": t_start, "lower": None, "upper": None, "bin": 0, "period": None}

    def set_boundaries(t_in):                                                     # TimeDivide.C:354-501
        if st["start_phase"] is None:                                             # :360-437, division_turns < 1
            pi, pf = phase(st["start_time"])
            x_minus_r = pf - reference_phase
            if pf < reference_phase:
                x_minus_r += 1.0
                pi -= 1
            n = int(math.ceil(x_minus_r / D))
            x = reference_phase + n * D
            st["start_phase"] = (pi + int(math.floor(x)), x - math.floor(x))      # Phase (intturns, X)
            st["start_time"] = iphase(st["start_phase"], st["start_time"])
        divide_start = max(st["start_time"], t_in)
        ip = phase(divide_start)
        turns = (ip[0] - st["start_phase"][0]) + (ip[1] - st["start_phase"][1])
        division = int(turns / D)                                                 # :482
        ip = _padd(st["start_phase"], division * D)                               # :484
        ft = _padd(_padd(ip, -reference_phase), 0.5 * D)[1]                       # :488-490
        st["bin"] = int(ft / D)                                                   # :491
        mjd1 = iphase(ip, divide_start)
        mjd2 = iphase(_padd(ip, D), mjd1 + D * st["period"])
        # :503-540: both boundaries snapped to samples of the input
        samples = int(round((mjd1 - input_start) * rate))                         # lrint
        st["lower"] = input_start + samples / rate
        division_ndat = int(round((mjd2 - st["lower"]) * rate))
        st["upper"] = st["lower"] + division_ndat / rate

    # a period for iphase's initial guesses only
    p0, p1 = phase(t_start), phase(t_start + 1e-3)
    st["period"] = 1e-3 / ((p1[0] - p0[0]) + (p1[1] - p0[1]))

    wins = []
    is_valid, current_end = False, None
    while True:
        divide_start = input_start                                                # set_bounds, :146-158
        if is_valid:
            divide_start = max(current_end, input_start)
        if st["lower"] is None or input_end < st["lower"] or divide_start + 0.5 / rate > st["upper"]:
            set_boundaries(divide_start + 0.55 / rate)                            # :164-186
        divide_start = max(st["lower"], divide_start)                             # :188
        idat_start = int(round((divide_start - input_start) * rate))              # :201-211, rint
        if idat_start >= ndat:                                                    # :217-226, then PhaseLockedFilterbank.C:224-228
            break
        divide_end = min(input_end, st["upper"])                                  # :232
        idat_end = min(int(round((divide_end - input_start) * rate)), ndat)       # :241-297
        assert idat_end > idat_start
        is_valid, current_end = True, input_start + idat_end / rate               # :344-345
        if idat_start + ndat_fft > ndat:                                          # PhaseLockedFilterbank.C:224-228
            break
        wins.append((idat_start, st["bin"]))                                      # :230-235
    return wins


def window_totals(wins, nbin, ndat_fft, rate):
    """hits, ndat_total, integration_length of PhaseLockedFilterbank.C:233-235,306 (integration_length summed in window order)."""
    hits = np.zeros(nbin, dtype=np.uint32)
    total, time_per_fft = 0.0, float(ndat_fft) / rate
    for _, b in wins:
        hits[b] += 1
        total += time_per_fft
    return hits, len(wins), total
