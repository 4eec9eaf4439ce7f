#!/usr/bin/env python3
"""tools/dspsr_amd_fold.py : the path behind the reference's own option spellings (dspsr.C:207-510) -- a thin driver over
dspsr_amd.dada.fold_file for trying the engine on a DADA file, or on a GUPPI / PUPPI raw file (NBITS 8, several channels: recognised
from the file, no option; dspsr_amd/guppi.py); not a re-implementation of the dspsr application.

  dspsr_amd_fold.py -F 1024:D -D 1000 -b 1024 -c 0.0893 [-x 4096] [-L 10 | -s | -turns N] [-P polyco] [-K] [-d 1|2|4] [-ndim 1|2|4] [-r]
                    (-d npol, dspsr.C:389: 1 total intensity, 2 PP and QQ -- files of STATE Intensity / PPQQ, NPOL 1 / 2, NDIM 1 --,
                    4 the four products, the default; -d 3 reports the reference's refusal.  One-polarisation input with -d 1 or 2
                    folds as STATE PP.  -ndim N, dspsr's -n ndim (dspsr.C:392): the layout of the four products, which -d spelled here before)
  dspsr_amd_fold.py -F 128 ...   (no `:D`: filterbank, THEN coherent dedispersion per channel -- Filterbank::Config::After; -D 0: none)
  dspsr_amd_fold.py -F 128:B ... (coherent dedispersion of the whole band, THEN the filterbank -- Filterbank::Config::Before)
                    [--dump Detection] [--dump Fold] [-O out_prefix] file.dada
  dspsr_amd_fold.py -F 64:D -4 ...   (fourth-order moments: Stokes detection with ndim 4, then the four Stokes parameters and their
                    ten pairwise products folded into every bin -- files of STATE FourthMoment, NPOL 1, NDIM 14)
  dspsr_amd_fold.py -F 64:D -cyclic 256 [-cyclicoversample 4] [-d 1|2|4] ...   (cyclic spectra: dsp::CyclicFold instead of
                    Detection + Fold; -d is then the number of output polarisations, default 4 -- 1 for single-polarisation input)
  dspsr_amd_fold.py -F 16:D -G 256 [-d 1|2|4] ...   (phase-locked filterbank: dsp::PhaseLockedFilterbank instead of Detection + Fold;
                    pulse-phase-resolved spectra in 256 phase bins, one file of NDIM 1 with RATE and NSUB_SWAP; -d is the number of
                    output polarisations, default 4)
  dspsr_amd_fold.py -F 64:D -pac cal.npz ...   (phase-coherent polarimetric calibration, dspsr.C:372: the Jones matrix of every
                    response bin times the chirp, applied inside the filterbank; cal.npz holds `freq` in MHz and `jones` [n][2][2])

  dspsr_amd_fold.py -F 16:D -R ...   (narrow-band RFI filter, dspsr.C:369: the passband of the first second of the file is
                    integrated on the device in 1024 channels, dsp::RFIFilter's mask is multiplied into the dedispersion kernel; the
                    reference's lines `round k cutoff = ...` and `zapped N channels` go to stderr.  A channel zapped in any round
                    stays zapped -- the reference's own loop leaves a mask of all ones)

  dspsr_amd_fold.py -F 16:D -skz [-skzm 128] [-skzs 3] [-skz_start c -skz_end c] [-skz_no_fscr] [-skz_no_tscr] [-skz_no_ft] ...
                    (spectral-kurtosis RFI excision, dspsr.C:289-314: dsp::SpectralKurtosis zeroes what it zaps between the filterbank
                    and Detection, the fold counts its hits per channel -- files with HITS_NCHAN -- and the reference's line
                    `Zapped: total=...% skfb=...% tscr=...% fscr=...%` goes to stderr at the end)

  dspsr_amd_fold.py -F 8:D -2 c10 -2 n512 -2 t0.9674 two_bit.dada   (two-bit input, NBIT 2 of INSTRUMENT CPSR2, dspsr.C:280-287:
                    dsp::TwoBitCorrection's knobs -- excision cutoff in sigma, samples per power estimate, sampling threshold;
                    windows it excises are dropped by the fold, and -r shows their count in the Discarded column)

Every completed sub-integration is written as <prefix>_<n>.ps (the PhaseSeries hand-off file of INTEGRATION.md:
raw sums + hits; dsp::Archiver's normalisation is the reader's job).

Several pulsars from the same data in one pass (dspsr -P a.polyco -P b.polyco): repeat -P and/or -c, one pulsar each (-P files
first, then -c periods, each in the order given).  Pulsar k writes <prefix>_<k>_<n>.ps with its own folding period in the header.
One -P, one -c or one of each is today's single pulsar (a -c given with a -P overrides its period).

  dspsr_amd_fold.py -K -D 26.8 -c 0.7145 -b 256 file.fil   (a SIGPROC filterbank file, recognised from the file: detected input, the
                    first branch of LoadToFold::construct.  No -F: the channels, the polarisations and the STATE of the files written
                    are the file's own (nifs 1 Intensity, 2 PPQQ, 4 Coherence).  -D is needed only with -K, which removes the
                    inter-channel delay with dsp::SampleDelay.  -L, -s, -turns, several -c / -P and -r work as above; -F N with
                    another N, -cyclic, -G, -4, -skz, -R, -pac, --dump and a -d other than the file's are refused by name)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    ap.add_argument("-F", dest="fb", default=None, help="(required for voltages; a SIGPROC filterbank file takes none) nchan:D (convolving filterbank, coherent dedispersion During) or nchan (filterbank, then dsp::Convolution: After)")
    ap.add_argument("-D", dest="dm", type=float, default=None, help="dispersion measure (default: DM of the header)")
    ap.add_argument("-b", dest="nbin", type=int, default=0, help="phase bins (default: dsp::Fold::choose_nbin)")
    ap.add_argument("-c", dest="period", type=float, action="append", default=[], help="constant folding period in seconds (repeat: one pulsar each)")
    ap.add_argument("-P", dest="polyco", action="append", default=[], help="TEMPO polyco file (repeat: one pulsar each)")
    ap.add_argument("-x", dest="nfft", type=int, default=0, help="response (FFT) length per channel")
    ap.add_argument("-L", dest="subint", type=float, default=0.0, help="sub-integration length in seconds")
    ap.add_argument("-s", dest="single", action="store_true", help="single pulses (one turn per sub-integration)")
    ap.add_argument("-turns", dest="turns", type=float, default=0.0, help="turns per sub-integration")
    ap.add_argument("-K", dest="interchan", action="store_true", help="remove the inter-channel dispersion delay")
    # (the attribute keeps the name it had when -d spelled the layout; it holds the reference's npol)
    ap.add_argument("-d", dest="ndim", type=int, default=None, choices=[1, 2, 3, 4],
                    help="output polarisations (dspsr -d npol): 1 Intensity, 2 PPQQ, 4 the four products; also with -cyclic and -G")
    # (dspsr spells it -n; here -n<text> must stay an unrecognised argument: -noskz_too is refused that way)
    ap.add_argument("-ndim", dest="layout", type=int, default=4, choices=[1, 2, 4], help="ndim of the detected rows when npol=4 (dspsr -n ndim, dspsr.C:392)")
    ap.add_argument("-4", dest="fourth", action="store_true", help="compute fourth-order moments")
    ap.add_argument("-cyclic", dest="cyclic", type=int, default=0, help="form cyclic spectra with N channels per filterbank channel")
    ap.add_argument("-cyclicoversample", dest="cyclic_mover", type=int, default=1, help="use M times as many lags to improve the cyclic channel isolation")
    ap.add_argument("-G", dest="plfb_nbin", type=int, default=0, help="create phase-locked filterbank with nbin phase bins")
    ap.add_argument("-pac", dest="pac", default=None, help="phase-coherent polarimetric calibration: .npz with freq (MHz) and jones [n][2][2]")
    ap.add_argument("-R", dest="zap_rfi", action="store_true", help="apply time-variable narrow-band RFI filter")
    ap.add_argument("-skz", dest="skz", action="store_true", help="apply spectral kurtosis filterbank RFI zapping")
    ap.add_argument("-skzm", dest="skzm", type=int, default=128, help="samples to integrate for spectral kurtosis statistics")
    ap.add_argument("-skzs", dest="skzs", type=int, default=3, help="number of std deviations to use for spectral kurtosis excisions")
    ap.add_argument("-skz_start", dest="skz_start", type=int, default=0, help="first channel where signal is expected")
    ap.add_argument("-skz_end", dest="skz_end", type=int, default=0, help="last channel where signal is expected")
    ap.add_argument("-skz_no_fscr", dest="skz_no_fscr", action="store_true", help="do not use SKDetector Fscrunch feature")
    ap.add_argument("-skz_no_tscr", dest="skz_no_tscr", action="store_true", help="do not use SKDetector Tscrunch feature")
    ap.add_argument("-skz_no_ft", dest="skz_no_ft", action="store_true", help="do not use SKDetector despeckeler")
    ap.add_argument("-2", dest="unpack", action="append", default=[], metavar="c<cutoff>|n<samples>|t<threshold>",
                    help="unpacker options (\"2-bit\" excision): c<cutoff> threshold for impulsive interference excision, n<sample> "
                         "number of samples used to estimate undigitized power, t<threshold> two-bit sampling threshold at record time")
    ap.add_argument("-r", dest="record", action="store_true", help="report the time spent in each operation")
    ap.add_argument("--dump", action="append", default=[], help="dump the input of this operation (Detection, Fold)")
    ap.add_argument("-O", dest="prefix", default="dspsr_amd", help="output file name prefix")
    ap.add_argument("--cuda", dest="device", type=int, default=0, help="device id (the reference's spelling)")
    a = ap.parse_args(argv)
    a.d_given = a.ndim is not None
    if a.ndim is None:
        a.ndim = 4
    if a.ndim == 3 and (a.cyclic or a.plfb_nbin):              # nothing changed for -cyclic and -G: 1, 2 or 4
        ap.error("argument -d: invalid choice: 3 (choose from 1, 2, 4)")
    return a


def unpacker_options(unpack, log=None):
    """dspsr.C:530-559: the -2 arguments in order, each tried as n<unsigned>, c<float>, t<float> (what matches none is ignored, as
    there), with the reference's lines on `log`.  Returns the Config fields they set."""
    import re
    out = {}
    number = r"[+-]?(?:\d+\.?\d*(?:[eE][+-]?\d+)?|\.\d+(?:[eE][+-]?\d+)?)"
    for arg in unpack:
        m = re.match(r"n(\d+)", arg)
        if m:
            out["excision_nsample"] = int(m.group(1))
            print("dspsr: Using %d samples to estimate undigitized power" % out["excision_nsample"], file=log or sys.stderr)
            continue
        m = re.match("c(%s)" % number, arg)
        if m:
            out["excision_cutoff"] = float(m.group(1))
            print("dspsr: Setting impulsive interference excision threshold to %g" % out["excision_cutoff"], file=log or sys.stderr)
            continue
        m = re.match("t(%s)" % number, arg)
        if m:
            out["excision_threshold"] = float(m.group(1))
            print("dspsr: Setting two-bit sampling threshold to %g" % out["excision_threshold"], file=log or sys.stderr)
    return out


def detection_options(a, input_npol=2):
    """The Config fields -d and -ndim set.  Plain path: -d is the reference's npol (1 Intensity, 2 PPQQ, 3 its refusal, 4 the four
    products) and -ndim the layout of the four products (dspsr -n, dspsr.C:392) -- until this spelling -d chose that layout here.  With -cyclic
    and -G nothing changed: -d is their number of output polarisations and the rows have ndim 1."""
    if a.cyclic or a.plfb_nbin:
        return dict(ndim=1, npol=a.ndim if a.plfb_nbin else 4, cyclic_npol=(a.ndim if input_npol == 2 else 1) if a.cyclic else 0)
    return dict(ndim=a.layout, npol=a.ndim, cyclic_npol=0)


def fold_targets(a, nbin, out_rate, mjd_day, mjd_sec):
    """The pulsars of repeated -P / -c as pipeline.FoldTarget (nbin: -b, or Fold::choose_nbin per period); [] = one pulsar."""
    from dspsr_amd import pipeline
    if len(a.polyco) < 2 and len(a.period) < 2:
        return []
    out = []
    for path in a.polyco:
        pc = pipeline.Polyco(open(path).read())
        out.append(pipeline.FoldTarget(name=os.path.basename(path), polyco=pc,
                                       nbin=nbin or pipeline.choose_nbin(1.0 / pc.frequency(mjd_day, mjd_sec), out_rate)))
    for p in a.period:
        out.append(pipeline.FoldTarget(name="P=%g" % p, folding_period=p, nbin=nbin or pipeline.choose_nbin(p, out_rate)))
    return out


def detected_input(a):
    """A SIGPROC filterbank file: nchan and state come from the file, -D matters only with -K.  Returns what main() takes of an
    input: (info, the rate of the rows that are folded, dm, the Config fields of this input -- a function: built behind the refusals)."""
    from dspsr_amd import sigproc
    f = sigproc.SigprocFile(a.file)
    info = f.info
    if a.fb is not None and ":" in a.fb:
        sys.exit("-F %s: detected input has no voltages to dedisperse coherently (give no -F)" % a.fb)
    if a.d_given and a.ndim != info.npol:
        sys.exit("-d %d: the file holds %d polarisation(s), STATE %s; detected rows are folded as they are (give no -d)" % (a.ndim, info.npol, info.detected))
    dm = a.dm if a.dm is not None else f.extras["dm"] or 0.0
    if a.interchan and a.dm is None and f.extras["dm"] is None:
        sys.exit("-K needs -D: no refdm in the header")
    # a block of about 64 MiB of float rows, whole spectra
    block = max(1, min(max(f.ndat, 1), (1 << 24) // (info.nchan * info.npol)))
    return info, info.rate, dm, lambda: dict(nchan=int(a.fb) if a.fb is not None else info.nchan, parts_per_block=block)


def voltage_input(a):
    """A DADA or GUPPI raw file: -F says where the coherent dedispersion goes.  Returns what detected_input returns."""
    if a.fb is None:
        sys.exit("the following arguments are required: -F (the input holds voltages)")
    when = "during" if a.fb.endswith(":D") else "before" if a.fb.endswith(":B") else "after"
    if ":" in a.fb and when == "after":
        sys.exit("-F nchan:D (coherent dedispersion During the filterbank), -F nchan (After it) or -F nchan:B (Before it) are on this "
                 "path; not %s" % a.fb)
    from dspsr_amd import dada, guppi
    if guppi.is_valid(a.file):                              # a GUPPI / PUPPI raw file: recognised from the file, no option
        f = guppi.GuppiFile(a.file)
        info, extras = f.info, f.extras
    else:
        hdr, _ = dada.read_header(a.file)
        info, extras = dada.observation(hdr)
    dm = a.dm if a.dm is not None else extras["dm"]
    if dm is None:
        sys.exit("no -D and no DM in the header")
    nchan = int(a.fb.split(":")[0])
    out_rate = info.rate / (2 if info.ndim == 1 else 1) / (nchan // info.nchan)
    return info, out_rate, dm, lambda: dict(
        nchan=nchan, freq_res=a.nfft, cyclic_mover=a.cyclic_mover, **detection_options(a, info.npol), sk_m=a.skzm, sk_std_devs=a.skzs,
        sk_chan_start=a.skz_start, sk_chan_end=a.skz_end, sk_no_fscr=a.skz_no_fscr, sk_no_tscr=a.skz_no_tscr, sk_no_ft=a.skz_no_ft,
        **unpacker_options(a.unpack), convolve_when="never" if when == "after" and dm == 0.0 else when)


def main(argv=None):
    a = parse_args(argv)
    from dspsr_amd import sigproc
    detected = sigproc.is_valid(a.file)                     # a SIGPROC filterbank file: recognised from the file, no option
    info, out_rate, dm, options = (detected_input if detected else voltage_input)(a)
    import torch
    from dspsr_amd import dada, pipeline
    targets = fold_targets(a, a.nbin, out_rate, info.mjd_day, info.mjd_sec)
    period = a.period[0] if len(a.period) == 1 else 0.0
    polyco = pipeline.Polyco(open(a.polyco[0]).read()) if len(a.polyco) == 1 and not targets else None
    if not targets and polyco is None and period <= 0:
        sys.exit("dsp::Fold::fold no polynomial and no period specified (-c or -P)")
    pfold = period if period > 0 else 1.0 / polyco.frequency(info.mjd_day, info.mjd_sec) if polyco else 0.0
    nbin = a.nbin or (pipeline.choose_nbin(pfold, out_rate) if pfold else targets[0].nbin)
    cfg = pipeline.Config(dispersion_measure=dm, nbin=nbin, folding_period=period, subint_seconds=a.subint,
                          subint_turns=1.0 if a.single else a.turns, plfb_nbin=a.plfb_nbin, cyclic_nchan=a.cyclic,
                          interchan_dedispersion=a.interchan, record_time=a.record, fourth_moment=a.fourth, calibrator=a.pac, zap_rfi=a.zap_rfi,
                          sk_zap=a.skz, **options())
    torch.cuda.set_device(a.device)
    lt = dada.fold_file(a.file, cfg, polyco=polyco, device=a.device, stream=torch.cuda.current_stream().cuda_stream,
                        dump_before=tuple(a.dump), targets=targets or None, rfi_log=sys.stderr)
    for line in lt.vitals():
        print(line, file=sys.stderr)
    outputs = [("%s_%%04d.ps" % a.prefix, lt.subints, pfold)]
    if targets:
        outputs = [("%s_%d_%%04d.ps" % (a.prefix, k), p.subints,
                    p.target.folding_period or 1.0 / p.target.polyco.frequency(info.mjd_day, info.mjd_sec))
                   for k, p in enumerate(lt.pulsars)]
    series = {}                                             # what the mode, not Detection, says about the phase series
    if detected:                                            # the file's own channels, under the Config of the detected back end
        cfg, series = lt.cfg, {"nchan": info.nchan}
    if a.cyclic:                                            # nchan * nchan_spec / mover channels, ndim 1 (CyclicFold.C:96-119)
        g = pipeline.cyclic_geometry(cfg, info)
        series = {"nchan": g["nchan"], "state": g["state"]}
    if a.plfb_nbin:                                         # PhaseLockedFilterbank.C:123-159: what it sets on its output
        g = lt.plfb_geometry
        series = {"nchan": g["nchan"], "state": g["state"], "rate": g["rate"], "nsub_swap": g["nsub_swap"]}
    for pattern, subints, pf in outputs:
        for n, sub in enumerate(subints):
            path = pattern % n
            pipeline.write_phase_series(path, sub, info, cfg, npol=lt.npol_out, scale=sub.get("scale", lt.scalefac), division=n,
                                        start_seconds=lt.out_start, folding_period=pf, **series)
            print("dspsr_amd: %s  integration %.6f s  %d samples" % (path, sub["integration_length"], sub["ndat_total"]))
    if a.skz:                                               # SpectralKurtosis.C:53-69, the destructor's line
        st = lt.sk.get_statistics()
        pct = [100 * float(z) / float(st["npart_total"]) if st["npart_total"] else 0.0 for z in st["zap_counts"]]
        print("Zapped:  total=%g%% skfb=%g%% tscr=%g%% fscr=%g%%" % (pct[0], pct[1], pct[3], pct[2]), file=sys.stderr)
    if a.record:
        lt.report()
    lt.close()


if __name__ == "__main__":
    main()
