#!/usr/bin/env python3
"""tools/dspsr_amd_digifits.py : PSRFITS search mode on an 8-bit DADA voltage file, behind the reference's own option spellings
(digifits.C:78-145) -- a thin driver over pipeline.LoadToFITS; not a re-implementation of the digifits application.

  dspsr_amd_digifits.py file.dada [-F nchan[:D]] [-x nfft] [-D dm] [-do_dedisp bool] [-t tsamp] [-p npol] [-b bits] [-nsblk N]
                                  [-I secs] [-c] [-K] [-o out.sblk] [--cuda id]

PSRFITS itself is written by cfitsio from a PSRCHIVE template; neither is here.  The output is the hand-off file of
pipeline.write_search_blocks: the SUBINT header values by their PSRFITS names, then DAT_OFFS, DAT_SCL and DATA of
every block."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _bool(s):
    if s.lower() in ("1", "true", "yes", "y"):
        return True
    if s.lower() in ("0", "false", "no", "n"):
        return False
    raise argparse.ArgumentTypeError("bool expected, not %r" % s)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    ap.add_argument("-D", dest="dm", type=float, default=None, help="set the dispersion measure (default: DM of the header)")
    ap.add_argument("-x", dest="freq_res", type=int, default=0, help="set backward FFT length in voltage filterbank")
    ap.add_argument("-do_dedisp", dest="coherent_dedisp", type=_bool, default=False, metavar="bool", help="enable coherent dedispersion (default: false)")
    ap.add_argument("-c", dest="constant", action="store_true", help="keep offset and scale constant")
    ap.add_argument("-I", dest="rescale_seconds", type=float, default=-1.0, help="rescale interval in seconds")
    ap.add_argument("-t", dest="tsamp", type=float, default=64e-6, help="integration time (s) per output sample (default=64mus)")
    ap.add_argument("-p", dest="npol", type=int, default=4, help="output 1 (Intensity), 2 (AABB), or 4 (Coherence) products")
    ap.add_argument("-b", dest="nbit", type=int, default=2, help="number of bits per sample output to file [1,2,4,8]")
    ap.add_argument("-F", dest="filterbank", default=None, metavar="nchan[:D]", help="create a filterbank (voltages only)")
    ap.add_argument("-nsblk", dest="nsblk", type=int, default=2048, help="output block size in samples (default=2048)")
    ap.add_argument("-L", dest="integration_length", type=float, default=0.0, help="set maximum file length (not built)")
    ap.add_argument("-K", dest="dedisperse", action="store_true", help="remove inter-channel dispersion delays")
    ap.add_argument("-o", dest="output", default=None, help="output filename")
    ap.add_argument("--cuda", dest="device", type=int, default=0, help="device id (the reference's spelling)")
    ap.add_argument("--parts", dest="parts_per_block", type=int, default=0, help="parts (-F) or time samples (no -F) per call")
    ap.add_argument("--fuse-coherence", dest="fuse_coherence", action="store_true",
                    help="-F with -p 4: detection and time scrunch inside the inverse pass where the tile fits (not a reference spelling; "
                         "the same bytes)")
    return ap.parse_args(argv)


def fits_config(a, extras):
    """pipeline.FitsConfig of the parsed options (extras: dada.observation's second value)."""
    from dspsr_amd import DspsrAmdError, pipeline
    nchan, convolve = 0, False
    if a.filterbank:
        head, _, when = a.filterbank.partition(":")
        nchan = int(head)
        if when not in ("", "D", "d"):
            raise DspsrAmdError("dspsr_amd_digifits: -F %s (nchan or nchan:D; during is the only option for the filterbank)" % a.filterbank)
        convolve = bool(when)
    dm = a.dm if a.dm is not None else extras.get("dm")
    kw = dict(parts_per_block=a.parts_per_block) if a.parts_per_block else (dict(parts_per_block=65536) if not nchan else {})
    return pipeline.FitsConfig(nchan=nchan, convolve=convolve, freq_res=a.freq_res, dispersion_measure=float(dm or 0.0),
                               coherent_dedisp=a.coherent_dedisp, tsamp=a.tsamp, npol=a.npol, nbit=a.nbit, nsblk=a.nsblk,
                               rescale_seconds=a.rescale_seconds, rescale_constant=a.constant, dedisperse=a.dedisperse,
                               integration_length=a.integration_length, fuse_coherence=a.fuse_coherence, **kw)


def main(argv=None):
    a = parse_args(argv)
    from dspsr_amd import dada, inputs, pipeline
    cfg = fits_config(a, inputs.open_input(a.file).extras)   # a DADA file, or a GUPPI raw file: recognised from the file
    header, blocks = dada.search_blocks_file(a.file, cfg, device=a.device, log=sys.stderr)
    out = a.output or os.path.splitext(os.path.basename(a.file))[0] + ".sblk"
    pipeline.write_search_blocks(out, header, blocks)
    print("%s: %d blocks of %d samples, %d channels x %d pol, %d bit" % (out, len(blocks), cfg.nsblk, header["NCHAN"], cfg.npol, cfg.nbit))
    return 0


if __name__ == "__main__":
    sys.exit(main())
