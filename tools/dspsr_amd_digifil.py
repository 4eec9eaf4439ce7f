#!/usr/bin/env python3
"""tools/dspsr_amd_digifil.py : search mode on an already channelised 8-bit voltage file, behind the reference's own option
spellings (digifil.C:78-131) -- a thin driver over pipeline.LoadToFilDirect for trying the path on a DADA file; not a
re-implementation of the digifil application.

  dspsr_amd_digifil.py file.dada [-b nbit] [-t T] [-f F] [-d npol] [-K [-D dm]] [-I secs] [-c] [-s fac] [-B MB] [-o out.fil]
                       [--fuse-coherence]

The file must be channelised complex voltages (NCHAN >= 1, NDIM 2, NBIT 8): there is no -F here, the channels of the output
are those of the file (LoadToFil.C:233-234).  The blocks are read with dspsr_amd.dada, copied to the device, and the packed
bytes follow the SIGPROC header in the output file."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    ap.add_argument("-b", dest="nbit", type=int, default=8, choices=[1, 2, 4, 8, 16, -32], help="number of bits per sample output to file")
    ap.add_argument("-B", dest="block_mb", type=float, default=64.0, help="block size in megabytes")
    ap.add_argument("-c", dest="constant", action="store_true", help="keep offset and scale constant")
    ap.add_argument("-K", dest="dedisperse", action="store_true", help="remove inter-channel dispersion delays")
    ap.add_argument("-D", dest="dm", type=float, default=None, help="set the dispersion measure (default: DM of the header)")
    ap.add_argument("-t", dest="tscrunch", type=int, default=1, help="decimate in time")
    ap.add_argument("-f", dest="fscrunch", type=int, default=0, help="decimate in frequency")
    ap.add_argument("-d", dest="npol", type=int, default=1, help="1=PP+QQ, 2=PP,QQ, 4=PP,QQ,PQ,QP")
    ap.add_argument("-I", dest="rescale_seconds", type=float, default=10.0, help="rescale interval in seconds (0: no rescaling)")
    ap.add_argument("-s", dest="scale_fac", type=float, default=1.0, help="data scale factor to apply")
    ap.add_argument("-o", dest="output", default=None, help="output filename")
    ap.add_argument("--cuda", dest="device", type=int, default=0, help="device id (the reference's spelling)")
    ap.add_argument("--fuse-coherence", dest="fuse_coherence", action="store_true",
                    help="-d 4 behind a convolving filterbank: detection and time scrunch inside the inverse pass (not a reference "
                         "spelling; SearchConfig.fuse_coherence -- this driver has no -F, its one-pass front end ignores it)")
    return ap.parse_args(argv)


def search_config(a, info, extras):
    """pipeline.SearchConfig of the parsed options for an input of `info` (DADA header; extras: dada.observation's second value)."""
    from dspsr_amd import DspsrAmdError, pipeline
    dm = a.dm if a.dm is not None else extras.get("dm")
    if a.dedisperse and not dm:
        raise DspsrAmdError("dspsr_amd_digifil: -K needs a dispersion measure (DM in the header, or -D)")
    per_sample = info.nchan * info.npol * info.ndim
    ndat = max(1, int(a.block_mb * 1024 * 1024) // per_sample)
    return pipeline.SearchConfig(nchan=info.nchan, tscrunch=max(1, a.tscrunch), nbit=a.nbit, rescale_seconds=a.rescale_seconds,
                                 rescale_constant=a.constant, scale_fac=a.scale_fac, parts_per_block=ndat,
                                 dispersion_measure=float(dm or 0.0), fscrunch=a.fscrunch, npol=a.npol, dedisperse=a.dedisperse,
                                 fuse_coherence=a.fuse_coherence)


def write_header(f, lt, info, rawdatafile):
    """The SIGPROC header of `lt`'s output (pipeline.write_sigproc_header with lt.header_values())."""
    from dspsr_amd import pipeline
    pipeline.write_sigproc_header(f, source_name=info.source, rawdatafile=os.path.basename(rawdatafile), **lt.header_values())


def main(argv=None):
    a = parse_args(argv)
    import torch

    from dspsr_amd import inputs, pipeline
    df = inputs.open_input(a.file)                          # (a GUPPI raw file is recognised here and refused by LoadToFilDirect, by name)
    info = df.info
    info.nbit = df.extras["nbit"]
    cfg = search_config(a, info, df.extras)
    lt = pipeline.LoadToFilDirect(cfg, info, device=a.device)
    out = a.output or os.path.splitext(os.path.basename(a.file))[0] + ".fil"
    nsamp = 0
    with open(out, "wb") as f:
        write_header(f, lt, info, a.file)
        for raw, ndat in lt.file_calls(df):
            packed = lt.process_block(torch.from_numpy(raw.copy()).to("cuda:%d" % a.device), ndat)
            packed.cpu().numpy().tofile(f)
            nsamp += packed.numel() // lt.bytes_per_sample
    lt.synchronize()
    lt.close()
    print("%s: %d samples of %d channels x %d pol, %d bit" % (out, nsamp, lt.nchan_out, cfg.npol, 32 if cfg.nbit == -32 else cfg.nbit))
    return 0


if __name__ == "__main__":
    sys.exit(main())
