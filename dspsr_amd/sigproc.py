"""SIGPROC filterbank files on the input side of the fold (sigproc/read_header.c, SigProcObservation.C, SigProcFile.C and
SigProcUnpacker.C of the reference): a header of length-prefixed keywords from HEADER_START to HEADER_END, then detected spectra in
time order -- spectrum t holds nifs * nchans values of nbits bits, polarisation by polarisation, the first channel in the lowest
bits of a byte.

This is the first branch of LoadToFold::construct (LoadToFold1.C:126-180): the input is detected already, there is no filterbank,
no convolution and no Detection.  The spectra go to the device as they lie in the file and dspsr_amd.unpack_sigproc_fpt
(k_unpack_sigproc) transposes them into float rows: SigprocFile presents the interface dada.DadaFile presents to the drivers, its
blocks are runs of whole spectra.

Host logic only.  Refused by name at open: a frequency table (FREQUENCY_START / fchannel), an unknown keyword, nbits outside
1 / 2 / 4 / 8 / 16 / 32, sub-byte samples whose polarisations do not start on a byte, nifs other than 1 / 2 / 4, tsamp <= 0,
nchans < 1."""
from __future__ import annotations

import os
import struct

import numpy as np

from .engine import DspsrAmdError
from .inputs import InputFile, raw_form, tsamp_us

# read_header.c:50-125: the type of every keyword that carries a value
INT_KEYS = ("nchans", "telescope_id", "machine_id", "data_type", "ibeam", "nbeams", "nbits", "barycentric", "pulsarcentric", "nbins",
            "nsamples", "nifs")
DOUBLE_KEYS = ("az_start", "za_start", "src_raj", "src_dej", "tstart", "tsamp", "period", "fch1", "foff", "refdm")
STRING_KEYS = ("rawdatafile", "source_name")
# sized by the reference's globals (header.h): npuls is a `long int`, isign -- the `signed` key -- a `char`
OTHER_KEYS = {"npuls": "<q", "signed": "<b"}

TELESCOPES = {0: "Fake", 1: "Arecibo", 2: "Ooty", 3: "Nancay", 4: "Parkes", 5: "Jodrell", 6: "GBT", 7: "GMRT", 8: "Effelsberg", 11: "LOFAR",
              12: "VLA"}                                                  # SigProcObservation.C:69-101
MACHINES = {0: "FAKE", 1: "PSPM", 2: "WAPP", 3: "AOFTM", 4: "BPP", 5: "OOTY", 6: "SCAMP", 7: "GMRTFB", 8: "PULSAR2000", 11: "COBALT"}   # :140-175
STATES = {1: "Intensity", 2: "PPQQ", 4: "Coherence"}                      # SigProcObservation.C:198-205
NBITS = (1, 2, 4, 8, 16, 32)                                              # SigProcUnpacker::matches


def telescope_name(telescope_id: int) -> str:
    return TELESCOPES.get(telescope_id, "unknown")


def machine_name(machine_id: int, telescope_id: int) -> str:
    if machine_id == 10:
        return "BPSR" if telescope_id == 4 else "ARTEMIS"
    return MACHINES.get(machine_id, "?????")


def _get_string(f):
    """get_string (read_header.c:15-26): an int32 length, then that many characters; a length outside 1 ... 80 reads as "ERROR".
    Returns None at the end of the file (the reference exits there)."""
    b = f.read(4)
    if len(b) < 4:
        return None
    n = struct.unpack("<i", b)[0]
    if n > 80 or n < 1:
        return "ERROR"
    return f.read(n).decode("latin-1")


def is_valid(path: str) -> bool:
    """The file starts with the length-prefixed string HEADER_START (read_header.c:37-47)."""
    try:
        with open(path, "rb") as f:
            return _get_string(f) == "HEADER_START"
    except OSError:
        return False


def read_header(path: str):
    """read_header (read_header.c:29-138): walk the keywords up to HEADER_END.  Returns (dict keyword -> value, header_bytes).  A
    keyword the reference does not know is an error that names it (the reference exits); so is a frequency table, which
    dsp::SigProcObservation cannot describe (it reads fch1 and foff alone, and the table sets both to 0)."""
    who = "dspsr_amd.sigproc.read_header"
    values, expecting = {}, None
    with open(path, "rb") as f:
        if _get_string(f) != "HEADER_START":
            raise DspsrAmdError("%s: %s does not start with HEADER_START" % (who, path))
        while True:
            s = _get_string(f)
            if s is None:
                raise DspsrAmdError("%s: %s ends before HEADER_END" % (who, path))
            if s == "HEADER_END":
                break
            if s in STRING_KEYS:
                expecting = s
            elif s in ("FREQUENCY_START", "FREQUENCY_END", "fchannel"):
                raise DspsrAmdError("%s: %s holds a frequency table (%s); dsp::SigProcObservation describes evenly spaced channels "
                                    "(fch1, foff) alone" % (who, path, s))
            elif s in INT_KEYS or s in DOUBLE_KEYS or s in OTHER_KEYS:
                fmt = "<i" if s in INT_KEYS else "<d" if s in DOUBLE_KEYS else OTHER_KEYS[s]
                b = f.read(struct.calcsize(fmt))
                if len(b) < struct.calcsize(fmt):
                    raise DspsrAmdError("%s: %s ends inside the value of %s" % (who, path, s))
                values[s] = struct.unpack(fmt, b)[0]
            elif expecting is not None:
                values[expecting], expecting = s, None
            else:
                raise DspsrAmdError("%s: read_header - unknown parameter: %s" % (who, s))
        return values, f.tell()


def check_geometry(who, nbits, nchans, nifs):
    """What dsp::SigProcUnpacker cannot unpack, by name"""
    if nbits not in NBITS:
        raise DspsrAmdError("%s: nbits=%d; dsp::SigProcUnpacker matches nbits 1, 2, 4, 8, 16 and 32" % (who, nbits))
    if nchans < 1:
        raise DspsrAmdError("%s: nchans=%d (nchans >= 1)" % (who, nchans))
    if nifs not in STATES:
        raise DspsrAmdError("%s: nifs=%d; nifs 1 (Intensity), 2 (PPQQ) and 4 (Coherence) name a state (SigProcObservation.C:198-205)" % (who, nifs))
    if nbits < 8 and (nchans * nbits) % 8:
        raise DspsrAmdError("%s: nchans=%d of nbits=%d do not fill whole bytes: a polarisation would start inside a byte, where the "
                            "reference's nchan >> div_shift and (ichan & mod_mask) address the wrong bits for ipol > 0 "
                            "(SigProcUnpacker.C:90,107-110)" % (who, nchans, nbits))


class SigprocFile(InputFile):
    """dsp::SigProcFile + the block loop of dsp::IOManager: a SIGPROC filterbank file cut into the blocks LoadToFold's detected
    back end (pipeline.DetectedFold) consumes: runs of whole spectra as they lie in the file, no overlap, no transposition.

    .info is the pipeline.InputInfo of the stream (info.detected names the state: the driver takes its back end from it), .header the
    values read_header found (the `signed` key among them: read and ignored, as the unpacker ignores it)."""

    def __init__(self, path: str):
        from .pipeline import InputInfo
        who = "dspsr_amd.SigprocFile"
        self.path = path
        h, self.header_bytes = read_header(path)
        self.header = h
        for key in ("nchans", "nbits", "tsamp", "fch1", "foff"):
            if key not in h:
                raise DspsrAmdError("%s: %s has no %s in its header" % (who, path, key))
        nbits, nchans, nifs, tsamp = h["nbits"], h["nchans"], h.get("nifs", 1), h["tsamp"]
        check_geometry(who, nbits, nchans, nifs)
        if not tsamp > 0:
            raise DspsrAmdError("%s: tsamp=%g is not positive" % (who, tsamp))
        self.nbit, self.nchan, self.npol = nbits, nchans, nifs
        self.spectrum_bytes = nifs * nchans * nbits // 8
        nbytes = os.path.getsize(path) - self.header_bytes
        self.ndat = (nbytes * 8) // (nbits * nifs * nchans)             # File::open_fd: from the file size, whole spectra
        fch1, foff, tstart = h["fch1"], h["foff"], h.get("tstart", 0.0)
        telescope_id, machine_id = h.get("telescope_id", 0), h.get("machine_id", 0)
        day = int(np.floor(tstart))
        source = h.get("source_name", "")
        self.coordinates = (h.get("src_raj", 0.0), h.get("src_dej", 0.0))
        self.info = InputInfo(centre_frequency=fch1 + 0.5 * (foff * (nchans - 1)), bandwidth=foff * nchans, nchan=nchans, npol=nifs, ndim=1,
                              tsamp_us=tsamp_us(tsamp), machine=machine_name(machine_id, telescope_id), start_seconds=0.0, mjd_day=day,
                              mjd_sec=(tstart - day) * 86400.0, source=source, telescope=telescope_name(telescope_id), nbit=nbits,
                              detected=STATES[nifs])
        self.extras = {"nbit": nbits, "ndat": 0, "offset_bytes": 0, "source": source, "telescope": telescope_name(telescope_id),
                       "dual_sideband": None, "dm": h.get("refdm"), "resolution": 1}
        self.form = raw_form(self.info)
        self.data = np.memmap(path, dtype=np.int8, mode="r", offset=self.header_bytes,
                              shape=(self.ndat * self.spectrum_bytes,)) if self.ndat else np.zeros(0, np.int8)

    def samples(self, s0, n):
        """Spectra s0 ... s0 + n - 1 as they lie in the file: a view of the memory map"""
        return self.data[s0 * self.spectrum_bytes:(s0 + n) * self.spectrum_bytes]

    def read_units(self, g0, n, channel, granule):
        """A unit is one spectrum (for the detected back end a part is one spectrum, no overlap: InputFile.blocks yields blocks of
        parts_per_block spectra, the last one shorter)."""
        if channel is not None:
            raise DspsrAmdError("dspsr_amd.SigprocFile.blocks: a detected file is not sharded by channel; channel=%d asked" % channel)
        return self.samples(g0, n)
