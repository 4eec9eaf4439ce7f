"""GUPPI / PUPPI raw files on the input side of the path (guppi/GUPPIFile.C, GUPPIBlockFile.C, GUPPIUnpacker.C of the reference):
a sequence of blocks, each a FITS-style header of 80-character cards closed by an END card and a data section of BLOCSIZE bytes.
Inside a data section the channels are time-ordered runs: run c holds the consecutive samples of channel c, 2 * npol int8 each
((re, im) of polarisation 0, then of polarisation 1), and the last OVERLAP samples of every run repeat the next block's first ones.

The reference un-transposes every block on the host (GUPPIBlockFile::load_bytes: one memcpy per sample and channel) and unpacks
the TFP bytes.  Here the data sections go to the device as they lie in the file and dspsr_amd.unpack_guppi_fpt (k_unpack_guppi)
writes the float rows: GuppiFile presents the interface dada.DadaFile presents to the drivers, its blocks are whole data sections.

Host logic only.  Built: 8-bit complex samples of several channels (PKTFMT 1SFA and its kin).  Refused by name at open: NBITS 2 / 4,
PKTFMT VDIF and SIMPLE, OBSNCHAN 1, DIRECTIO headers, a BACKEND the unpacker does not match."""
from __future__ import annotations

import os
import re

import numpy as np

from .engine import DspsrAmdError
from .inputs import InputFile, open_input, raw_form, tsamp_us          # noqa: F401  (open_input: the factory's earlier home)

CARD = 80                    # bytes of a header card
MAX_CARDS = 2304             # GUPPIFile.C:49
REQUIRED = ("NBITS", "OBSBW", "OBSFREQ", "OBSNCHAN", "NPOL", "PKTFMT", "PKTSIZE", "TBIN", "OVERLAP", "BLOCSIZE", "STT_IMJD", "STT_SMJD",
            "STT_OFFS", "PKTIDX", "TELESCOP", "SRC_NAME", "BACKEND", "FD_POLN", "RA_STR", "DEC_STR", "FRONTEND")     # GUPPIBlockFile.C:51-160
_END = b"END" + b" " * (CARD - 3)


def _card_value(card: str):
    """The value of a `KEYWORD = value / comment` card as text: a quoted string without its quotes and trailing blanks, else the
    first token."""
    v = card[card.index("=") + 1:].strip()
    if v.startswith("'"):
        e = v.find("'", 1)
        return (v[1:e] if e > 0 else v[1:]).rstrip()
    return v.split("/", 1)[0].strip()


def read_header(f):
    """get_header (GUPPIFile.C:41-84) from the current position of the binary file object `f`: cards of 80 characters up to and
    including the END card, at most 2304 of them.  Returns (dict keyword -> value text, header bytes), or (None, 0) when no END card
    is found; the file is then left wherever the reading stopped."""
    cards, count, got_end = {}, 0, False
    while count < MAX_CARDS and not got_end:
        card = f.read(CARD)
        if len(card) != CARD:
            break
        count += 1
        if card == _END:
            got_end = True
            break
        text = card.decode("latin-1")
        key = text[:8].strip()
        if key and "=" in text[8:10] and key not in cards:          # hget: the first card of a keyword
            cards[key] = _card_value(text)
    if not got_end:
        return None, 0
    return cards, count * CARD


def is_valid(path: str) -> bool:
    """GUPPIFile::is_valid (GUPPIFile.C:86-124): a first header with an END card that holds BLOCSIZE and PKTIDX."""
    try:
        with open(path, "rb") as f:
            cards, _ = read_header(f)
    except OSError:
        return False
    return cards is not None and "BLOCSIZE" in cards and "PKTIDX" in cards


def _number(cards, key, conv):
    try:
        return conv(cards[key])
    except KeyError:
        raise DspsrAmdError("dsp::GUPPIBlockFile::parse_header Couldn't find %s keyword in header." % key)
    except ValueError:
        m = re.match(r"[+-]?(\d+\.?\d*([eEdD][+-]?\d+)?|\.\d+([eEdD][+-]?\d+)?)", cards[key])
        if not m:
            raise DspsrAmdError("dspsr_amd.guppi: %s = %r is not a number" % (key, cards[key]))
        return conv(float(m.group(0).replace("D", "E").replace("d", "e")))


class GuppiFile(InputFile):
    """dsp::GUPPIFile + the block loop of dsp::IOManager: an 8-bit GUPPI / PUPPI raw file cut into the blocks LoadToFold consumes.
    Opening indexes the file once -- header offset, data offset and PKTIDX of every block -- and applies the reference's rules:
    a first block of another BLOCSIZE is skipped (GUPPIFile.C:144-164); the stream holds nblocks * block_nsamp samples with nblocks from
    the file size (:174-177); a block whose PKTIDX does not advance is skipped, missing blocks are delivered as zeros in front of the
    block behind the gap, a gap that is no whole number of blocks delivers none (GUPPIBlockFile.C:238-294).  `log`: where the
    reference's three stderr lines go.

    .info is the pipeline.InputInfo of the stream (info.guppi = (block_nsamp, chan_stride, BLOCSIZE): the drivers take the layout
    from it), .stream the delivered blocks: a data offset in the file each, or None for a block of zeros."""

    def __init__(self, path: str, log=None):
        from .pipeline import InputInfo
        self.path = path
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            cards, hb = read_header(f)
            if cards is None:
                raise DspsrAmdError("dsp::GUPPIFile::open_file Error parsing block0 header.")
            for key in REQUIRED:
                if key not in cards:
                    raise DspsrAmdError("dsp::GUPPIBlockFile::parse_header Couldn't find %s keyword in header." % key)
            blocsize0 = _number(cards, "BLOCSIZE", int)
            f.seek(hb + blocsize0)
            cards1, hb1 = read_header(f)
            if cards1 is None:
                raise DspsrAmdError("dsp::GUPPIFile::open_file Error parsing block1 header.")
            pos0 = 0
            if _number(cards1, "BLOCSIZE", int) != blocsize0:          # the first block is ignored: the stream starts at the second
                pos0, cards, hb = hb + blocsize0, cards1, hb1
                for key in REQUIRED:
                    if key not in cards:
                        raise DspsrAmdError("dsp::GUPPIBlockFile::parse_header Couldn't find %s keyword in header." % key)
            self.cards, self.header_bytes, self.pos0 = cards, hb, pos0
            self._parse(cards, InputInfo)
            nblocks = (size - pos0) // (self.blocsize + hb)
            self.ndat = nblocks * self.block_nsamp
            self.index = self._index(f, size)
        self.stream = self._stream(self.index, log)[:nblocks]
        self.data = np.memmap(path, dtype=np.int8, mode="r") if size else np.zeros(0, np.int8)
        self.form = raw_form(self.info)

    def _parse(self, c, InputInfo):
        who = "dspsr_amd.GuppiFile"
        nbit, nchan = _number(c, "NBITS", int), _number(c, "OBSNCHAN", int)
        npol = 1 if _number(c, "NPOL", int) == 1 else 2
        pktfmt, backend = c["PKTFMT"].strip(), c["BACKEND"].strip()
        if nbit != 8:
            raise DspsrAmdError("%s: NBITS=%d; 8-bit samples are read (the 2-bit and 4-bit unpackers GUPPITwoBitCorrection and GUPPIFourBit "
                                "are not built)" % (who, nbit))
        if pktfmt == "VDIF":
            raise DspsrAmdError("%s: PKTFMT VDIF (real, unsigned samples) is not built" % who)
        if pktfmt == "SIMPLE":
            raise DspsrAmdError("%s: PKTFMT SIMPLE (channel-interleaved blocks) is not built; the time-ordered runs of the other formats are" % who)
        if nchan <= 1:
            raise DspsrAmdError("%s: OBSNCHAN %d (real-sampled single-channel data) is not built" % (who, nchan))
        if len(backend) != 5 or backend[1:] != "UPPI":
            raise DspsrAmdError("%s: BACKEND %s; dsp::GUPPIUnpacker matches ?UPPI (GUPPI, PUPPI, ...) with NBITS 8" % (who, backend))
        if "DIRECTIO" in c and _number(c, "DIRECTIO", int) != 0:
            raise DspsrAmdError("%s: DIRECTIO=%s (headers padded to 512 bytes) is not built" % (who, c["DIRECTIO"]))
        self.blocsize, self.overlap = _number(c, "BLOCSIZE", int), _number(c, "OVERLAP", int)
        self.packet_size = _number(c, "PKTSIZE", int)
        sb = 2 * npol
        if self.blocsize <= 0 or self.blocsize % (nchan * sb):
            raise DspsrAmdError("%s: BLOCSIZE=%d is not a multiple of nchan * 2 * npol = %d" % (who, self.blocsize, nchan * sb))
        self.chan_stride = self.blocsize // nchan
        if not 0 <= self.overlap < self.chan_stride // sb:
            raise DspsrAmdError("%s: OVERLAP=%d is not below the %d samples of a run" % (who, self.overlap, self.chan_stride // sb))
        self.block_nsamp = self.chan_stride // sb - self.overlap
        self.block_stride = self.blocsize
        self.packets_per_block = (self.blocsize - self.overlap * sb * nchan) // self.packet_size if self.packet_size > 0 else 0
        if self.packets_per_block < 1:
            raise DspsrAmdError("%s: PKTSIZE=%d gives no whole packet per block of %d bytes" % (who, self.packet_size, self.blocsize))
        tbin = _number(c, "TBIN", float)
        if tbin <= 0:
            raise DspsrAmdError("%s: TBIN=%g is not positive" % (who, tbin))
        rate, ndim = 1.0 / tbin, 2
        self.pktidx0 = _number(c, "PKTIDX", int)
        t_offset = _number(c, "STT_OFFS", float)
        t_offset += self.pktidx0 * self.packet_size * 8.0 / rate / (nbit * nchan * npol * ndim)               # GUPPIBlockFile.C:119-120
        self.basis = "Circular" if c["FD_POLN"].strip().upper().startswith("CIR") else "Linear"
        self.receiver, self.coordinates = c["FRONTEND"], (c["RA_STR"], c["DEC_STR"])
        self.info = InputInfo(centre_frequency=_number(c, "OBSFREQ", float), bandwidth=_number(c, "OBSBW", float), nchan=nchan, npol=npol,
                              ndim=ndim, tsamp_us=tsamp_us(tbin), machine=backend, start_seconds=0.0, mjd_day=_number(c, "STT_IMJD", int),
                              mjd_sec=_number(c, "STT_SMJD", int) + t_offset, source=c["SRC_NAME"], telescope=c["TELESCOP"], nbit=8,
                              guppi=(self.block_nsamp, self.chan_stride, self.blocsize))
        self.extras = {"nbit": 8, "ndat": 0, "offset_bytes": 0, "source": c["SRC_NAME"], "telescope": c["TELESCOP"], "dual_sideband": None,
                       "dm": None, "resolution": 1}

    def _index(self, f, size):
        """[(header offset, data offset, PKTIDX)] of every whole block from the start position on (load_next_block: a header that
        does not parse, or a data section cut short, ends the data)"""
        index, pos = [], self.pos0
        while pos < size:
            f.seek(pos)
            cards, hb = read_header(f)
            if cards is None or pos + hb + self.blocsize > size:
                break
            index.append((pos, pos + hb, _number(cards, "PKTIDX", int)))
            pos += hb + self.blocsize
        return index

    def _stream(self, index, log):
        """The delivered blocks (GUPPIBlockFile.C:238-294): data offsets, None for zeros"""
        if not index:
            return []
        who, ppb = "dsp::GUPPIBlockFile::load_bytes()", self.packets_per_block
        stream, last = [index[0][1]], index[0][2]
        for _hdr, data, idx in index[1:]:
            diff = idx - last
            if diff <= 0:
                if diff < 0 and log is not None:
                    print("%s unordered pktidx=%d last=%d diff=%d inc=%d" % (who, idx, last, diff, ppb), file=log)
                continue
            if diff != ppb:
                if log is not None:
                    print("%s skipped pktidx=%d last=%d diff=%d inc=%d" % (who, idx, last, diff, ppb), file=log)
                if diff % ppb:
                    if log is not None:
                        print("%s WARNING fraction skipped block" % who, file=log)
                else:
                    stream.extend([None] * (diff // ppb - 1))
            stream.append(data)
            last = idx
        return stream

    def usable(self, lt=None):
        """Samples the block loop reads: the stream's, never past ndat (skipped blocks leave the stream shorter than ndat)"""
        return min(self.ndat, len(self.stream) * self.block_nsamp)

    def sections(self, k0, nblk, channel=None):
        """int8 host array: the data sections of stream blocks k0 ... k0 + nblk - 1, BLOCSIZE bytes each and contiguous (zeros for a
        missing block); channel = g: that channel's runs alone, chan_stride bytes per block"""
        per = self.blocsize if channel is None else self.chan_stride
        out = np.empty(nblk * per, np.int8)
        for i, data in enumerate(self.stream[k0:k0 + nblk]):
            if data is None:
                out[i * per:(i + 1) * per] = 0
            else:
                a = data if channel is None else data + channel * self.chan_stride
                out[i * per:(i + 1) * per] = self.data[a:a + per]
        return out

    def read_units(self, g0, n, channel, granule):
        """The whole stream blocks that hold a pipeline block (InputFile.blocks), with block_stride = BLOCSIZE; channel = g: channel
        g's runs only, a block with nchan = 1 and block_stride = chan_stride."""
        if channel is not None and not 0 <= channel < self.info.nchan:
            raise DspsrAmdError("dspsr_amd.GuppiFile.blocks: channel=%d outside the %d channels" % (channel, self.info.nchan))
        return self.sections(g0, n, channel)
