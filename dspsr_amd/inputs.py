"""What kind of block a run is looking at, said once: the form of the input (generic DADA bytes, the CASPSR interleave, MeerKAT
heaps, CPSR2's two-bit windows, GUPPI raw blocks, detected spectra) and the protocol of the files that deliver it.

A form is built once per run by raw_form() from the pipeline.InputInfo and answers every question the drivers, the readers and
the RFI filter have about the bytes of a block: on which sample boundary it starts (granule), the layout word of the block in hand,
its size in bytes, and the words a driver without a reader for it refuses it with.  InputFile is what dada.DadaFile,
guppi.GuppiFile and sigproc.SigprocFile share: the block loop of dsp::IOManager over whole units of the form's granule.  A new
format is one form, one reader (read_units) and one unpacker.  Host logic only."""
from __future__ import annotations

import math
from dataclasses import dataclass

from . import _lib
from .engine import DspsrAmdError, twobit_block_bytes


@dataclass(frozen=True)
class Form:
    """The generic DADA order ([t][chan][pol][dim] int8), and what every other form overrides."""
    layout: int = _lib.RAW_GENERIC    # the layout word of a block that starts on a granule
    granule: int = 1                  # a block the readers cut starts inside a whole unit of this many samples, at first_sample of it
    geometry: tuple | None = None     # GUPPI raw blocks: (block_nsamp, chan_stride, block_stride), as FilterbankEngine.set_guppi takes it
    name = "generic"

    def describe(self, info):
        return "the generic DADA byte order"

    def refusal(self, info, instead):
        return "%s is not built on this path; %s" % (self.describe(info), instead)

    def layout_word(self, first_sample=0):
        if first_sample:
            raise DspsrAmdError("dspsr_amd.pipeline: first_sample=%d given for a layout without heaps" % first_sample)
        return self.layout

    def block_bytes(self, nsamp, nchan, npol, ndim, first_sample=0):
        """Bytes of the whole units that hold `nsamp` samples from `first_sample` of the first one on."""
        if self.granule == 1:
            self.layout_word(first_sample)               # (refuses a first sample where a block has none)
        return _lib.raw_block_bytes(self.layout, nsamp, nchan, npol, ndim, first_sample, self.geometry)


@dataclass(frozen=True)
class Caspsr(Form):
    """One channel of two real polarisations, 4 bytes of one then 4 of the other (CASPSRUnpacker.C:132-187)."""
    layout: int = _lib.RAW_CASPSR
    name = "caspsr"

    def describe(self, info):
        return "the CASPSR byte order"

    def refusal(self, info, instead):
        return "%s is not built on this path (generic DADA order only)" % self.describe(info)


@dataclass(frozen=True)
class Heaps(Form):
    """MeerKAT beamformer heaps, plain (MKBF) or with odd and even samples exchanged (MKBFRo)."""
    layout: int = _lib.RAW_MEERKAT
    granule: int = _lib.HEAP_NSAMP
    name = "heaps"

    def describe(self, info):
        return "the heap order of INSTRUMENT %s (MeerKAT beamformer: 256-sample runs per polarisation and channel)" % info.machine

    def layout_word(self, first_sample=0):
        return _lib.raw_at(self.layout, first_sample)


@dataclass(frozen=True)
class Guppi(Form):
    """The blocks of a GUPPI raw file: time-ordered runs per channel, `granule` = block_nsamp kept samples each."""
    layout: int = _lib.RAW_GUPPI
    name = "guppi"

    def describe(self, info):
        return "the block order of a GUPPI raw file (BACKEND %s: time-ordered runs per channel inside every block)" % info.machine

    def layout_word(self, first_sample=0):
        return _lib.guppi_at(first_sample)


@dataclass(frozen=True)
class TwoBit(Form):
    """CPSR2's two-bit real samples: whole excision windows of `granule` samples, four samples per byte and digitiser."""
    layout: int = _lib.RAW_TWOBIT
    name = "twobit"

    def describe(self, info):
        return "two-bit input (NBIT 2)"

    def refusal(self, info, instead):
        return Form.refusal(self, info, "dspsr_amd.LoadToFold folds it with -F N:D")

    def layout_word(self, first_sample=0):
        if not 0 <= first_sample < self.granule:
            raise DspsrAmdError("dspsr_amd.LoadToFold.process_block: first_sample=%d is not inside a window of %d samples"
                                % (first_sample, self.granule))
        return _lib.twobit_at(first_sample)

    def block_bytes(self, nsamp, nchan, npol, ndim, first_sample=0):
        return twobit_block_bytes(first_sample, nsamp, self.granule, npol)


@dataclass(frozen=True)
class Detected(Form):
    """Detected spectra (a SIGPROC filterbank file): a sample is one spectrum of npol * nchan values of nbit bits."""
    nbit: int = 8
    name = "detected"

    def describe(self, info):
        return "the input is detected already (STATE %s, %d channels of %d-bit values)" % (info.detected, info.nchan, info.nbit)

    def refusal(self, info, instead):
        return "%s: this driver forms its spectra from voltages; dspsr_amd.LoadToFold folds such a file" % self.describe(info)

    def block_bytes(self, nsamp, nchan, npol, ndim, first_sample=0):
        self.layout_word(first_sample)
        return nsamp * (npol * nchan * self.nbit // 8)


VOLTAGES = frozenset(("generic", "caspsr", "heaps", "guppi"))       # the 8-bit forms the convolving filterbank reads
FORMS = VOLTAGES | {"twobit", "detected"}


def raw_form(info, *, channel_sharded=False, excision_nsample=None):
    """The form of the blocks of `info` (pipeline.InputInfo): the one place that reads info.detected, info.nbit, info.guppi and
    info.machine for it.  channel_sharded: a sub-band rank reads one channel's runs of every GUPPI block (block_stride =
    chan_stride).  excision_nsample: the window of a two-bit run (default: the unpacker's)."""
    if info.detected is not None:
        return Detected(nbit=info.nbit)
    if info.nbit == 2:
        from . import twobit
        return TwoBit(granule=excision_nsample or twobit.NSAMPLE)
    if info.guppi is not None:                           # the layout comes from the file, not from the machine
        block_nsamp, chan_stride, block_stride = info.guppi
        return Guppi(granule=block_nsamp, geometry=(block_nsamp, chan_stride, chan_stride if channel_sharded else block_stride))
    if info.machine in _lib.HEAP_MACHINES:
        return Heaps(layout=_lib.HEAP_MACHINES[info.machine])
    return Caspsr() if info.machine == "CASPSR" else Form()


def refuse_forms(who, info, accepted, instead=None, own=None):
    """Plan-time refusal of a driver that has no reader for the form of `info`; returns the form where it is one of `accepted`
    (names).  instead: what the message points to -- one text, or one per form name; own: {form name: the driver's own sentence in
    place of the form's}."""
    form = raw_form(info)
    if form.name not in accepted:
        pointer = instead.get(form.name) if isinstance(instead, dict) else instead
        raise DspsrAmdError("%s: %s" % (who, (own or {}).get(form.name) or form.refusal(info, pointer)))
    return form


class InputFile:
    """What the drivers and tools use of an input file: .info (pipeline.InputInfo), .extras, .ndat, .form, and the block loop of
    dsp::IOManager -- consecutive blocks of parts_per_block overlap-save parts that share nsamp_overlap samples (the InputBuffering
    tail, Filterbank.C:443-444), each delivered as the whole units of the driver's granule that hold it.  A reader supplies
    read_units, and usable where the stream is not simply its ndat samples."""

    heaps = property(lambda self: self.form.name == "heaps")
    twobit = property(lambda self: self.form.name == "twobit")
    guppi = property(lambda self: self.form.name == "guppi")
    detected = property(lambda self: self.form.name == "detected")

    def granule(self, lt):
        """The unit the blocks of the driver `lt` are cut in: the file's own (a heap, a raw block, a sample), or, for two-bit
        samples, the excision window of the run -- the file does not know it."""
        return lt.form.granule if self.twobit else self.form.granule

    def usable(self, lt):
        """Samples the block loop reads for the driver `lt`: whole units (what follows the file's last one is dropped)."""
        return (self.ndat // self.granule(lt)) * self.granule(lt)

    def read_units(self, g0, n, channel, granule):
        """int8 host array: the contiguous bytes of `n` whole units of `granule` samples from unit g0 on (channel = g: that input
        channel's bytes alone), a view of the memory-mapped file where they lie there as they are delivered."""
        raise NotImplementedError

    def samples(self, s0, n):
        """The bytes of `n` whole samples from sample s0 on, for the forms in which a sample is a run of whole bytes."""
        raise DspsrAmdError("dspsr_amd.%s.samples: %s holds no samples of whole, consecutive bytes"
                            % (type(self).__name__, self.form.describe(self.info)))

    def nblocks(self, lt):
        """(whole blocks, parts of the ragged last block)."""
        ndat = self.usable(lt)
        if ndat < lt.nsamp_overlap + lt.nsamp_step:
            return 0, 0
        return divmod((ndat - lt.nsamp_overlap) // lt.nsamp_step, lt.cfg.parts_per_block)

    def blocks(self, lt, channel=None):
        """Yield (int8 host array, npart, first_sample) for the driver `lt` (its form, parts_per_block, nsamp_step and
        nsamp_overlap); the last block may hold fewer parts.  Samples past the last whole overlap-save part are not used (the
        reference leaves them in the input buffer at end of data).  The array holds the whole units around the block -- parts
        straddle units freely -- and the block starts at sample first_sample = (b * parts_per_block * nsamp_step) % granule of
        the first one (0 where the granule is 1).  channel = g: only input channel g's bytes, what rank g of a sub-band sharded
        run reads."""
        full, rest = self.nblocks(lt)
        ppb, step, ovl, granule = lt.cfg.parts_per_block, lt.nsamp_step, lt.nsamp_overlap, self.granule(lt)
        for b in range(full + (1 if rest else 0)):
            npart = ppb if b < full else rest
            g0, first = divmod(b * ppb * step, granule)
            yield self.read_units(g0, -(-(first + npart * step + ovl) // granule), channel, granule), npart, first


def tsamp_us(seconds):
    """A sampling interval in microseconds such that InputInfo.rate = 1e6 / tsamp_us is the reference's 1 / seconds to the bit where
    a neighbour of seconds * 1e6 gives it (the product alone may round the other way)"""
    rate, t = 1.0 / seconds, seconds * 1e6
    for c in (t, math.nextafter(t, 0.0), math.nextafter(t, math.inf)):
        if 1e6 / c == rate:
            return c
    return t


def open_input(path: str, log=None):
    """The input factory of the drivers and tools: a sigproc.SigprocFile where the file is a SIGPROC filterbank file, a
    guppi.GuppiFile where it is GUPPI raw (is_valid), else a dada.DadaFile.  The format is recognised from the file, never from
    its name."""
    from . import dada, guppi, sigproc
    if sigproc.is_valid(path):
        return sigproc.SigprocFile(path)
    if guppi.is_valid(path):
        return guppi.GuppiFile(path, log=log)
    return dada.DadaFile(path)
