"""dspsr_amd.inputs on the host: every form of input through the one block loop (InputFile.blocks) and the one size of a block
(Form.block_bytes), on small files written by the case helpers of the formats; and every driver's refusal of the forms it does not
read, in the words the tests of the formats match.

A stand-in driver cuts each file into blocks of 3 parts.  Its part step and overlap are chosen against the form's granule G (the
heap of 256 samples, a GUPPI raw block of 64, an excision window of 32, 1 elsewhere) so that block 0 starts at first = 0, block 1 at
first = G - 1 and straddles three units, and the last block is ragged."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guppi_cases as gc                                                            # noqa: E402
import heap_cases as hc                                                             # noqa: E402
import sigproc_cases as sc                                                          # noqa: E402
from dspsr_amd import DspsrAmdError, dada, guppi, inputs, pipeline, sigproc, synth  # noqa: E402

NDAT, NCHAN, NPOL, OVERLAP = 1216, 4, 2, 20          # (1216 - 20) // 21 = 56 parts and (2304 - 20) // 85 = 26: two parts in the last block
BN, GUPPI_OVERLAP, WINDOW = 64, 8, 32


def _codes(raw, npol):
    """two-bit codes [npol][4 * nbyte] of bytes interleaved by digitiser, the first sample in the top bits of a byte"""
    b = np.asarray(raw).view(np.uint8).reshape(-1, npol)
    return ((b[:, :, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).transpose(1, 0, 2).reshape(npol, -1)


def _generic(tmp_path, channel):
    data = np.random.default_rng(1).integers(-128, 128, (NDAT, NCHAN, NPOL, 2), dtype=np.int8)
    p = tmp_path / "g.dada"
    p.write_bytes(synth.dada_header(1400.0, 32.0, NCHAN, NPOL, 2, 0.0625) + data.tobytes() + b"\x01\x02\x03")
    return dada.DadaFile(str(p)), data.transpose(1, 2, 3, 0), lambda raw, nchan: raw.reshape(-1, nchan, NPOL, 2).transpose(1, 2, 3, 0), 1


def _heaps(tmp_path, channel, machine="MKBFRo"):
    block = hc.random_block(9, NCHAN, NPOL, seed=3)
    f = dada.DadaFile(hc.write_dada(tmp_path / "h.dada", np.concatenate([block, np.zeros(100, np.int8)]), machine=machine, nchan=NCHAN, npol=NPOL))
    decode = lambda raw, nchan: np.moveaxis(hc.stream_from_heaps(raw, nchan, NPOL, hc.MACHINES[machine]), 2, -1)
    return f, decode(block, NCHAN), decode, hc.HEAP


def _guppi(tmp_path, channel):
    x = gc.random_samples(NCHAN, NPOL, NDAT, seed=4)
    path = str(tmp_path / "r.raw")
    gc.write_raw(path, x, BN, GUPPI_OVERLAP)
    f = guppi.GuppiFile(path)
    strides = dict(chan_stride=f.chan_stride, block_stride=f.chan_stride if channel is not None else f.blocsize)
    return f, gc.complex_of(x), lambda raw, nchan: gc.stream_from_blocks(raw, nchan, NPOL, BN, GUPPI_OVERLAP, **strides), BN


def _twobit(tmp_path, channel):
    data = np.random.default_rng(5).integers(0, 256, NDAT // 4 * NPOL + 7, dtype=np.uint8)          # (seven bytes short of a window more)
    p = tmp_path / "t.dada"
    p.write_bytes(synth.dada_header(1400.0, 16.0, 1, NPOL, 1, 1.0 / 32.0, instrument="CPSR2").replace(b"NBIT 8", b"NBIT 2") + data.tobytes())
    return dada.DadaFile(str(p)), _codes(data[:NDAT // 4 * NPOL], NPOL), lambda raw, nchan: _codes(raw, NPOL), WINDOW


def _detected(tmp_path, channel, nbit=4):
    S = sc.spectrum_bytes(nbit, NCHAN, NPOL)
    data = sc.random_spectra(nbit, NCHAN, NPOL, NDAT)
    path = str(tmp_path / "d.fil")
    sc.write_fil(path, np.concatenate([data, np.zeros(S - 1, np.uint8)]), nbits=nbit, nchans=NCHAN, nifs=NPOL)
    return sigproc.SigprocFile(path), data.reshape(NDAT, S).T, lambda raw, nchan: np.asarray(raw).view(np.uint8).reshape(-1, S).T, 1


CASES = {"generic": (_generic, None), "generic_channel": (_generic, 2), "heaps": (_heaps, None), "heaps_subband": (_heaps, 1),
         "guppi": (_guppi, None), "guppi_subband": (_guppi, 1), "twobit": (_twobit, None), "detected": (_detected, None)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_blocks_of_every_form(tmp_path, case):
    """first == s0 % granule, len(array) == form.block_bytes(...), and the kept samples of the blocks are the stream written: time is
    the last axis of what `decode` returns, for the file's stream and for a block alike.  GUPPI raw blocks: the array holds whole data
    sections, as it always has, and block_bytes counts to the last kept sample (what process_block needs): the difference is the
    unused end of the last section, to the byte."""
    write, channel = CASES[case]
    f, stream, decode, granule = write(tmp_path, channel)
    info = f.info
    form = inputs.raw_form(info, channel_sharded=channel is not None, excision_nsample=WINDOW)
    assert form.granule == granule and form.name == case.split("_")[0] == f.form.name
    step = 85 if granule == hc.HEAP else 21                                # 3 * step = G - 1 (mod G): 255, and 63 = 31 (mod 32)
    lt = SimpleNamespace(cfg=SimpleNamespace(parts_per_block=3), nsamp_step=step, nsamp_overlap=OVERLAP, form=form)
    nchan = info.nchan if channel is None else 1
    if channel is not None:
        stream = stream[channel:channel + 1]
    usable = f.usable(lt)
    assert usable == (f.ndat // granule) * granule == stream.shape[-1]
    full, rest = f.nblocks(lt)
    assert (full, rest) == divmod((usable - OVERLAP) // step, 3) and full >= 3 and rest, "a ragged last block"
    got, firsts, units = [], [], []
    for b, (raw, npart, first) in enumerate(f.blocks(lt, channel=channel)):
        s0, nsamp = b * 3 * step, npart * step + OVERLAP
        assert npart == (3 if b < full else rest) and first == s0 % granule
        need = form.block_bytes(nsamp, nchan, info.npol, info.ndim, first)
        if form.name == "guppi":
            # the reader delivers whole data sections; the block ends with the last kept sample of the last section's last run
            section = f.chan_stride if channel is not None else f.blocsize
            need += section - ((nchan - 1) * f.chan_stride + BN * 2 * info.npol)
        assert raw.dtype == np.int8 and len(raw) == need
        mine = decode(raw, nchan)[..., first:first + nsamp]
        assert np.array_equal(mine, stream[..., s0:s0 + nsamp])
        got.append(mine[..., :npart * step] if b < full else mine)        # the new samples; behind the last block its overlap
        firsts.append(first)
        units.append(-(-(first + nsamp) // granule))
    assert len(got) == full + 1 and firsts[0] == 0 and firsts[1] == granule - 1 and units[1] >= 3
    nparts = 3 * full + rest
    assert np.array_equal(np.concatenate(got, axis=-1), stream[..., :nparts * step + OVERLAP])
    # whole samples byte by byte: the forms that have them
    if form.name in ("generic", "detected"):
        assert np.array_equal(decode(f.samples(5, 7), info.nchan), decode(f.samples(0, 12), info.nchan)[..., 5:])
    else:
        with pytest.raises(DspsrAmdError, match=r"\.samples: "):
            f.samples(0, 1)


def test_layout_words_and_their_range():
    from dspsr_amd import _lib
    info = lambda **kw: pipeline.InputInfo(**dict(dict(nchan=NCHAN, npol=NPOL, ndim=2, machine="DADA"), **kw))
    assert inputs.raw_form(info()).layout_word() == _lib.RAW_GENERIC and inputs.raw_form(info(machine="CASPSR")).layout_word() == _lib.RAW_CASPSR
    for machine, layout in _lib.HEAP_MACHINES.items():
        assert inputs.raw_form(info(machine=machine)).layout_word(255) == _lib.raw_at(layout, 255)
    g = inputs.raw_form(info(guppi=(BN, 288, 1152)), channel_sharded=True)
    assert g.geometry == (BN, 288, 288) and g.layout_word(63) == _lib.guppi_at(63)
    t = inputs.raw_form(info(nbit=2, machine="CPSR2"), excision_nsample=WINDOW)
    assert t.layout_word(31) == _lib.twobit_at(31) and inputs.raw_form(info(nbit=2)).granule == 512
    assert inputs.raw_form(info(nbit=2, detected="PPQQ")).name == "detected"       # (two-bit detected values are not two-bit voltages)
    for form, first in ((inputs.raw_form(info()), 1), (inputs.raw_form(info(machine="MKBF")), 256), (g, -1), (t, WINDOW),
                        (inputs.raw_form(info(detected="PPQQ")), 1)):
        with pytest.raises((DspsrAmdError, ValueError), match="first_sample"):
            form.layout_word(first)


# what each driver refuses, by the pattern the tests of the formats match (test_heap_host, test_guppi_host, test_twobit_host,
# test_sigproc_host, test_pipeline_construction_host); LoadToFold reads every form
HEAPS, GUPPI = r"INSTRUMENT MKBF", r"GUPPI raw file"
TWOBIT, DETECTED, CASPSR = r"two-bit input", r"the input is detected already", r"the CASPSR byte order is not built on this path"
REFUSED = {
    "LoadToFil": dict(heaps="LoadToFil:.*" + HEAPS, guppi="LoadToFil:.*" + GUPPI, twobit=TWOBIT, detected="LoadToFil:.*" + DETECTED),
    "LoadToFilCoherent": dict(twobit=TWOBIT, detected="LoadToFilCoherent:.*" + DETECTED),
    "LoadToFilDirect": dict(caspsr="LoadToFilDirect: " + CASPSR, heaps="LoadToFilDirect.*" + HEAPS, guppi="LoadToFilDirect.*" + GUPPI, twobit=TWOBIT,
                            detected="LoadToFilDirect:.*" + DETECTED),
    "LoadToFITS": dict(twobit=TWOBIT, detected="LoadToFITS: detected input"),
}
CHANS = dict(centre_frequency=1400.0, bandwidth=-8.0, nchan=8, npol=2, ndim=2, tsamp_us=1.0)
INFOS = dict(caspsr=dict(CHANS, machine="CASPSR"), heaps=dict(CHANS, machine="MKBF"), guppi=dict(CHANS, machine="GUPPI", guppi=(BN, 288, 2304)),
             twobit=dict(CHANS, nchan=1, ndim=1, machine="CPSR2", nbit=2), detected=dict(CHANS, ndim=1, machine="FAKE", detected="PPQQ"))


@pytest.mark.parametrize("driver,form", [(d, f) for d in sorted(REFUSED) for f in sorted(REFUSED[d])])
def test_a_driver_refuses_the_forms_it_does_not_read(driver, form):
    info = pipeline.InputInfo(**INFOS[form])
    assert inputs.raw_form(info).name == form
    cfg = pipeline.FitsConfig() if driver == "LoadToFITS" else pipeline.SearchConfig(nchan=16, tscrunch=4, nbit=8)
    with pytest.raises(DspsrAmdError, match=REFUSED[driver][form]):
        getattr(pipeline, driver)(cfg, info, device=None)
