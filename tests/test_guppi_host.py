"""dspsr_amd.guppi on the host: the header, every field of the observation, the start time, ndat, and the stream blocks() delivers
-- reassembled with the restatement of tests/guppi_cases.py -- for files in sequence, with missing, unordered and fractionally
skipped blocks, a first block of another size, a trailing partial block and one channel's runs; every refusal by name.  CPU only."""
import io

import numpy as np
import pytest

import guppi_cases as gc

NCHAN, NPOL, BN, OVL, PPB = 3, 2, 259, 5, 4          # packets per block 4: a PKTIDX step of 4 is in sequence


@pytest.fixture(scope="module")
def guppi():
    from dspsr_amd import guppi
    return guppi


def _samples(nblk, nchan=NCHAN, npol=NPOL, bn=BN, seed=5):
    return gc.random_samples(nchan, npol, nblk * bn, seed)


def _delivered(f, lt, nchan, npol, channel=None):
    """the samples blocks() hands to the driver `lt`: every pipeline block's new samples, and behind the last one its overlap --
    complex64 [nchan][npol][n] -- and the first of every block.  Each block's overlap must be the next block's first samples."""
    got, firsts, tail = [], [], None
    cs = f.chan_stride
    for raw, npart, first in f.blocks(lt, channel=channel):
        new = npart * lt.nsamp_step
        s = gc.stream_from_blocks(raw, nchan, npol, f.block_nsamp, f.overlap, chan_stride=cs, block_stride=cs if channel is not None else f.blocsize)
        assert s.shape[2] >= first + new + lt.nsamp_overlap and s.shape[2] - (first + new + lt.nsamp_overlap) < f.block_nsamp
        if tail is not None:
            assert np.array_equal(tail, s[:, :, first:first + lt.nsamp_overlap])
        got.append(s[:, :, first:first + new])
        tail = s[:, :, first + new:first + new + lt.nsamp_overlap]
        firsts.append(first)
    return np.concatenate(got + [tail], axis=2), firsts


def test_header_and_every_field_of_the_observation(guppi, tmp_path):
    x = _samples(4)
    path = str(tmp_path / "a.raw")
    cards = gc.write_raw(path, x, BN, OVL, packets_per_block=PPB, seq=[(k, 40 + 4 * k) for k in range(4)], cards={"FD_POLN": "CIRC", "BACKEND": "PUPPI"})
    with open(path, "rb") as fh:
        got, nbytes = guppi.read_header(fh)
    assert nbytes == 80 * (len(cards) + 1)
    assert got["BACKEND"] == "PUPPI" and got["SRC_NAME"] == "B0329+54" and int(got["BLOCSIZE"]) == NCHAN * (BN + OVL) * 4 and float(got["TBIN"]) == 2.5e-07
    assert guppi.is_valid(path)
    f = guppi.GuppiFile(path)
    i = f.info
    assert (i.machine, i.nchan, i.npol, i.ndim, i.nbit) == ("PUPPI", NCHAN, 2, 2, 8)
    assert (i.centre_frequency, i.bandwidth, i.source, i.telescope) == (820.0, -16.0, "B0329+54", "GBT")
    assert abs(i.rate - 4e6) <= 4e6 * 1e-15 and i.tsamp_us == pytest.approx(0.25, rel=1e-15)
    assert f.basis == "Circular" and f.receiver == "Rcvr_800"
    assert (f.heaps, f.twobit, f.guppi) == (False, False, True) and f.form.granule == BN and f.form.geometry == i.guppi
    assert (f.block_nsamp, f.chan_stride, f.block_stride, f.overlap) == (BN, (BN + OVL) * 4, NCHAN * (BN + OVL) * 4, OVL)
    assert i.guppi == (f.block_nsamp, f.chan_stride, f.block_stride)
    # the start time, worked by hand: PKTSIZE = 259 * 4 * 3 / 4 = 777 bytes; 40 packets = 31080 bytes = 248640 bits;
    # one sample of all channels and polarisations is 8 * 3 * 2 * 2 = 96 bits -> 2590 samples (ten blocks) of 0.25 us = 647.5 us
    assert cards["PKTSIZE"] == 777
    assert i.mjd_day == 55555 and i.start_seconds == 0.0
    assert i.mjd_sec == pytest.approx(43200 + 0.25 + 647.5e-6, rel=0, abs=1e-9)
    assert f.ndat == 4 * BN
    # one polarisation, linear basis
    x1 = _samples(2, npol=1)
    gc.write_raw(path, x1, BN, OVL, packets_per_block=1)
    f1 = guppi.GuppiFile(path)
    assert f1.info.npol == 1 and f1.basis == "Linear" and f1.chan_stride == (BN + OVL) * 2 and f1.ndat == 2 * BN


def test_is_valid_tells_the_formats_apart(guppi, tmp_path):
    from dspsr_amd import dada, synth
    d = str(tmp_path / "x.dada")
    with open(d, "wb") as fh:
        fh.write(synth.dada_header(1382.0, -16.0, 4, 2, 2, 0.25) + bytes(8192))
    r = str(tmp_path / "x.raw")
    gc.write_raw(r, _samples(2), BN, OVL, packets_per_block=PPB)
    assert dada.is_valid(d) and not guppi.is_valid(d)
    assert guppi.is_valid(r) and not dada.is_valid(r)
    assert isinstance(guppi.open_input(d), dada.DadaFile) and isinstance(guppi.open_input(r), guppi.GuppiFile)
    assert not guppi.is_valid(str(tmp_path / "absent.raw"))
    cards, n = guppi.read_header(io.BytesIO(b"X" * 400))
    assert cards is None and n == 0


# what the file holds -> what is delivered.  seq: (stream block of x | None, PKTIDX); want: stream blocks of x, None = zeros
CASES = {
    "in sequence": ([(k, 4 * k) for k in range(6)], [0, 1, 2, 3, 4, 5], ""),
    # nblocks = 5 from the file size: the zeros lengthen the stream, its tail (block 5) falls off
    "one missing block": ([(0, 0), (1, 4), (3, 12), (4, 16), (5, 20)], [0, 1, None, 3, 4], "skipped pktidx=12 last=4 diff=8 inc=4"),
    "two missing blocks": ([(0, 0), (3, 12), (4, 16), (5, 20)], [0, None, None, 3], "skipped pktidx=12 last=0 diff=12 inc=4"),
    # the block with the older PKTIDX is skipped; nothing takes its place: the stream is shorter than ndat
    "out of order": ([(0, 0), (1, 4), (5, 0), (2, 8), (3, 12)], [0, 1, 2, 3], "unordered pktidx=0 last=4 diff=-4 inc=4"),
    "fractional gap": ([(0, 0), (1, 4), (3, 10), (4, 14)], [0, 1, 3, 4], "WARNING fraction skipped block"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_stream_of_a_file(guppi, tmp_path, case):
    seq, want, line = CASES[case]
    x = _samples(6)
    path = str(tmp_path / "s.raw")
    gc.write_raw(path, x, BN, OVL, seq=seq, packets_per_block=PPB)
    log = io.StringIO()
    f = guppi.GuppiFile(path, log=log)
    assert f.packets_per_block == PPB
    assert f.ndat == len(seq) * BN                                   # nblocks from the file size
    assert line in log.getvalue() and (line or log.getvalue() == "")
    if case == "fractional gap":
        assert "skipped pktidx=10 last=4 diff=6 inc=4" in log.getvalue()
    cx = gc.complex_of(x)
    exp = np.concatenate([np.zeros((NCHAN, NPOL, BN), np.complex64) if k is None else cx[:, :, k * BN:(k + 1) * BN] for k in want], axis=2)
    got = gc.stream_of_file(f, NCHAN, NPOL)
    assert got.shape == exp.shape and np.array_equal(got, exp)
    assert f.usable() == min(f.ndat, len(want) * BN)
    # through blocks(): parts of 100 samples and 37 behind them, 3 parts per pipeline block
    lt = gc.Driver(3, 100, 37, f.form)
    full, rest = f.nblocks(lt)
    nparts = (len(want) * BN - 37) // 100
    assert (full, rest) == divmod(nparts, 3)
    got, firsts = _delivered(f, lt, NCHAN, NPOL)
    assert np.array_equal(got, exp[:, :, :nparts * 100 + 37])
    assert firsts == [(b * 300) % BN for b in range(len(firsts))]


def test_first_block_of_another_size_is_skipped(guppi, tmp_path):
    x = _samples(4)
    path = str(tmp_path / "l.raw")
    lead_cards = dict(gc.CARDS, OBSNCHAN=NCHAN, NPOL=4, OVERLAP=OVL, BLOCSIZE=NCHAN * 100 * 4, PKTSIZE=777, PKTIDX=0)
    gc.write_raw(path, x, BN, OVL, packets_per_block=PPB, seq=[(k, 100 + 4 * k) for k in range(4)], lead=(lead_cards, gc.random_blocks(NCHAN * 400, 9)))
    f = guppi.GuppiFile(path)
    assert f.pos0 == 80 * (len(lead_cards) + 1) + NCHAN * 400 and f.pktidx0 == 100
    assert f.blocsize == NCHAN * (BN + OVL) * 4 and f.ndat == 4 * BN
    assert np.array_equal(gc.stream_of_file(f, NCHAN, NPOL), gc.complex_of(x))


def test_trailing_partial_block_is_dropped(guppi, tmp_path):
    x = _samples(3)
    path = str(tmp_path / "t.raw")
    cards = gc.write_raw(path, x, BN, OVL, packets_per_block=PPB, seq=[(k, 4 * k) for k in range(3)])
    with open(path, "ab") as fh:
        fh.write(gc.header(dict(cards, PKTIDX=12)) + bytes(1000))
    f = guppi.GuppiFile(path)
    assert f.ndat == 3 * BN and len(f.stream) == 3
    assert np.array_equal(gc.stream_of_file(f, NCHAN, NPOL), gc.complex_of(x))


def test_pipeline_blocks_start_everywhere_and_one_channels_runs(guppi, tmp_path):
    """pipeline blocks that start at sample 0, inside a GUPPI block and on a block's last sample; channel = g"""
    bn, ovl = 255, 2
    x = _samples(5, bn=bn)
    path = str(tmp_path / "c.raw")
    gc.write_raw(path, x, bn, ovl, packets_per_block=PPB)
    f = guppi.GuppiFile(path)
    cx = gc.complex_of(x)
    lt = gc.Driver(2, 127, 40, f.form)                     # pipeline blocks start at 0, 254 (the last sample of block 0), 508, 762
    got, firsts = _delivered(f, lt, NCHAN, NPOL)
    assert firsts[:3] == [0, bn - 1, 253] and 0 in firsts and bn - 1 in firsts and any(0 < v < bn - 1 for v in firsts)
    nparts = (5 * bn - 40) // 127
    assert np.array_equal(got, cx[:, :, :nparts * 127 + 40])
    for g in range(NCHAN):
        raws = list(f.blocks(lt, channel=g))
        assert all(r.size == -(-(first + n * 127 + 40) // bn) * f.chan_stride for r, n, first in raws)
        got_g, firsts_g = _delivered(f, lt, 1, NPOL, channel=g)
        assert firsts_g == firsts and np.array_equal(got_g[0], got[g])
    with pytest.raises(Exception, match="channel=3"):
        list(f.blocks(lt, channel=3))


REFUSALS = [
    (dict(cards={"NBITS": 2}), "NBITS=2"),
    (dict(cards={"NBITS": 4}), "GUPPIFourBit"),
    (dict(cards={"PKTFMT": "VDIF"}), "VDIF"),
    (dict(cards={"PKTFMT": "SIMPLE"}), "SIMPLE"),
    (dict(cards={"OBSNCHAN": 1}), "OBSNCHAN 1"),
    (dict(cards={"BACKEND": "VEGAS"}), "BACKEND VEGAS"),
    (dict(cards={"DIRECTIO": 1}), "DIRECTIO"),
    (dict(cards={"BLOCSIZE": NCHAN * (BN + OVL) * 4 + 2}), "BLOCSIZE"),
    (dict(cards={"OVERLAP": BN + OVL}), "OVERLAP"),
] + [(dict(drop=(key,)), key) for key in ("NBITS", "OBSBW", "OBSFREQ", "OBSNCHAN", "NPOL", "PKTFMT", "PKTSIZE", "TBIN", "OVERLAP", "STT_IMJD", "STT_SMJD",
                                          "STT_OFFS", "TELESCOP", "SRC_NAME", "BACKEND", "FD_POLN", "RA_STR", "DEC_STR", "FRONTEND")]


@pytest.mark.parametrize("how,word", REFUSALS, ids=[w for _h, w in REFUSALS])
def test_refusals_at_open_name_what_is_not_built(guppi, tmp_path, how, word):
    from dspsr_amd import DspsrAmdError
    path = str(tmp_path / "r.raw")
    x = _samples(2)
    if how.get("cards", {}).get("BLOCSIZE"):
        # data sections of the odd size, so that the second header is where the first says
        n = how["cards"]["BLOCSIZE"]
        base = dict(gc.CARDS, OBSNCHAN=NCHAN, NPOL=4, OVERLAP=OVL, BLOCSIZE=n, PKTSIZE=777)
        with open(path, "wb") as fh:
            for k in range(2):
                fh.write(gc.header(dict(base, PKTIDX=4 * k)) + bytes(n))
    else:
        gc.write_raw(path, x, BN, OVL, packets_per_block=PPB, **how)
    with pytest.raises(DspsrAmdError, match=word.replace("+", r"\+")):
        guppi.GuppiFile(path)


def test_directio_zero_is_read_and_one_header_is_refused(guppi, tmp_path):
    from dspsr_amd import DspsrAmdError
    path = str(tmp_path / "d.raw")
    x = _samples(2)
    gc.write_raw(path, x, BN, OVL, packets_per_block=PPB, cards={"DIRECTIO": 0})
    assert guppi.GuppiFile(path).ndat == 2 * BN
    gc.write_raw(path, x, BN, OVL, packets_per_block=PPB, seq=[(0, 0)])
    assert guppi.is_valid(path)
    with pytest.raises(DspsrAmdError, match="Error parsing block1 header"):
        guppi.GuppiFile(path)


def test_drivers_without_a_reader_refuse_the_format_by_name(guppi, tmp_path):
    """-R (integrate_raw), LoadToFil and LoadToFilDirect read raw bytes themselves: refused at plan time, no device opened"""
    from dspsr_amd import DspsrAmdError, pipeline
    path = str(tmp_path / "p.raw")
    gc.write_raw(path, _samples(2, nchan=4), BN, OVL, packets_per_block=PPB)
    info = guppi.GuppiFile(path).info
    with pytest.raises(DspsrAmdError, match="LoadToFilDirect.*GUPPI raw file"):
        pipeline.LoadToFilDirect(pipeline.SearchConfig(nchan=4, tscrunch=4, nbit=8), info, device=None)
    with pytest.raises(DspsrAmdError, match="LoadToFil:.*GUPPI raw file"):
        pipeline.LoadToFil(pipeline.SearchConfig(nchan=16, tscrunch=4, nbit=8), info, device=None)
    with pytest.raises(DspsrAmdError, match=r"\(-R\).*GUPPI raw file"):
        pipeline.rfi_check(pipeline.Config(nchan=4, dispersion_measure=10.0, folding_period=0.004, zap_rfi=True), info)
