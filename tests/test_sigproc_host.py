"""dspsr_amd.sigproc on the host: the header reader against the fixture the reference's own writer produced, against
write_sigproc_header for every sample size and number of polarisations, and -- where oracle/_ref/libsigproc_ref.so is built --
against the reference's read_header on the same bytes; every field of the observation; ndat from the file size; blocks(); every
refusal of the reader and of the detected back end by its message, with no device opened; the restatement of the unpacker against
the oracle's digitiser, its inverse; the case table of the kernel test.  CPU only."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import sigproc_cases as sc

ROOT = sc.ROOT
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "libsigproc_ref.so")


@pytest.fixture(scope="module")
def sigproc():
    from dspsr_amd import sigproc
    return sigproc


def _string(s):
    return struct.pack("<i", len(s)) + s.encode("ascii")


def _header(items):
    """a header from (keyword, value) pairs: int -> int32, float -> float64, str -> the next string, bytes -> as they are"""
    b = _string("HEADER_START")
    for key, v in items:
        b += _string(key)
        b += struct.pack("<i", v) if isinstance(v, int) else struct.pack("<d", v) if isinstance(v, float) else v if isinstance(v, bytes) else _string(v)
    return b + _string("HEADER_END")


def _file(tmp_path, items, nbytes=0, name="a.fil"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(_header(items) + bytes(nbytes))
    return path


BASE = [("nchans", 16), ("nbits", 8), ("nifs", 1), ("tsamp", 64e-6), ("fch1", 1500.0), ("foff", -0.5), ("tstart", 56000.25)]


def _with(**over):
    return [(k, over.pop(k) if k in over else v) for k, v in BASE] + list(over.items())


def test_reads_the_header_the_reference_wrote(sigproc):
    want = json.load(open(os.path.join(GOLD, "sigproc_header.json")))
    path = os.path.join(GOLD, "sigproc_header.bin")
    assert sigproc.is_valid(path)
    got, nbytes = sigproc.read_header(path)
    assert nbytes == os.path.getsize(path)
    want["tstart"] = want.pop("tstart_mjd")
    for key, v in want.items():
        assert got[key] == v and type(got[key]) is type(v), key
    assert (got["az_start"], got["za_start"], got["data_type"], got["nbeams"], got["ibeam"]) == (0.0, 0.0, 1, 0, 0)
    f = sigproc.SigprocFile(path)
    i = f.info
    assert (i.nchan, i.npol, i.ndim, i.nbit, i.detected) == (4096, 1, 1, 8, "Intensity")
    assert i.centre_frequency == 1581.951171875 + 0.5 * (-0.09765625 * 4095) and i.bandwidth == -0.09765625 * 4096
    assert i.rate == 1.0 / 0.00016384 and (i.source, i.telescope, i.machine) == ("J0835-4510", "Fake", "FAKE")
    assert i.mjd_day == 55299 and abs(i.mjd_sec - 0.087326388886 * 86400.0) < 1e-5
    assert f.ndat == 0 and f.header_bytes == nbytes and list(f.blocks(_Driver(8))) == []


class _Driver:
    """what blocks() / nblocks() read of a driver"""

    def __init__(self, parts_per_block):
        from dspsr_amd import inputs, pipeline
        self.cfg = pipeline.Config(parts_per_block=parts_per_block)
        self.nsamp_step, self.nsamp_overlap, self.form = 1, 0, inputs.Detected()


@pytest.mark.parametrize("nifs", [1, 2, 4])
@pytest.mark.parametrize("nbit", sc.NBITS)
def test_round_trips_the_writer(sigproc, tmp_path, nbit, nifs):
    path = str(tmp_path / "w.fil")
    values = dict(source_name="B1937+21", rawdatafile="obs.dada", machine_id=10, telescope_id=4, src_raj=193938.56, src_dej=213459.1,
                  fch1=1500.25, foff=-0.5, nchans=24, nbits=nbit, tstart_mjd=60000.75, tsamp=6.4e-5, nifs=nifs)
    S, ndat = sc.spectrum_bytes(nbit, 24, nifs), 11
    nhead = sc.write_fil(path, np.zeros(ndat * S + S - 1, np.uint8), **values)           # (a last spectrum one byte short)
    assert sigproc.is_valid(path)
    got, nbytes = sigproc.read_header(path)
    assert nbytes == nhead
    values["tstart"] = values.pop("tstart_mjd")
    assert {k: got[k] for k in values} == values
    f = sigproc.SigprocFile(path)
    i = f.info
    assert f.ndat == ndat and f.spectrum_bytes == S and f.header_bytes == nhead
    assert (i.nchan, i.npol, i.ndim, i.nbit) == (24, nifs, 1, nbit) and i.detected == {1: "Intensity", 2: "PPQQ", 4: "Coherence"}[nifs]
    assert i.centre_frequency == 1500.25 + 0.5 * (-0.5 * 23) and i.bandwidth == -12.0 and i.rate == 1.0 / 6.4e-5
    assert (i.machine, i.telescope, i.source) == ("BPSR", "Parkes", "B1937+21")
    assert i.mjd_day == 60000 and i.mjd_sec == 0.75 * 86400.0 and i.start_seconds == 0.0
    assert (f.heaps, f.twobit, f.guppi, f.detected) == (False, False, False, True) and (f.form.nbit, f.form.granule) == (nbit, 1)
    from dspsr_amd import guppi, inputs
    assert isinstance(guppi.open_input(path), sigproc.SigprocFile) and guppi.open_input is inputs.open_input


def test_id_tables(sigproc):
    """SigProcObservation.C:69-175"""
    assert [sigproc.telescope_name(k) for k in (0, 1, 4, 6, 8, 9, 11, 12, 99)] == ["Fake", "Arecibo", "Parkes", "GBT", "Effelsberg", "unknown", "LOFAR", "VLA", "unknown"]
    assert [sigproc.machine_name(k, 0) for k in (0, 1, 2, 7, 8, 9, 10, 11, 12)] == ["FAKE", "PSPM", "WAPP", "GMRTFB", "PULSAR2000", "?????", "ARTEMIS", "COBALT", "?????"]
    assert sigproc.machine_name(10, 4) == "BPSR"


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/libsigproc_ref.so is not built")
@pytest.mark.parametrize("nbit,nifs", [(1, 1), (2, 2), (8, 4), (32, 1)])
def test_the_reference_read_header_agrees(sigproc, tmp_path, nbit, nifs):
    """the reference's read_header (sigproc/read_header.c, compiled as it is) on the same bytes: the same globals, the same length"""
    path = str(tmp_path / "r.fil")
    sc.write_fil(path, np.zeros(7, np.uint8), nbits=nbit, nchans=40, nifs=nifs, source_name="J1234-5678", rawdatafile="x.raw", machine_id=2,
                 telescope_id=1, src_raj=123456.7, src_dej=-567800.1, fch1=1400.5, foff=-0.25, tstart_mjd=58000.125, tsamp=1e-4)
    got, nbytes = sigproc.read_header(path)
    lib, libc = C.CDLL(REF), C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    lib.read_header.argtypes = [C.c_void_p]
    fp = libc.fopen(path.encode(), b"rb")
    try:
        assert lib.read_header(fp) == nbytes
    finally:
        libc.fclose(fp)
    for key in ("nchans", "nbits", "nifs", "machine_id", "telescope_id", "data_type", "nbeams", "ibeam"):
        assert C.c_int.in_dll(lib, key).value == got[key], key
    for key in ("tsamp", "tstart", "fch1", "foff", "src_raj", "src_dej", "az_start", "za_start"):
        assert C.c_double.in_dll(lib, key).value == got[key], key
    assert (C.c_char * 80).in_dll(lib, "source_name").value.decode() == got["source_name"]
    assert (C.c_char * 80).in_dll(lib, "rawdatafile").value.decode() == got["rawdatafile"]


def test_every_keyword_and_its_size(sigproc, tmp_path):
    """read_header.c:50-125: int32, float64, the two strings; npuls is a long int and `signed` a char (header.h) -- read and ignored"""
    items = _with(telescope_id=6, machine_id=11, data_type=1, ibeam=3, nbeams=13, barycentric=1, pulsarcentric=0, nbins=5, nsamples=99,
                  az_start=1.5, za_start=2.5, src_raj=1.0, src_dej=-2.0, period=0.5, refdm=26.75)
    items = items + [("npuls", struct.pack("<q", 1 << 40)), ("signed", struct.pack("<b", 1)), ("source_name", "PSR X"), ("rawdatafile", "f.raw")]
    path = _file(tmp_path, items, nbytes=3 * 16 + 5)
    got, nbytes = sigproc.read_header(path)
    assert nbytes == len(_header(items))
    assert got["npuls"] == 1 << 40 and got["signed"] == 1 and got["refdm"] == 26.75 and got["nsamples"] == 99 and got["ibeam"] == 3
    f = sigproc.SigprocFile(path)
    assert f.ndat == 3 and f.extras["dm"] == 26.75 and f.info.source == "PSR X" and (f.info.telescope, f.info.machine) == ("GBT", "COBALT")
    # the unpacker ignores `signed`: the same observation without the key
    g = sigproc.SigprocFile(_file(tmp_path, [kv for kv in items if kv[0] != "signed"], nbytes=3 * 16 + 5, name="b.fil"))
    assert g.info == f.info and g.ndat == f.ndat


@pytest.mark.parametrize("nbit", sc.NBITS)
def test_ndat_and_blocks(sigproc, tmp_path, nbit):
    """ndat = (file size - header) * 8 / (nbits * nifs * nchans) rounded down; blocks() yields the whole spectra as they lie in the
    file, in runs of parts_per_block, no overlap"""
    nchan, nifs, ndat = 40, 2, 23
    S = sc.spectrum_bytes(nbit, nchan, nifs)
    data = sc.random_spectra(nbit, nchan, nifs, ndat)
    path = str(tmp_path / "d.fil")
    for extra in (0, 1, S - 1):                                                          # a truncated last spectrum is dropped
        sc.write_fil(path, np.concatenate([data, np.zeros(extra, np.uint8)]), nbits=nbit, nchans=nchan, nifs=nifs)
        f = sigproc.SigprocFile(path)
        assert f.ndat == ndat == (os.path.getsize(path) - f.header_bytes) * 8 // (nbit * nifs * nchan)
        lt = _Driver(8)
        assert f.nblocks(lt) == (2, 7) and f.usable(lt) == ndat
        got = list(f.blocks(lt))
        assert [n for _b, n, _f in got] == [8, 8, 7] and all(b.dtype == np.int8 and b.size == n * S and first == 0 for b, n, first in got)
        assert np.array_equal(np.concatenate([b for b, _n, _f in got]).view(np.uint8), data)
    with pytest.raises(Exception, match="channel"):
        list(f.blocks(lt, channel=0))


def test_reader_refusals(sigproc, tmp_path):
    from dspsr_amd import DspsrAmdError, dada
    p = str(tmp_path / "x.dada")
    open(p, "wb").write(b"HDR_VERSION 1.0\n" + bytes(4080))
    assert not sigproc.is_valid(p) and not sigproc.is_valid(str(tmp_path / "missing"))
    with pytest.raises(DspsrAmdError, match="HEADER_START"):
        sigproc.read_header(p)
    with pytest.raises(DspsrAmdError, match="unknown parameter: nchan$"):
        sigproc.SigprocFile(_file(tmp_path, _with(nchan=4)))
    for key in ("FREQUENCY_START", "fchannel"):
        with pytest.raises(DspsrAmdError, match="frequency table \\(%s\\)" % key):
            sigproc.SigprocFile(_file(tmp_path, BASE + [(key, b"")]))
    open(p, "wb").write(_header(BASE)[:-14])
    with pytest.raises(DspsrAmdError, match="ends before HEADER_END"):
        sigproc.read_header(p)
    for bad in (0, 3, 5, 12, 24, 64):
        with pytest.raises(DspsrAmdError, match="nbits=%d; dsp::SigProcUnpacker matches" % bad):
            sigproc.SigprocFile(_file(tmp_path, _with(nbits=bad)))
    for nbit, nchan in ((1, 4), (1, 12), (2, 6), (4, 3)):
        with pytest.raises(DspsrAmdError, match=r"nchans=%d of nbits=%d do not fill whole bytes.*SigProcUnpacker.C:90,107-110" % (nchan, nbit)):
            sigproc.SigprocFile(_file(tmp_path, _with(nbits=nbit, nchans=nchan)))
    for bad in (0, 3, 8):
        with pytest.raises(DspsrAmdError, match="nifs=%d" % bad):
            sigproc.SigprocFile(_file(tmp_path, _with(nifs=bad)))
    for bad in (0.0, -1e-4):
        with pytest.raises(DspsrAmdError, match="tsamp=.* is not positive"):
            sigproc.SigprocFile(_file(tmp_path, _with(tsamp=bad)))
    for bad in (0, -2):
        with pytest.raises(DspsrAmdError, match="nchans=%d" % bad):
            sigproc.SigprocFile(_file(tmp_path, _with(nchans=bad)))
    with pytest.raises(DspsrAmdError, match="has no tsamp"):
        sigproc.SigprocFile(_file(tmp_path, [kv for kv in BASE if kv[0] != "tsamp"]))
    # a file with no whole spectrum opens; fold_file plans the run from its header before it opens a device
    from dspsr_amd import pipeline
    assert sigproc.SigprocFile(_file(tmp_path, BASE, nbytes=15)).ndat == 0
    with pytest.raises(DspsrAmdError, match="no polynomial and no period"):
        dada.fold_file(_file(tmp_path, BASE, nbytes=15), pipeline.Config(nchan=16))


def _info(sigproc, tmp_path, **over):
    return sigproc.SigprocFile(_file(tmp_path, _with(**over), nbytes=64)).info


def test_back_end_refusals_open_no_device(sigproc, tmp_path, monkeypatch):
    """every refusal of the detected back end by its message, with the option's spelling; pipeline.Context is replaced by a trap:
    nothing may reach for a device"""
    from dspsr_amd import DspsrAmdError, pipeline

    def trap(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(pipeline, "Context", trap)
    info = _info(sigproc, tmp_path, nifs=2)
    ok = dict(nchan=16, folding_period=0.01, nbin=16)
    for over, words in ((dict(nchan=32), r"nchan=32 \(-F 32\) asks for a filterbank, the file holds 16 channels"),
                        (dict(nchan=8), r"-F 8"),
                        (dict(cyclic_nchan=4), r"-cyclic"), (dict(plfb_nbin=8), r"-G"), (dict(fourth_moment=True), r"-4"),
                        (dict(sk_zap=True), r"-skz"), (dict(zap_rfi=True), r"-R"), (dict(calibrator="cal.npz"), r"-pac"),
                        (dict(npol=1), r"npol=1 \(-d 1\) asks for another state than the file's 2 polarisations"),
                        (dict(npol=3), r"-d 3")):
        with pytest.raises(DspsrAmdError, match=r"detected input \(STATE PPQQ\).*" + words):
            pipeline.LoadToFold(pipeline.Config(**dict(ok, **over)), info)
    for tap in ("Detection", "Fold"):
        with pytest.raises(DspsrAmdError, match=r"detected input.*--dump %s" % tap):
            pipeline.LoadToFold(pipeline.Config(**ok), info, dump_before=(tap,))
    with pytest.raises(DspsrAmdError, match=r"detected input.*sub-band sharded runs \(subband=1\)"):
        pipeline.LoadToFold(pipeline.Config(**ok), info, subband=1)
    with pytest.raises(DspsrAmdError, match="no polynomial and no period"):
        pipeline.LoadToFold(pipeline.Config(nchan=16), info)
    # -d of the file's own state and the default pass the plan: the trap is the first thing they meet
    for npol in (2, 4):
        with pytest.raises(AssertionError, match="a device was opened"):
            pipeline.LoadToFold(pipeline.Config(**dict(ok, npol=npol)), info)
    # the search-mode drivers
    cfg = pipeline.SearchConfig(nchan=16, tscrunch=4, nbit=8)
    for drv, who in ((pipeline.LoadToFil, "LoadToFil:"), (pipeline.LoadToFilDirect, "LoadToFilDirect:"), (pipeline.LoadToFilCoherent, "LoadToFilCoherent:")):
        for nbits in (8, 2):                                       # (nbits 2 is not the two-bit voltage format)
            with pytest.raises(DspsrAmdError, match=who + ".*the input is detected already"):
                drv(cfg, _info(sigproc, tmp_path, nbits=nbits), device=None)
    with pytest.raises(DspsrAmdError, match="LoadToFITS: detected input"):
        pipeline.LoadToFITS(pipeline.FitsConfig(), info, device=None)



def test_communicators_are_refused(sigproc, tmp_path, monkeypatch):
    """the multi-GPU exchange: a planned detected run (the device side stopped) refuses both communicators by the back end's words"""
    from dspsr_amd import DspsrAmdError, pipeline
    info = _info(sigproc, tmp_path, nifs=2)
    ok = dict(nchan=16, folding_period=0.01, nbin=16)
    stop = RuntimeError("stop before the device")

    def no_open(self, *a):
        raise stop
    monkeypatch.setattr(pipeline.LoadToFold, "_open", no_open)
    monkeypatch.setattr(pipeline.LoadToFold, "close", lambda self: None)
    planned = []
    monkeypatch.setattr(pipeline.DetectedFold, "plan", lambda self, *a, _plan=pipeline.DetectedFold.plan: (planned.append(self.lt), _plan(self, *a))[1])
    with pytest.raises(RuntimeError, match="stop before the device"):
        pipeline.LoadToFold(pipeline.Config(**ok), info)
    lt = planned[0]
    assert isinstance(lt.mode, pipeline.DetectedFold)
    with pytest.raises(DspsrAmdError, match=r"LoadToFold.set_communicator: detected input is not built for a multi-GPU exchange"):
        lt.set_communicator(None, 0, 2)
    with pytest.raises(DspsrAmdError, match=r"LoadToFold.set_rccl_communicator: detected input is not built for a multi-GPU exchange"):
        lt.set_rccl_communicator(object())
    assert lt.comm is None and lt._subint_comm == pipeline.LoadToFold._subint_comm


def test_the_plan_of_a_detected_run(sigproc, tmp_path, monkeypatch):
    """what the host plan derives: no response, the file's rate, channels and polarisations, one spectrum per part, and with -K the
    delays of the file's own channels, the head room and the start time of DetectFold's plan"""
    import dspsr_amd
    from dspsr_amd import pipeline
    info = _info(sigproc, tmp_path, nifs=4, nbits=2)
    seen = {}

    class Stop(Exception):
        pass

    def opened(lt_self, *a):
        seen["lt"] = lt_self
        raise Stop()
    monkeypatch.setattr(pipeline.LoadToFold, "_open", opened)
    monkeypatch.setattr(pipeline.LoadToFold, "close", lambda self: None)
    for k in (False, True):
        with pytest.raises(Stop):
            pipeline.LoadToFold(pipeline.Config(nchan=16, folding_period=0.01, nbin=16, dispersion_measure=50.0, interchan_dedispersion=k,
                                                parts_per_block=4096), info)
        lt = seen["lt"]
        assert isinstance(lt.mode, pipeline.DetectedFold) and lt.fb is None and lt.response is None and lt.twobit is None
        assert (lt.nchan_out, lt.npol_out, lt.cfg.ndim, lt.cfg.npol, lt.nkeep, lt.nsamp_step, lt.nsamp_overlap) == (16, 4, 1, 4, 1, 1, 0)
        assert lt.out_rate == info.rate and lt.scalefac == 1.0 and lt.state_name() == "Coherence" and lt._fold_dims() == (4, 1)
        assert lt.block_bytes() == 4096 * 16 and lt.block_bytes(3) == 3 * 16
        if not k:
            assert lt.out_start == 0.0 and (lt.sd.head, lt.sd.zero) == (0, 0)
        else:
            d = dspsr_amd.dedispersion_sample_delays(info.centre_frequency, info.bandwidth, 50.0, 16, info.rate)
            assert np.array_equal(lt._delays, d) and lt.sd.zero == d.max() and lt.sd.head == (d.max() - d).max() > 0
            assert lt.out_start == lt.sd.zero / info.rate


@pytest.mark.parametrize("npol", [1, 2, 4])
@pytest.mark.parametrize("nbit", [1, 2, 4, 8])
def test_the_restatement_inverts_the_digitiser(nbit, npol):
    """two independent restatements of two reference files (SigProcDigitizer.C and SigProcUnpacker.C) that must be inverses: what the
    oracle's sigproc_digitize packs, unpack_fpt returns as the digitised levels -- at 8 bits, where the digitiser adds 127.5 to the
    cross products of dspsr's own files and the unpacker takes it off again, as the input itself"""
    import oracle.dspsr_oracle as o
    nchan, ndat, top = 24, 37, (1 << nbit) - 1
    rng = np.random.default_rng(nbit + npol)
    levels = rng.integers(0, top + 1, (ndat, nchan, npol))
    levels[0, :2, :] = [[0], [top]]
    mean = {1: 0.5, 2: 1.5, 4: 7.5, 8: 127.5}[nbit]
    x = levels.astype(np.float32)
    x[:, :, 2:] -= np.float32(mean)                       # use_digi_scales False: the mean is added to the cross products alone
    packed = o.sigproc_digitize(x, nbit, use_digi_scales=False)
    assert packed.dtype == np.uint8 and packed.size == ndat * sc.spectrum_bytes(nbit, nchan, npol)
    got = sc.unpack_fpt(packed.reshape(-1), nbit, nchan, npol, ndat)
    assert np.array_equal(got[:, :2], levels.transpose(1, 2, 0)[:, :2].astype(np.float32))
    if nbit == 8:
        assert np.array_equal(got, x.transpose(1, 2, 0))
    else:
        assert np.array_equal(got, levels.transpose(1, 2, 0).astype(np.float32))
    assert np.array_equal(sc.pack(levels.transpose(0, 2, 1), nbit), packed.reshape(-1))        # the files the pipeline tests write


def test_the_restatement_on_16_and_32_bits():
    v = np.arange(2 * 4 * 3, dtype=np.uint16).reshape(2, 4, 3) * 2500                     # [ndat][npol][nchan]
    got = sc.unpack_fpt(sc.pack(v, 16), 16, 3, 4, 2)
    want = v.transpose(2, 1, 0).astype(np.float32)
    want[:, 2:] -= 32768.0
    assert np.array_equal(got, want)
    f = np.array([[[1.5, -0.0, np.inf]], [[np.nan, 1e-45, -3.0]]], np.float32)
    got = sc.unpack_fpt(sc.pack(f, 32), 32, 3, 1, 2)
    assert np.array_equal(got.view(np.uint32), f.transpose(2, 1, 0).view(np.uint32).reshape(3, 1, 2))


def test_kernel_cases_reach_every_path():
    """the table of the kernel test: whole tiles (>= 128 values, >= 64 spectra) at every load width a sample size has, with rows
    that are and are not 16-byte aligned; spectra of odd length and of even length that is no multiple of 4; every raw offset"""
    for nbit in sc.NBITS:
        cases = sc.kernel_cases(nbit)
        whole = [(sc.load_width(nbit, off, sc.spectrum_bytes(nbit, nchan, npol)), (row_offset % 4 == 0 and (ndat + pad) % 4 == 0))
                 for nchan, npol, ndat, off, row_offset, pad in cases if nchan * npol >= 128 and ndat >= 64]
        assert {w for w, _a in whole} == set(sc.LOAD_WIDTHS[nbit])
        for w in sc.LOAD_WIDTHS[nbit]:
            assert {a for ww, a in whole if ww == w} == {True, False}, (nbit, w)
        assert {off for _c, _p, _n, off, _r, _d in cases} == set(sc.raw_offsets(nbit))
        assert {(c, p) for c, p, _n, _o, _r, _d in cases} >= {(c, p) for c in (sc.smallest_nchan(nbit), 24, 40, 64, 200, 1024) for p in sc.NPOLS if c != 1024}
        assert {n for _c, _p, n, _o, _r, _d in cases} == set(sc.NDATS)
        lengths = {sc.spectrum_bytes(nbit, c, p) for c, p, _n, _o, _r, _d in cases}
        if nbit == 1:
            assert {1, 3} <= lengths
        if nbit <= 2:
            assert any(s % 2 == 0 and s % 4 for s in lengths)
