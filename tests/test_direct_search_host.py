"""Search mode on channelised 8-bit voltages (`digifil file.dada` with no -F): what can be checked without a GPU -- the library's
symbols, the resources of the new kernels (read from the code objects inside the shipped library), the host side of
pipeline.LoadToFilDirect and of tools/dspsr_amd_digifil.py."""
import importlib.util
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from test_kernel_resources import LIB, _code_objects, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_direct_search_calls():
    import ctypes
    lib = ctypes.CDLL(LIB)
    for name in ("dspsr_amd_unpack_fpt", "dspsr_amd_detect_raw"):
        assert hasattr(lib, name), "%s is not exported by %s" % (name, LIB)
    import dspsr_amd
    assert callable(dspsr_amd.unpack_fpt) and callable(dspsr_amd.detect_raw)
    assert "dspsr_amd_unpack_fpt" in dspsr_amd._lib.SYMBOLS and "dspsr_amd_detect_raw" in dspsr_amd._lib.SYMBOLS


def test_direct_search_kernels_use_no_scratch():
    """Every instantiation of k_unpack_fpt and k_detect_raw: 0 bytes of scratch per lane and at most 256 VGPRs."""
    ks = {}
    for co in _code_objects(open(LIB, "rb").read()):
        ks.update(_kernels(co))
    names = sorted(ks)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    seen = {"k_unpack_fpt": 0, "k_detect_raw": 0}
    for d, n in zip(dem, names):
        short = d.split("(")[0].replace("void dspsr_amd::", "").replace("dspsr_amd::", "")
        for prefix in seen:
            if short.startswith(prefix):
                seen[prefix] += 1
                kd = ks[n]
                assert int(kd.get(".private_segment_fixed_size", 0)) == 0, "%s uses %s bytes of scratch per lane" % (
                    short, kd.get(".private_segment_fixed_size"))
                assert 0 < int(kd.get(".vgpr_count", 0)) <= 256, "%s: %s VGPRs" % (short, kd.get(".vgpr_count"))
    assert seen["k_unpack_fpt"] >= 1 and seen["k_detect_raw"] >= 1, seen


def _info(**kw):
    from dspsr_amd import pipeline
    base = dict(centre_frequency=1400.0, bandwidth=-64.0, nchan=8, npol=2, ndim=2, tsamp_us=0.125, machine="DADA")
    base.update(kw)
    return pipeline.InputInfo(**base)


def _planned(cfg, info):
    """A LoadToFilDirect with the host side of its constructor only (no device)."""
    from dspsr_amd import pipeline
    lt = pipeline.LoadToFilDirect(cfg, info, device=None)
    return lt, lt.sd.delays


def test_load_to_fil_direct_refusals_come_before_the_device():
    """No GPU here: a refusal that came after the context was created would surface as `no usable HIP device` instead."""
    from dspsr_amd import DspsrAmdError, pipeline
    S = pipeline.SearchConfig
    cases = [
        (S(npol=1), _info(ndim=1), "NDIM=1"),
        (S(npol=1), _info(nbit=16), "NBIT=16"),
        (S(npol=1), _info(machine="CASPSR"), "CASPSR"),
        (S(npol=3), _info(), "NthPower"),
        (S(npol=2), _info(npol=1), "invalid npol=1 for PPQQ formation"),
        (S(npol=4), _info(npol=1), "invalid npol=1 for Coherence formation"),
        (S(npol=1, fscrunch=3), _info(), "not a multiple of fscrunch=3"),
        (S(npol=1, dedisperse=True, dispersion_measure=500.0, parts_per_block=64), _info(), "inter-channel delay"),
        (S(npol=1, rescale_seconds=1e-9), _info(), "dsp::Rescale::init nsample == 0"),
    ]
    for cfg, info, text in cases:
        with pytest.raises(DspsrAmdError, match=text):
            pipeline.LoadToFilDirect(cfg, info)
    # the other two classes keep their refusals
    with pytest.raises(DspsrAmdError, match="single-channel input only"):
        pipeline.LoadToFil(S(), _info())
    with pytest.raises(DspsrAmdError, match="-F N:D"):
        pipeline.LoadToFilCoherent(S(nchan=8), _info())


def test_load_to_fil_direct_block_bytes_and_header_values(oracle):
    from dspsr_amd import dedispersion_sample_delays, pipeline
    info = _info(nchan=81, bandwidth=81.0, start_seconds=0.25, mjd_day=56000, mjd_sec=100.0)
    cfg = pipeline.SearchConfig(nchan=4096, tscrunch=16, nbit=2, npol=2, fscrunch=3, parts_per_block=1000, rescale_seconds=0.0)
    lt, delays = _planned(cfg, info)
    assert delays is None and not lt.fused                                  # -f: detected block, then FScrunch and TScrunch
    assert lt.block_bytes() == 1000 * 81 * 2 * 2 and lt.block_bytes(7) == 7 * 81 * 4 and lt.block_bytes(0) == 0
    assert lt.nchan_out == 27 and lt.bytes_per_sample == 27 * 2 * 2 // 8 and lt.input_scale == 48.0
    hv = lt.header_values()
    bw = -81.0                                                              # SigProcDigitizer.C:83-85: forced negative
    assert hv == dict(fch1=1400.0 - 0.5 * bw + 0.5 * bw / 27, foff=bw / 27, nchans=27, nbits=2, tsamp=16 / (1e6 / 0.125),
                      tstart_mjd=56000 + (100.0 + 0.25) / 86400.0, nifs=2)
    # one input polarisation, no scrunching: the one-pass form, float output
    lt, _ = _planned(pipeline.SearchConfig(tscrunch=0, nbit=-32, npol=1, parts_per_block=10, rescale_seconds=0.0), _info(npol=1))
    assert lt.fused and lt.ts == 1 and lt.block_bytes() == 10 * 8 * 2 and lt.bytes_per_sample == 8 * 4 and lt.header_values()["nbits"] == 32
    # -K: the delays of the file's channels (no swapped halves), start moved by the zero delay
    info = _info(nchan=8, bandwidth=-8.0, tsamp_us=1.0)
    cfg = pipeline.SearchConfig(tscrunch=4, nbit=8, npol=1, dedisperse=True, dispersion_measure=20.0, parts_per_block=4096)
    lt, delays = _planned(cfg, info)
    want = dedispersion_sample_delays(1400.0, -8.0, 20.0, 8, 1e6, swap=False, nsub_swap=0)
    obs = oracle.Observation(centre_frequency=1400.0, bandwidth=-8.0, tsamp_us=1.0, dispersion_measure=20.0)
    assert np.array_equal(delays, want) and np.array_equal(delays, oracle.dedispersion_sample_delays(obs, 8, 1e6))
    assert lt.sd_head == int(delays.max() - delays.min()) > 100 and not lt.fused
    assert lt.header_values()["tstart_mjd"] == info.mjd_day + (info.mjd_sec + int(delays.max()) / 1e6) / 86400.0


def _tool():
    spec = importlib.util.spec_from_file_location("dspsr_amd_digifil", os.path.join(ROOT, "tools", "dspsr_amd_digifil.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


HEADER = """HDR_VERSION 1.0
HDR_SIZE 4096
INSTRUMENT DADA
TELESCOPE PKS
SOURCE J0437-4715
FREQ 1400.0
BW 64.0
NCHAN 8
NPOL 2
NBIT 8
NDIM 2
TSAMP 0.125
UTC_START 2012-03-14-01:02:03
OBS_OFFSET 6400
"""


def test_digifil_tool_arguments():
    from dspsr_amd import DspsrAmdError, dada
    tool = _tool()
    a = tool.parse_args(["x.dada", "-b", "2", "-t", "16", "-f", "4", "-d", "2", "-K", "-D", "12.5", "-I", "5", "-c", "-s", "2.5", "-o", "y.fil"])
    assert (a.file, a.nbit, a.tscrunch, a.fscrunch, a.npol, a.dedisperse, a.dm, a.rescale_seconds, a.constant, a.scale_fac, a.output) == (
        "x.dada", 2, 16, 4, 2, True, 12.5, 5.0, True, 2.5, "y.fil")
    with pytest.raises(SystemExit):
        tool.parse_args(["x.dada", "-Z", "1"])                              # an unknown option
    with pytest.raises(SystemExit):
        tool.parse_args(["x.dada", "-F", "128"])                            # no filterbank on this path
    info, extras = dada.observation(HEADER)
    cfg = tool.search_config(a, info, extras)
    assert (cfg.tscrunch, cfg.fscrunch, cfg.npol, cfg.nbit, cfg.dedisperse, cfg.dispersion_measure, cfg.rescale_seconds,
            cfg.rescale_constant, cfg.scale_fac) == (16, 4, 2, 2, True, 12.5, 5.0, True, 2.5)
    assert cfg.parts_per_block == 64 * 1024 * 1024 // 32
    with pytest.raises(DspsrAmdError, match="-K needs a dispersion measure"):
        tool.search_config(tool.parse_args(["x.dada", "-K"]), info, extras)   # no DM in the header, no -D
    info2, extras2 = dada.observation(HEADER + "DM 30.5\n")
    assert tool.search_config(tool.parse_args(["x.dada", "-K"]), info2, extras2).dispersion_measure == 30.5


def test_digifil_tool_header_parses_back():
    """The .fil header of a tiny synthetic DADA header, walked keyword by keyword."""
    from dspsr_amd import dada
    tool = _tool()
    info, extras = dada.observation(HEADER)
    cfg = tool.search_config(tool.parse_args(["obs.dada", "-b", "8", "-t", "4", "-d", "2", "-I", "0"]), info, extras)
    lt, _ = _planned(cfg, info)
    f = io.BytesIO()
    tool.write_header(f, lt, info, "/somewhere/obs.dada")
    b = f.getvalue()
    assert b.startswith(struct.pack("<i", 12) + b"HEADER_START") and b.endswith(struct.pack("<i", 10) + b"HEADER_END")

    def value(key, fmt):
        k = struct.pack("<i", len(key)) + key.encode()
        i = b.index(k) + len(k)
        return struct.unpack_from(fmt, b, i)[0]

    def text(key):
        k = struct.pack("<i", len(key)) + key.encode()
        i = b.index(k) + len(k)
        n, = struct.unpack_from("<i", b, i)
        return b[i + 4:i + 4 + n].decode()
    assert text("rawdatafile") == "obs.dada" and text("source_name") == "J0437-4715"
    assert value("nchans", "<i") == 8 and value("nbits", "<i") == 8 and value("nifs", "<i") == 2 and value("data_type", "<i") == 1
    assert value("foff", "<d") == -8.0 and value("fch1", "<d") == 1400.0 + 32.0 - 4.0        # band flipped: highest channel first
    assert value("tsamp", "<d") == 4 / (1e6 / 0.125)
    start = (6400 * 8 // (8 * 2 * 2 * 8)) * 0.125e-6                                          # OBS_OFFSET in samples
    day, sec = info.mjd_day, info.mjd_sec
    assert (day, sec) == (56000, 3723.0) and value("tstart", "<d") == day + (sec + start) / 86400.0
