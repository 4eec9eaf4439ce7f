"""The phase-locked filterbank (dspsr -G nbin) without a device: the host plan against a sample-walking restatement of
dsp::TimeDivide (tests/plfb_reference.py), the choice of nchan, every refusal of the pipeline and of the C-ABI with its message,
the hand-off file through the Python and the C++ reader, and the resources of the k_plfb* kernels in the shipped library."""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import plfb_reference as pr
from plfb_cases import EXACT, IDS, SENTINEL_UNITS, exact_case
from dspsr_amd import DspsrAmdError, pipeline
import dspsr_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 390625.0
PERIOD = 0.0893


def _ephemeris(use_polyco):
    """phase(t) -> (int, frac), iphase((int, frac), guess) -> t, period guess; t in seconds of the stream"""
    if use_polyco:
        pc = pipeline.Polyco(json.load(open(os.path.join(ROOT, "tests", "golden", "vela_polyco.json")))["text"])
        phase = lambda t: pc.phase(55299, 7545.0 + t)
        iphase = lambda ph, guess: pc.iphase(ph, 55299, 7545.0 + guess) - 7545.0
        return phase, iphase, 1.0 / pc.frequency(55299, 7545.0)
    phase = lambda t: (int(np.floor(t / PERIOD)), t / PERIOD - np.floor(t / PERIOD))
    iphase = lambda ph, guess: (ph[0] + ph[1]) * PERIOD
    return phase, iphase, PERIOD


def _boundary_start(phase, iphase, nbin, ref, side):
    """a stream start whose phase lies 1e-9 s below (side = -1) or above (+1) a bin boundary ref + m / nbin"""
    d = 1.0 / nbin
    pi, pf = phase(0.00108)
    x = ref + np.ceil((pf - ref) / d + 2) * d
    t_b = iphase((pi + int(np.floor(x)), x - np.floor(x)), 0.00108)
    return t_b + side * 1e-9


def _plan(phase, iphase, pguess, t_start, nbin, ref, ndat_fft):
    div = pipeline.TurnsDivider(phase, iphase, pguess, t_start, RATE, 1.0 / nbin, ref)
    return pipeline.PlfbPlan(div, nbin, ref, ndat_fft)


def _as_list(starts, bins):
    return list(zip((int(s) for s in starts), (int(b) for b in bins)))


@pytest.mark.parametrize("use_polyco", [False, True])
@pytest.mark.parametrize("nbin", [2, 3, 64, 1024])
@pytest.mark.parametrize("ref", [0.0, 0.3])
@pytest.mark.parametrize("side", [-1, 1])
def test_plan_equals_the_restatement(use_polyco, nbin, ref, side):
    phase, iphase, pguess = _ephemeris(use_polyco)
    t_start = _boundary_start(phase, iphase, nbin, ref, side)
    ndat_fft = pr.reference_nchan(pguess, RATE, nbin)
    turns = 2.2 if nbin < 1024 else 0.6
    ndat = int(turns * pguess * RATE)
    want = pr.divider_windows(phase, iphase, t_start, RATE, nbin, ref, ndat, ndat_fft)
    got = _as_list(*_plan(phase, iphase, pguess, t_start, nbin, ref, ndat_fft).take(ndat))
    assert got == want
    assert len(want) >= min(nbin, 4) and all(0 <= b < nbin for _, b in want)
    # consecutive divisions fall into consecutive phase bins, and the first starts less than one division after the first sample
    assert all((b1 - b0) % nbin == 1 for (_, b0), (_, b1) in zip(want, want[1:]))
    assert 0 <= want[0][0] <= int(pguess * RATE / nbin) + 1
    # a stream that ends exactly at a window's last sample keeps it; one sample short of it does not (PhaseLockedFilterbank.C:224-228)
    j = len(want) - 2
    end = want[j][0] + ndat_fft
    for n, count in ((end, j + 1), (end - 1, j)):
        w = pr.divider_windows(phase, iphase, t_start, RATE, nbin, ref, n, ndat_fft)
        g = _as_list(*_plan(phase, iphase, pguess, t_start, nbin, ref, ndat_fft).take(n))
        assert g == w == want[:count]
    hits, total, length = pr.window_totals(want, nbin, ndat_fft, RATE)
    assert hits.sum() == total == len(want) and abs(length - total * ndat_fft / RATE) < 1e-9


@pytest.mark.parametrize("use_polyco", [False, True])
@pytest.mark.parametrize("nbin,ref", [(3, 0.3), (64, 0.0)])
def test_plan_does_not_depend_on_the_blocks(use_polyco, nbin, ref):
    phase, iphase, pguess = _ephemeris(use_polyco)
    ndat_fft = pr.reference_nchan(pguess, RATE, nbin)
    ndat = int(3.3 * pguess * RATE)
    whole = _as_list(*_plan(phase, iphase, pguess, 0.00108, nbin, ref, ndat_fft).take(ndat))
    assert whole == pr.divider_windows(phase, iphase, 0.00108, RATE, nbin, ref, ndat, ndat_fft)
    for nblock in (2, 7):
        plan, got = _plan(phase, iphase, pguess, 0.00108, nbin, ref, ndat_fft), []
        for k in range(1, nblock + 1):
            avail = ndat * k // nblock
            got += _as_list(*plan.take(avail))
            assert plan.next_start() + ndat_fft > avail           # what is carried is shorter than a window
        assert got == whole


@pytest.mark.parametrize("period,rate,nbin", [(0.0893, 1e6, 256), (0.0016, 1e6, 64), (0.004, 5e5, 8), (0.0893, 390625.0, 1024),
                                               (0.001, 1e6, 3)])
def test_nchan_zero_is_the_reference_choice(period, rate, nbin):
    n = pipeline.plfb_choose_nchan(period, rate, nbin)
    assert n == pr.reference_nchan(period, rate, nbin)
    assert n & (n - 1) == 0 and n <= period * rate / nbin < 2 * n


def test_the_issue_shapes():
    """-F 16:D -G 256 at the Vela period and -G 64 at 1.6 ms, 16 channels of 400 MHz: 8192 and 512 channels per window"""
    rate = 400e6 / 16
    assert pipeline.plfb_choose_nchan(0.0893, rate, 256) == 8192
    assert pipeline.plfb_choose_nchan(0.0016, rate, 64) == 512


CFG = pipeline.Config(nchan=8, dispersion_measure=30.0, nbin=64, folding_period=0.004, plfb_nbin=8)
INFO = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=-16.0, npol=2, ndim=1, tsamp_us=1.0 / 32.0, machine="DADA")


@pytest.mark.parametrize("change,kwargs,text", [
    (dict(subint_seconds=1.0), {}, "sub-integrations .*counts windows twice"),
    (dict(subint_turns=1.0), {}, "sub-integrations .*counts windows twice"),
    (dict(subint_turns=16.0), {}, "sub-integrations .*counts windows twice"),
    (dict(interchan_dedispersion=True), {}, "not built for -K"),
    ({}, dict(targets=[pipeline.FoldTarget(folding_period=0.004), pipeline.FoldTarget(folding_period=0.005)]), "one pulsar; 2 targets"),
    (dict(cyclic_nchan=32), {}, "cyclic spectra .*exclude each other"),
    (dict(fourth_moment=True), {}, "fourth moments .*exclude each other"),
    (dict(convolve_when="after"), {}, "convolve_when = during"),
    (dict(convolve_when="before"), {}, "convolve_when = during"),
    (dict(convolve_when="never"), {}, "convolve_when = during"),
    ({}, dict(subband=0), "sub-band sharded runs"),
    ({}, dict(dump_before=("Fold",)), "dump taps"),
    ({}, dict(dump_before=("Detection",)), "dump taps"),
    (dict(npol=3), {}, r"Invalid npol \(3\)"),
    (dict(plfb_nchan=1, plfb_nbin=1), {}, "invalid dimensions.  nchan=1 nbin=1"),
    (dict(plfb_nchan=48), {}, r"nchan=48 must be a power of two in \[2, 8192\]"),
    (dict(plfb_nchan=16384), {}, r"nchan=16384 must be a power of two in \[2, 8192\]"),
])
def test_pipeline_refusals_before_any_device(change, kwargs, text):
    with pytest.raises(DspsrAmdError, match=text):
        pipeline.LoadToFold(dataclasses.replace(CFG, **change), INFO, **kwargs)


def test_one_input_polarisation_gives_intensity_only():
    with pytest.raises(DspsrAmdError, match=r"Not enough input polns \(1\) for output npol \(4\)"):
        pipeline.LoadToFold(CFG, dataclasses.replace(INFO, npol=1))


def test_plfb_off_is_the_default():
    c = pipeline.Config()
    assert (c.plfb_nbin, c.plfb_nchan) == (0, 0)


@pytest.mark.parametrize("args,text", [
    ((1, 2, 2, 1, 1, 1), "invalid dimensions.  nchan=1 nbin=1"),
    ((1, 2, 2, 1, 1, 8), r"nchan=1 must be a power of two in \[2, 8192\]"),
    ((1, 2, 2, 24, 1, 8), r"nchan=24 must be a power of two in \[2, 8192\]"),
    ((1, 2, 2, 16384, 1, 8), r"nchan=16384 must be a power of two in \[2, 8192\]"),
    ((1, 2, 2, 16, 3, 8), r"Invalid npol \(3\)"),
    ((1, 2, 2, 16, 0, 8), r"Invalid npol \(0\)"),
    ((1, 1, 2, 16, 2, 8), r"Not enough input polns \(1\) for output npol \(2\)"),
    ((1, 1, 2, 16, 4, 8), r"Not enough input polns \(1\) for output npol \(4\)"),
    ((1, 2, 3, 16, 4, 8), "ndim_in=3 is neither Nyquist"),
    ((1, 2, 0, 16, 4, 8), "ndim_in=0 is neither Nyquist"),
    ((0, 2, 2, 16, 4, 8), "zero dimension"),
    ((1, 2, 2, 16, 4, 0), "zero dimension"),
    ((1, 3, 2, 16, 4, 8), "npol_in=3 not 1 or 2"),
])
def test_shape_refusals(args, text):
    with pytest.raises(DspsrAmdError, match=text):
        dspsr_amd.plfb_check_shape(*args)


def test_shapes_accepted():
    for nchan in (2, 16, 8192):
        for npol_in, npol_out in ((1, 1), (2, 1), (2, 2), (2, 4)):
            for ndim in (1, 2):
                dspsr_amd.plfb_check_shape(3, npol_in, ndim, nchan, npol_out, 1025)
    dspsr_amd.plfb_check_shape(1, 2, 2, 2, 4, 1)           # nbin 1 with nchan >= 2 (PhaseLockedFilterbank.C:61-63)


def _windows(**kw):
    a = dict(nchan_in=2, npol_in=2, ndim_in=2, nchan=16, nbin=8, in_addr=0x1000, chan_stride=4096, pol_stride=2048, ndat=1000,
             idat_start=[0, 16, 984], bins=[1, 2, 7])
    a.update(kw)
    dspsr_amd.plfb_check_windows(**a)


@pytest.mark.parametrize("kw,text", [
    (dict(idat_start=[0, 16, 985]), r"window 2: idat_start=985 \+ ndat_fft=16 > ndat=1000"),
    (dict(ndim_in=1, idat_start=[0, 16, 969]), r"window 2: idat_start=969 \+ ndat_fft=32 > ndat=1000"),
    (dict(bins=[1, 8, 7]), "window 1: bin=8 >= nbin=8"),
    (dict(idat_start=[0, 32, 16]), "window 2: idat_start=16 before its predecessor's 32: windows out of time order"),
    (dict(in_addr=0x1004), "rows must be 8-byte aligned"),
    (dict(chan_stride=4097), "rows must be 8-byte aligned"),
    (dict(pol_stride=2049), "rows must be 8-byte aligned"),
    (dict(ndim_in=1, in_addr=0x1002), "rows must be 4-byte aligned"),
    (dict(pol_stride=1998), "stride shorter than the row of 2000 floats"),
    (dict(chan_stride=1998), "stride shorter than the row of 2000 floats"),
    (dict(ndat=1 << 31), "ndat=2147483648 or nwin=3 >= 2\\^31"),
])
def test_window_refusals(kw, text):
    with pytest.raises(DspsrAmdError, match=text):
        _windows(**kw)


def test_windows_accepted():
    _windows()
    _windows(idat_start=[], bins=[])
    _windows(idat_start=[5, 5, 6], bins=[0, 0, 0])                          # overlapping windows, equal starts
    _windows(ndim_in=1, in_addr=0x1004, chan_stride=1001, pol_stride=1000, idat_start=[1, 3, 968])   # Nyquist rows: any float address
    _windows(nchan_in=1, npol_in=1, chan_stride=0, pol_stride=0)            # strides of absent dimensions are not looked at


DRIVER = r'''
#include "dspsr_amd_phase_series_io.h"
int main (int argc, char** argv)
{
  try {
    HIP::PhaseSeriesFile f = HIP::read_phase_series_file (argv[1]);
    double s = 0;
    for (size_t i = 0; i < f.sums.size (); i++) s += double (f.sums[i]) * double (i % 7 + 1);
    printf ("%u %u %u %u %.17g %s %.17g %u %.17g %.17g %llu\n", f.nchan, f.npol, f.ndim, f.nbin, s, f.text ("STATE").c_str (),
            f.number ("RATE"), unsigned (f.number ("NSUB_SWAP")), f.number ("SCALE"), f.number ("INTEGRATION_LENGTH"),
            (unsigned long long) f.number ("NDAT_TOTAL"));
  } catch (std::exception& e) { fprintf (stderr, "%s\n", e.what ()); return 1; }
  return 0;
}
'''


@pytest.mark.parametrize("npol,state", [(1, "Intensity"), (2, "PPQQ"), (4, "Coherence")])
def test_hand_off_file_round_trip(tmp_path, npol, state):
    rng = np.random.default_rng(npol)
    nchan_rows, nchan_fft, nbin = 8, 64, 8
    nchan = nchan_rows * nchan_fft
    sub = {"hits": rng.integers(1, 9, nbin).astype(np.uint32), "integration_length": 0.03125, "ndat_total": 977,
           "profile": rng.standard_normal((nchan, npol, nbin, 1)).astype(np.float32)}
    rate, scale = 1e6 / nchan_fft, 4096.0 * 512 * nchan_fft
    path = str(tmp_path / "g.ps")
    pipeline.write_phase_series(path, sub, INFO, CFG, nchan=nchan, npol=npol, state=state, ndim=1, scale=scale, folding_period=0.004,
                                rate=rate, nsub_swap=nchan_rows)
    hdr, hits, prof = pipeline.read_phase_series(path)
    assert (hdr["STATE"], hdr["NDIM"], hdr["NPOL"], hdr["NCHAN"], hdr["NBIN"]) == (state, "1", str(npol), str(nchan), str(nbin))
    assert float(hdr["RATE"]) == rate and int(hdr["NSUB_SWAP"]) == nchan_rows and float(hdr["SCALE"]) == scale
    assert int(hdr["NDAT_TOTAL"]) == 977 and float(hdr["INTEGRATION_LENGTH"]) == 0.03125
    assert np.array_equal(hits, sub["hits"]) and np.array_equal(prof, sub["profile"])
    # the C++ reader of the DSPSR side
    src, exe = tmp_path / "r.cpp", tmp_path / "r"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "dspsr_amd", "host"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe), path], check=True, capture_output=True, text=True).stdout.split()
    flat = sub["profile"].reshape(-1).astype(np.float64)
    want_s = float((flat * (np.arange(flat.size) % 7 + 1)).sum())
    assert [int(v) for v in out[:4]] == [nchan, npol, 1, nbin] and abs(float(out[4]) - want_s) <= 1e-9 * abs(want_s)
    assert out[5] == state and float(out[6]) == rate and int(out[7]) == nchan_rows and float(out[8]) == scale
    assert float(out[9]) == 0.03125 and int(out[10]) == 977
    # a file without the two keys is what it always was
    pipeline.write_phase_series(path, sub, INFO, CFG, nchan=nchan, npol=npol, state=state, ndim=1)
    hdr, _, _ = pipeline.read_phase_series(path)
    assert "RATE" not in hdr and "NSUB_SWAP" not in hdr


def test_tool_takes_G():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold", os.path.join(ROOT, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["-F", "8:D", "-G", "8", "-c", "0.004", "-d", "2", "x.dada"])
    assert a.plfb_nbin == 8 and a.ndim == 2
    assert tool.parse_args(["-F", "8:D", "-c", "0.004", "x.dada"]).plfb_nbin == 0


def test_plfb_kernels_use_no_scratch():
    """Every k_plfb* kernel of the shipped library: no scratch memory, at most 256 VGPRs (read as tests/test_kernel_resources.py
    reads the hot kernels)."""
    import test_kernel_resources as tkr
    blob = open(tkr.LIB, "rb").read()
    ks = {}
    for co in tkr._code_objects(blob):
        ks.update(tkr._kernels(co))
    names = sorted(n for n in ks if "k_plfb" in n)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    got = {d.split("(")[0].replace("void dspsr_amd::", "").replace("dspsr_amd::", ""): ks[n] for d, n in zip(dem, names)}
    want = ["k_plfb<%d, %d, %d>" % (logc, ndim, npo) for logc in range(1, 14) for ndim in (1, 2) for npo in (1, 2, 4)] + ["k_plfb_combine"]
    assert sorted(got) == sorted(want)
    for name, kd in got.items():
        assert int(kd.get(".private_segment_fixed_size", 0)) == 0, "%s: %d bytes of scratch per lane" % (name, kd[".private_segment_fixed_size"])
        assert int(kd.get(".vgpr_count", 0)) <= 256


@pytest.mark.parametrize("index", range(len(EXACT)), ids=IDS)
def test_reference_stays_exact(index):
    """(no device) every sum of the case is an integer multiple of nchan^2 with a multiplier below 2^24, the sentinel included:
    the float64 reference converted to float32 is the one expected bit pattern"""
    nchan = EXACT[index][1]
    ref = exact_case(index)[3]
    units = ref / float(nchan * nchan)
    assert np.array_equal(units, np.round(units)) and np.abs(units).max() + SENTINEL_UNITS < 2 ** 24
    assert np.abs(units).max() > 0
    assert sum(len(np.setdiff1d(np.arange(c[5]), exact_case(i)[2])) > 0 for i, c in enumerate(EXACT)) >= 8     # bins without a window
