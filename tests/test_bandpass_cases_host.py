"""What the device tests of the passband kernels rest on (tests/bandpass_cases.py), checked without a device: the exact cases are
exact, every refusal of the C-ABI's device-free checks, the launch arithmetic restated -- each part count reaches the edge it is
there for -- and every refusal of pipeline.rfi_check.  CPU only."""
import numpy as np
import pytest

import bandpass_cases as bc
import rfi_reference as rr
import dspsr_amd
from dspsr_amd import _lib, pipeline

FORM = {"float": -1, "generic": _lib.RAW_GENERIC, "caspsr": _lib.RAW_CASPSR}


@pytest.mark.parametrize("index", range(len(bc.EXACT)), ids=bc.IDS)
def test_exact_cases_are_exact_and_reach_their_edges(index):
    form, ndim, res, npol_in, npol_out, nchan_in, _tone, big = bc.EXACT[index]
    dspsr_amd.bandpass_check_shape(nchan_in, npol_in, ndim, res, npol_out)
    nsamp_fft = res * (2 if ndim == 1 else 1)
    tp = 8192 // res
    seen = set()
    for npart in bc.part_counts(index):
        data, ndat, ref = bc.exact_case(index, npart)
        # every sum is a small integer times resolution^2: exact in float32 in any order
        units = ref / float(res * res)
        assert np.array_equal(units, np.rint(units)) and np.abs(units).max() + bc.SENTINEL_UNITS < 2 ** 23
        assert ref.shape == (npol_out, nchan_in, res) and ref[:2].min() >= 0 and ref.any()
        assert ndat // nsamp_fft == npart and ndat % nsamp_fft                 # a trailing partial transform
        if form == "float":
            assert np.isnan(data[:, :, npart * nsamp_fft * ndim:]).all() and np.isfinite(data[:, :, :npart * nsamp_fft * ndim]).all()
            row = ndat * ndim
            got = dspsr_amd.bandpass_check_input(nchan_in, npol_in, ndim, res, -1, 4, 2 * row + 7, row + 3, ndat)
        else:
            rows = rr.decode_raw(data, form, nchan_in, npol_in, ndim, bc.RAW_SCALE)
            assert (rows[:, :, npart * nsamp_fft * ndim:] == -255).all()        # -128 bytes
            assert np.array_equal(rr.bandpass_loop(rows[:, :, :ndat * ndim], ndim, res, npol_out, strict=False), ref)
            got = dspsr_amd.bandpass_check_input(nchan_in, npol_in, ndim, res, FORM[form], 8, 0, 0, ndat)
        want = bc.launch_arithmetic(npart, nchan_in, res)
        assert got == want and want[0] == tp
        _tp, tps, nseg = want
        ntile = -(-npart // tp)
        last = ntile - (nseg - 1) * tps
        if npart == tp - 1:
            seen.add("one tile, its last part missing")
            assert (ntile, nseg) == (1, 1)
        if npart == tp:
            seen.add("one whole tile")
            assert (ntile, nseg) == (1, 1)
        if npart == tp + 1 and tp > 1:
            seen.add("a second tile of one part")
            assert ntile == 2
        if npart == 2 * tp + 1:
            seen.add("three segments")
            assert nseg >= 3 and last == 1
        if npart == 256 * tp + 1:
            seen.add("segments of two tiles")
            assert (tps, nseg, last) == (2, 129, 1)
    assert {"one whole tile", "three segments"} <= seen
    assert ("segments of two tiles" in seen) == big
    if tp > 1:
        assert {"one tile, its last part missing", "a second tile of one part"} <= seen


def test_the_case_list_covers_what_it_must():
    cases = bc.EXACT
    assert {c[2] for c in cases} == {2, 16, 512, 1024, 8192}
    for form in ("float", "generic", "caspsr"):
        assert {c[2] for c in cases if c[0] == form} == {2, 16, 512, 1024, 8192}
        assert any(c[7] for c in cases if c[0] == form)
    for form in ("float", "generic"):
        mine = [c for c in cases if c[0] == form]
        assert {c[1] for c in mine} == {1, 2} and {(c[3], c[4]) for c in mine} == {(1, 1), (2, 2), (2, 4)} and {c[5] for c in mine} == {1, 3}
    assert {(c[3], c[4]) for c in cases if c[0] == "caspsr"} == {(2, 2), (2, 4)}
    assert {(n[0], n[1]) for n in bc.NOISE} == {(d, r) for d in (1, 2) for r in (2, 1024, 8192)} and min(n[2] for n in bc.NOISE) >= 64


def test_the_cut_depends_on_parts_channels_and_resolution_alone():
    for res, nchan_in, ndim, npart in ((2, 1, 1, 5), (1024, 3, 2, 1000), (8192, 1, 1, 600), (1024, 1, 1, 262144), (8192, 700, 2, 9)):
        nsamp_fft = res * (2 if ndim == 1 else 1)
        want = bc.launch_arithmetic(npart, nchan_in, res)
        for npol_in in (1, 2):
            got = dspsr_amd.bandpass_check_input(nchan_in, npol_in, ndim, res, -1, 0, 1 << 40, 1 << 36, npart * nsamp_fft)
            assert got == want
    assert bc.launch_arithmetic(262144, 1, 1024) == (8, 128, 256)              # the headline block: 2^29 samples, 1024 channels


@pytest.mark.parametrize("args,text", [
    ((1, 2, 1, 0, 2), "number of output frequency channels == 0"),
    ((1, 2, 1, 1, 2), "resolution=1 must be a power of two in"),
    ((1, 2, 1, 24, 2), "resolution=24 must be a power of two"),
    ((1, 2, 1, 16384, 2), "resolution=16384 must be a power of two in"),
    ((1, 2, 4, 16, 2), "ndim_in=4 is neither Nyquist .1. nor Analytic .2.; detected input is not built"),
    ((1, 3, 1, 16, 3), "npol_in=3 not 1 or 2"),
    ((1, 1, 1, 16, 4), "npol_out=4 must be npol_in=1, or 4 with npol_in=2"),
    ((1, 2, 1, 16, 1), "npol_out=1 must be npol_in=2"),
    ((0, 2, 1, 16, 2), "nchan_in=0 outside"),
    ((65536, 2, 1, 16, 2), "nchan_in=65536 outside"),
    ((4096, 2, 1, 8192, 2), "nchan_in=4096 x resolution=8192 > 2.24: the sums of one segment would exceed 256 MiB"),
    ((65535, 1, 2, 512, 1), "nchan_in=65535 x resolution=512 > 2.24"),
])
def test_shape_refusals(args, text):
    with pytest.raises(dspsr_amd.DspsrAmdError, match=text):
        dspsr_amd.bandpass_check_shape(*args)


@pytest.mark.parametrize("args,text", [
    ((1, 2, 1, 16, -1, 4, 0, 64, 1 << 31), "ndat=2147483648 >= 2.31"),
    ((1, 2, 1, 16, -1, 2, 0, 64, 64), "rows must be 4-byte aligned"),
    ((1, 2, 1, 16, -1, 4, 0, 63, 64), "stride shorter than the row of 64 floats"),
    ((3, 1, 2, 16, -1, 4, 127, 0, 64), "stride shorter than the row of 128 floats"),
    ((1, 2, 1, 16, -1, 4, 0, 64, 31), "error ndat=31 < nfft=32"),
    ((1, 2, 2, 16, _lib.RAW_GENERIC, 1, 0, 0, 15), "error ndat=15 < nfft=16"),
    ((1, 2, 1, 16, _lib.RAW_UWB16, 0, 0, 0, 64), "DSPSR_AMD_RAW_UWB16 .16-bit input. is not built"),
    ((3, 2, 1, 16, _lib.RAW_CASPSR, 0, 0, 0, 64), "DSPSR_AMD_RAW_CASPSR is one channel of two real polarisations"),
    ((1, 2, 2, 16, _lib.RAW_CASPSR, 0, 0, 0, 64), "DSPSR_AMD_RAW_CASPSR is one channel of two real polarisations"),
    ((1, 2, 1, 16, _lib.RAW_CASPSR, 4, 0, 0, 64), "starts on an 8-byte group"),
    ((1, 2, 1, 16, 7, 0, 0, 0, 64), "unknown raw_layout 7"),
])
def test_input_refusals(args, text):
    with pytest.raises(dspsr_amd.DspsrAmdError, match=text):
        dspsr_amd.bandpass_check_input(*args)


def test_the_partial_arrays_stay_within_their_limit():
    """the largest shapes set_shape accepts: segments x one partial array (four output polarisations) <= 256 MiB"""
    for nchan_in, res in ((2048, 8192), (65535, 256), (1, 8192), (3, 1024)):
        dspsr_amd.bandpass_check_shape(nchan_in, 2, 1, res, 4)
        for npart in (1, 100000):
            _tp, _tps, nseg = dspsr_amd.bandpass_check_input(nchan_in, 2, 2, res, -1, 0, 1 << 40, 1 << 36, npart * res)
            assert nseg >= 1 and nseg * 4 * nchan_in * res * 4 <= 256 << 20
            assert (_tp, _tps, nseg) == bc.launch_arithmetic(npart, nchan_in, res)


def test_rfi_check_refusals():
    cfg = pipeline.Config(nchan=16, dispersion_measure=10.0, zap_rfi=True)
    info = pipeline.InputInfo()
    pipeline.rfi_check(cfg, info)
    import dataclasses
    for c, i, sub, text in (
            (dataclasses.replace(cfg, calibrator=("f", "j")), info, None, "-pac .calibrator. is not built"),
            (cfg, dataclasses.replace(info, nchan=4), None, "one input channel .info.nchan=4."),
            (dataclasses.replace(cfg, convolve_when="never"), info, None, "needs a dedispersion kernel"),
            (dataclasses.replace(cfg, dispersion_measure=0.0), info, None, "needs a dedispersion kernel"),
            (cfg, dataclasses.replace(info, npol=1), None, "two polarisations .info.npol=1."),
            (dataclasses.replace(cfg, plfb_nbin=8, ndim=1, npol=1), dataclasses.replace(info, npol=1), None, "two polarisations .info.npol=1."),
            (cfg, info, 0, "sub-band sharded runs .subband=0."),
            (cfg, dataclasses.replace(info, nbit=16), None, "16-bit input is not built")):
        with pytest.raises(dspsr_amd.DspsrAmdError, match=text):
            pipeline.rfi_check(c, i, sub)
        with pytest.raises(dspsr_amd.DspsrAmdError, match=text):         # LoadToFold refuses before it opens a device
            pipeline.LoadToFold(dataclasses.replace(c, folding_period=0.01), i, subband=sub)
