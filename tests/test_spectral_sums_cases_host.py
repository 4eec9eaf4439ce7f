"""What tests/test_gpu_spectral_sums_parent.py rests on, checked without a device: the fixture holds exactly the cases of
tests/spectral_sums_cases.py, the list covers every size, form and polarisation path it is there for, and each case is what it claims
to be -- three tiles in at least two segments; for the phase-locked filterbank a bin that spans segments and one that does not.
CPU only."""
import json
import os

import numpy as np
import pytest

import bandpass_cases as bc
import spectral_sums_cases as cases
import dspsr_amd
from dspsr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM = {"float": -1, "generic": _lib.RAW_GENERIC, "caspsr": _lib.RAW_CASPSR}

with open(os.path.join(ROOT, "tests", "golden", "spectral_sums_parent.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_holds_exactly_the_cases():
    assert len(set(cases.IDS)) == len(cases.IDS) == len(cases.BANDPASS) + len(cases.PLFB)
    assert sorted(GOLDEN) == sorted(cases.IDS)
    for name, rec in GOLDEN.items():
        assert sorted(rec) == ["first", "sha256", "shape"], name
        assert len(rec["sha256"]) == 64 and int(rec["sha256"], 16) >= 0, name
        assert len(rec["first"]) == 8 and all(np.isfinite(float.fromhex(v)) for v in rec["first"]), name
    for c, name in zip(cases.BANDPASS, cases.BANDPASS_IDS):
        assert GOLDEN[name]["shape"] == [c[4], 1, c[2]], name
    for c, name in zip(cases.PLFB, cases.PLFB_IDS):
        assert GOLDEN[name]["shape"] == [cases.PLFB_NCHAN_IN * c[1], c[3], cases.PLFB_NBIN], name
    assert len({rec["sha256"] for rec in GOLDEN.values()}) == len(GOLDEN)


def test_the_case_list_covers_what_it_must():
    sizes, ends = {2, 16, 512, 2048, 4096, 8192}, {16, 8192}
    b = cases.BANDPASS
    for ndim in (1, 2):
        assert {c[2] for c in b if c[:2] == ("float", ndim) and c[3:] == (2, 4)} == sizes
        assert {c[2] for c in b if c[:2] == ("float", ndim) and c[3:] == (1, 1)} == ends
        assert {c[2] for c in b if c[:2] == ("float", ndim) and c[3:] == (2, 2)} == ends
        assert {c[2] for c in b if c[:2] == ("generic", ndim)} == ends
    assert {c[1:3] for c in b if c[0] == "caspsr"} == {(1, 16), (1, 1024), (1, 8192)}
    assert all(c[3:] == (2, 4) for c in b if c[0] != "float")
    p = cases.PLFB
    for ndim in (1, 2):
        assert {c[1] for c in p if c[0] == ndim and c[2:] == (2, 4)} == sizes
        for pols in ((2, 1), (1, 1), (2, 2)):
            assert {c[1] for c in p if c[0] == ndim and c[2:] == pols} == ends
    assert {c[2:] for c in p} == {(2, 4), (2, 1), (1, 1), (2, 2)}


@pytest.mark.parametrize("index", range(len(cases.BANDPASS)), ids=cases.BANDPASS_IDS)
def test_bandpass_cases_have_three_tiles_in_several_segments(index):
    form, ndim, res, npol_in, npol_out = cases.BANDPASS[index]
    dspsr_amd.bandpass_check_shape(1, npol_in, ndim, res, npol_out)
    data, ndat = cases.bandpass_case(index)
    nsamp_fft = res * (2 if ndim == 1 else 1)
    npart = ndat // nsamp_fft
    assert npart == 2 * (8192 // res) + 1 and data.nbytes <= 512 << 10
    if form == "float":
        assert data.dtype == np.float32 and data.shape == (1, npol_in, ndat * ndim) and np.isfinite(data).all() and data.std() > 0.9
        got = dspsr_amd.bandpass_check_input(1, npol_in, ndim, res, -1, 0, npol_in * ndat * ndim, ndat * ndim, ndat)
    else:
        assert data.dtype == np.uint8 and data.ndim == 1 and len(np.unique(data)) > 200
        assert data.size >= (ndat * npol_in * ndim if form == "generic" else -(-ndat // 4) * 8)
        got = dspsr_amd.bandpass_check_input(1, npol_in, ndim, res, FORM[form], 0, 0, 0, ndat)
    tp, tps, nseg = got
    assert got == bc.launch_arithmetic(npart, 1, res) and tp == 8192 // res
    assert -(-npart // tp) == 3 and nseg >= 2 and npart - 2 * tp == 1          # three tiles, the last of one part
    assert cases.bandpass_case(index)[0] is data                              # computed once, shared


@pytest.mark.parametrize("index", range(len(cases.PLFB)), ids=cases.PLFB_IDS)
def test_plfb_cases_have_a_bin_across_segments_and_one_inside(index):
    ndim, nchan, npol_in, npol_out = cases.PLFB[index]
    nchan_in, nbin = cases.PLFB_NCHAN_IN, cases.PLFB_NBIN
    dspsr_amd.plfb_check_shape(nchan_in, npol_in, ndim, nchan, npol_out, nbin)
    rows, starts, bins, ndat = cases.plfb_case(index)
    assert rows.dtype == np.float32 and rows.shape == (nchan_in, npol_in, ndat * ndim) and np.isfinite(rows).all() and rows.std() > 0.9
    assert rows.nbytes <= 512 << 10
    dspsr_amd.plfb_check_windows(nchan_in, npol_in, ndim, nchan, nbin, 0, npol_in * ndat * ndim, ndat * ndim, ndat, starts, bins)
    nwin = len(starts)
    assert nwin == 2 * (8192 // nchan) + 1 and np.array_equal(np.diff(starts.astype(np.int64)), np.ones(nwin - 1))
    assert int(starts[-1]) + nchan * (2 if ndim == 1 else 1) == ndat            # the last window ends on the last sample
    tp, wps, nseg = cases.plfb_cut(nwin, nchan_in, nchan, npol_out)
    assert tp == 8192 // nchan and -(-nwin // tp) == 3 and nseg >= 2
    spans = cases.plfb_bin_segments(bins, wps)
    assert any(lo != hi for lo, hi in spans.values()), "no bin spans segments: k_plfb_combine would not run"
    assert any(lo == hi for lo, hi in spans.values()), "no bin inside a segment: nothing would be added to the profile directly"
