"""What tests/test_gpu_spectral_truth.py rests on, checked without a device: the cases of tests/spectral_truth_cases.py are exactly the
instantiations of k_bandpass and k_plfb in the shipped library; every case cuts into the tiles and segments it is there for; the
float64 truth is non-zero at every bin (the property the tone cases lack); the float32 restatement's error figures are finite and not
zero; what must not be read is NaN, or the code -128 behind ndat.  CPU only."""
import re
import subprocess

import numpy as np
import pytest

import plfb_reference as pr
import rfi_reference as rr
import spectral_sums_cases as sums
import spectral_truth_cases as cases
import dspsr_amd
from dspsr_amd import _lib
from test_kernel_resources import LIB, _code_objects, _kernels

RAW = {"float": -1, "generic": _lib.RAW_GENERIC, "caspsr": _lib.RAW_CASPSR}
B_INDEX, P_INDEX = range(len(cases.BANDPASS)), range(len(cases.PLFB))


@pytest.fixture(scope="module")
def kernels():
    """the demangled kernel names of the shipped library, read as tests/test_bandpass_kernel_resources.py reads them"""
    ks = {}
    for co in _code_objects(open(LIB, "rb").read()):
        ks.update(_kernels(co))
    dem = subprocess.run(["c++filt"], input="\n".join(sorted(ks)), capture_output=True, text=True).stdout.splitlines()
    return {d.split("(")[0].replace("void dspsr_amd::", "").replace("dspsr_amd::", "") for d in dem}


def _instantiations(kernels, name):
    """the template arguments of every `name<...>` in the library"""
    found = [re.fullmatch(name + r"<([-0-9, ]+)>", k) for k in kernels]
    return {tuple(int(v) for v in m.group(1).split(",")) for m in found if m}


def test_one_case_per_instantiation_and_one_instantiation_per_case(kernels):
    logc = {1 << l: l for l in range(1, 14)}
    assert len(set(cases.BANDPASS_IDS)) == len(cases.BANDPASS) == 182 + 4 and len(set(cases.PLFB_IDS)) == len(cases.PLFB) == 104 + 4
    want = {(logc[c[2]], c[1], c[4], cases.FORM[c[0]]) for c in cases.BANDPASS}
    assert len(want) == 182 and _instantiations(kernels, "k_bandpass") == want
    want = {(logc[c[1]], c[0], c[3]) for c in cases.PLFB}
    assert len(want) == 78 and _instantiations(kernels, "k_plfb") == want
    # the output forms of k_plfb<.., 1>: the sum of two polarisations and one polarisation alone, at every length and ndim
    for pols in ((2, 1), (1, 1), (2, 2), (2, 4)):
        assert {(c[1], c[0]) for c in cases.PLFB if c[2:4] == pols and not c[4]} == {(n, d) for n in cases.SIZES for d in (1, 2)}
    # every ordinary case shares its references with its polarisation forms alone
    assert {c[:2] + c[3:5] for c in cases.BANDPASS if c[5]} == {("float", 1, 2, 4), ("float", 2, 2, 4)}
    assert {c[2] for c in cases.BANDPASS if c[5]} == {c[1] for c in cases.PLFB if c[4]} == {512, 8192}


@pytest.mark.parametrize("index", B_INDEX, ids=cases.BANDPASS_IDS)
def test_bandpass_case_tiles_segments_and_what_must_not_be_read(index):
    form, ndim, res, npol_in, npol_out, several = cases.BANDPASS[index]
    nchan_in = cases.bandpass_nchan_in(form, several)
    assert nchan_in == (1 if several or form == "caspsr" else 3 if form == "generic" else 2)
    dspsr_amd.bandpass_check_shape(nchan_in, npol_in, ndim, res, npol_out)
    data, ndat = cases.bandpass_data(form, ndim, res, npol_in, several)
    nsamp_fft = res * (2 if ndim == 1 else 1)
    npart, tp = ndat // nsamp_fft, 8192 // res
    assert npart == cases.bandpass_parts(res, several) and npart >= (256 * tp + 1 if several else max(2 * tp + 1, 64))
    assert data.nbytes <= (34 << 20 if several else 17 << 20)
    if form == "float":
        assert data.dtype == np.float32 and data.shape == (nchan_in, npol_in, ndat * ndim)
        body, tail = data[:, :, :npart * nsamp_fft * ndim], data[:, :, npart * nsamp_fft * ndim:]
        assert np.isfinite(body).all() and body.std() > 0.9
        assert ndat - npart * nsamp_fft == nsamp_fft // 2 and tail.size and np.isnan(tail).all()   # counted in ndat, never read
        # dense strides at an odd float address; the device test pads both strides
        cut = dspsr_amd.bandpass_check_input(nchan_in, npol_in, ndim, res, -1, 4, npol_in * ndat * ndim, ndat * ndim, ndat)
    else:
        assert data.dtype == np.uint8 and data.ndim == 1 and len(np.unique(data)) > 200
        assert ndat == npart * nsamp_fft                                                          # ndat ends before the trailing codes
        codes = rr.decode_raw(data, form, nchan_in, npol_in, ndim, 1.0).reshape(nchan_in, npol_in, -1, ndim) - 0.5
        assert codes.shape[2] >= ndat + nsamp_fft // 2 and (codes[:, :, ndat:] == -128).all() and codes[:, :, :ndat].std() > 70
        assert np.isfinite(cases.bandpass_rows(form, ndim, res, npol_in, several)).all()
        cut = dspsr_amd.bandpass_check_input(nchan_in, npol_in, ndim, res, RAW[form], 0, 0, 0, ndat)
    ntile = -(-npart // tp)
    assert cut[0] == tp and ntile >= 3 and npart - (ntile - 1) * tp == 1           # at least three tiles, the last holding one part
    if several:
        assert ntile == 257 and cut == (tp, 2, 129)                                # segments of two tiles, the last of one
    else:
        assert cut[2] >= 2


@pytest.mark.parametrize("index", P_INDEX, ids=cases.PLFB_IDS)
def test_plfb_case_windows_and_segments(index):
    ndim, nchan, npol_in, npol_out, several = cases.PLFB[index]
    nchan_in = 1 if several else cases.PLFB_NCHAN_IN
    dspsr_amd.plfb_check_shape(nchan_in, npol_in, ndim, nchan, npol_out, cases.PLFB_NBIN)
    rows, starts, bins, ndat = cases.plfb_data(ndim, nchan, npol_in, several)
    assert rows.dtype == np.float32 and rows.shape == (nchan_in, npol_in, ndat * ndim) and np.isfinite(rows).all() and rows.std() > 0.9
    dspsr_amd.plfb_check_windows(nchan_in, npol_in, ndim, nchan, cases.PLFB_NBIN, 8, npol_in * ndat * ndim, ndat * ndim, ndat, starts, bins)
    nwin, tp = len(starts), 8192 // nchan
    assert nwin == (256 * tp + 1 if several else max(2 * tp + 1, 50))
    assert np.array_equal(starts, np.arange(nwin)) and np.array_equal(bins, sums.plfb_bins(nwin))   # odd and even starts
    assert int(starts[-1]) + nchan * (2 if ndim == 1 else 1) == ndat                # the last window ends on the last sample
    assert set(bins.tolist()) == set(range(cases.PLFB_NBIN))
    got_tp, wps, nseg = sums.plfb_cut(nwin, nchan_in, nchan, npol_out)
    assert got_tp == tp and -(-nwin // tp) >= 3
    if several:
        assert -(-nwin // tp) == 257 and (wps, nseg) == (2 * tp, 129)
    spans = sums.plfb_bin_segments(bins, wps)
    assert nseg >= 2 and any(lo != hi for lo, hi in spans.values()), "no bin spans segments: k_plfb_combine would not run"


def test_plfb_bins_inside_one_segment_occur_too():
    inside = 0
    for ndim, nchan, npol_in, npol_out, several in cases.PLFB:
        nwin = cases.plfb_windows(nchan, several)
        _tp, wps, _nseg = sums.plfb_cut(nwin, 1 if several else cases.PLFB_NCHAN_IN, nchan, npol_out)
        inside += sum(lo == hi for lo, hi in sums.plfb_bin_segments(sums.plfb_bins(nwin), wps).values())
    assert inside > 0


def _check_figures(ref, f32, power):
    assert ref.dtype == np.float64 and f32.dtype == np.float32 and ref.shape == f32.shape
    assert np.isfinite(ref).all() and (power > 0).all()                            # every bin has power
    e_f32, q_f32 = cases.figures(f32, ref, power)
    assert np.isfinite(e_f32) and e_f32 > 0 and np.isfinite(q_f32) and q_f32 > 0
    assert e_f32 < 1e-4 and q_f32 < 1e-4                                           # a single-precision figure
    return e_f32, q_f32


@pytest.mark.parametrize("index", B_INDEX, ids=cases.BANDPASS_IDS)
def test_bandpass_truth_is_general_and_the_float32_figures_are_not_zero(index):
    form, ndim, res, npol_in, npol_out, _several = cases.BANDPASS[index]
    ref, f32 = cases.bandpass_references(index)
    assert ref.shape == (npol_out, cases.bandpass_nchan_in(form, _several), res)
    _check_figures(ref, f32, cases.bandpass_power(ref))
    # every product at every general bin is non-zero and the bins differ: the Hermitian split A + w^k B, the mirror plane, the bin
    # order and the cross products have something to get wrong (Im P* Q of the real bin 0 of Nyquist rows is 0 by definition)
    k = np.arange(res) if ndim == 2 else np.setdiff1d(np.arange(res), (0, res // 2))
    if len(k):
        assert (ref[:, :, k] != 0).all() and len(np.unique(ref[0, 0, k])) == len(k)
    assert not ref.flags.writeable and not f32.flags.writeable                    # shared between the tests, read-only


@pytest.mark.parametrize("index", P_INDEX, ids=cases.PLFB_IDS)
def test_plfb_truth_is_general_and_the_float32_figures_are_not_zero(index):
    ndim, nchan, npol_in, npol_out, several = cases.PLFB[index]
    ref, f32 = cases.plfb_references(index)
    assert ref.shape == ((1 if several else cases.PLFB_NCHAN_IN) * nchan, npol_out, cases.PLFB_NBIN)
    _check_figures(ref, f32, cases.plfb_power(ref))
    k = np.arange(nchan) if ndim == 2 else np.setdiff1d(np.arange(nchan), (0, nchan // 2))
    if len(k):
        assert (ref[k] != 0).all() and len(np.unique(ref[k, 0, 0])) == len(k)
    assert not ref.flags.writeable and not f32.flags.writeable


def test_shared_references_are_those_of_the_form_itself():
    """(2, 2) is the first two products of (2, 4), bit for bit, in both restatements: what lets the forms share"""
    for form, ndim in (("float", 1), ("generic", 2), ("caspsr", 1)):
        index = cases.BANDPASS.index((form, ndim, 64, 2, 2, False))
        rows = cases.bandpass_rows(form, ndim, 64, 2, False)
        for got, dtype in zip(cases.bandpass_references(index), (np.float64, np.float32)):
            assert np.array_equal(got, rr.bandpass_loop(rows, ndim, 64, 2, dtype))
    for ndim in (1, 2):
        index = cases.PLFB.index((ndim, 64, 2, 2, False))
        rows, starts, bins, _ndat = cases.plfb_data(ndim, 64, 2, False)
        for got, dtype in zip(cases.plfb_references(index), (np.float64, np.float32)):
            assert np.array_equal(got, pr.plfb_loop(rows, ndim, 64, 2, cases.PLFB_NBIN, starts, bins, dtype))
