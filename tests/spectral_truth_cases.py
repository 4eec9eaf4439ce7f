"""Seeded noise through EVERY instantiation of the two transform-detect-add kernels (csrc/plfb.hip, csrc/bandpass.hip) that their pick
tables can return, with a float64 truth of every bin: tests/test_gpu_spectral_truth.py runs the cases on the device,
tests/test_spectral_truth_cases_host.py checks without one what the cases claim to reach.  Built without a device.

The tone cases of bandpass_cases.py and plfb_cases.py leave every bin but 0 and C / 2 at zero, and spectral_sums_cases.py compares the
kernels with their own earlier output; here every bin of every part is non-zero and different, and the answer is independent: the
numpy restatements rfi_reference.bandpass_loop and plfb_reference.plfb_loop, parts and windows in strict time order, once in float64
(the truth) and once in float32 (the error figure a correct single-precision sum may have).

Bandpass: max(2 Tp + 1, 64) parts, Tp = 8192 / C per workgroup tile, one more where that count would fill its last tile (C = 512 ..
4096: 65), so that every case has at least three tiles and the last tile holds one part; then half a transform of trailing samples
that must not be read.  PLFB: max(2 Tp + 1, 50) windows one sample apart over five phase bins.  SEVERAL: 256 Tp + 1 parts or
windows of one input channel, 257 tiles in 129 segments of two tiles, the last of one: the register sums carried across the tile
loop and its barrier.

The polarisation forms of one (kernel, form, ndim, C, npol_in) share their data and their references: the restatements compute PP
and QQ of four products exactly as they compute the two products of (2, 2)."""
import functools

import numpy as np

import plfb_reference as pr
import rfi_reference as rr
from bandpass_cases import RAW_SCALE
from spectral_sums_cases import plfb_bins

SIZES = tuple(1 << logc for logc in range(1, 14))
SEVERAL_SIZES = (512, 8192)
FORM = {"float": 0, "generic": 1, "caspsr": 2}                  # the FORM argument of k_bandpass
BANDPASS_NCHAN_IN = {"float": 2, "generic": 3, "caspsr": 1}
PLFB_NCHAN_IN, PLFB_NBIN = 2, 5

# (form, ndim, resolution, npol_in, npol_out, several)
BANDPASS = ([(f, d, c, pi, po, False) for f in ("float", "generic") for c in SIZES for d in (1, 2) for pi, po in ((1, 1), (2, 2), (2, 4))] +
            [("caspsr", 1, c, 2, po, False) for c in SIZES for po in (2, 4)] +
            [("float", d, c, 2, 4, True) for c in SEVERAL_SIZES for d in (1, 2)])
# (ndim, nchan, npol_in, npol_out, several)
PLFB = ([(d, c, pi, po, False) for c in SIZES for d in (1, 2) for pi, po in ((2, 1), (1, 1), (2, 2), (2, 4))] +
        [(d, c, 2, 4, True) for c in SEVERAL_SIZES for d in (1, 2)])

BANDPASS_IDS = ["bandpass-%s-ndim%d-res%d-pol%dto%d%s" % (c[:5] + ("-several" if c[5] else "",)) for c in BANDPASS]
PLFB_IDS = ["plfb-ndim%d-nchan%d-pol%dto%d%s" % (c[:4] + ("-several" if c[4] else "",)) for c in PLFB]


def _seed(*key):
    return [ord(ch) for ch in repr(key)]


def bandpass_nchan_in(form, several):
    return 1 if several else BANDPASS_NCHAN_IN[form]


def bandpass_parts(res, several):
    tp = 8192 // res
    if several:
        return 256 * tp + 1
    npart = max(2 * tp + 1, 64)
    return npart + 1 if tp > 1 and npart % tp == 0 else npart


@functools.lru_cache(maxsize=2)
def bandpass_data(form, ndim, res, npol_in, several):
    """(data, ndat): float rows float32 [nchan_in][npol_in][ndat * ndim] whose trailing half transform is NaN and counted in ndat; or
    the byte block (uint8) whose trailing half transform is the code -128 and lies behind ndat"""
    rng = np.random.default_rng(_seed("bandpass", form, ndim, res, npol_in, several))
    nchan_in = bandpass_nchan_in(form, several)
    nsamp_fft = res * (2 if ndim == 1 else 1)
    nbody = bandpass_parts(res, several) * nsamp_fft
    if form == "float":
        ndat = nbody + nsamp_fft // 2
        rows = np.full((nchan_in, npol_in, ndat * ndim), np.nan, dtype=np.float32)
        rows[:, :, :nbody * ndim] = rng.standard_normal((nchan_in, npol_in, nbody * ndim))
        return rows, ndat
    nbuf = nbody + nsamp_fft // 2
    if form == "caspsr":
        nbuf += (-nbuf) % 4                                                         # whole groups of 4 + 4 bytes
    codes = np.full((nchan_in, npol_in, nbuf, ndim), -128, dtype=np.int8)
    codes[:, :, :nbody] = rng.integers(0, 256, (nchan_in, npol_in, nbody, ndim), dtype=np.uint8).view(np.int8)
    return rr.encode_raw(codes, form), nbody


def bandpass_rows(form, ndim, res, npol_in, several):
    """what the references are given: the float rows with their trailing samples (ndat is the rows' length), or the ndat samples
    of the decoded block"""
    data, ndat = bandpass_data(form, ndim, res, npol_in, several)
    if form == "float":
        return data
    return rr.decode_raw(data, form, bandpass_nchan_in(form, several), npol_in, ndim, RAW_SCALE, np.float32)[:, :, :ndat * ndim]


@functools.lru_cache(maxsize=None)
def _bandpass_references(form, ndim, res, npol_in, several):
    rows = bandpass_rows(form, ndim, res, npol_in, several)
    npol_out = 4 if npol_in == 2 else 1
    ref = rr.bandpass_loop(rows, ndim, res, npol_out, np.float64)
    f32 = rr.bandpass_loop(rows, ndim, res, npol_out, np.float32)
    assert ref.dtype == np.float64 and f32.dtype == np.float32
    ref.setflags(write=False)
    f32.setflags(write=False)
    return ref, f32


def bandpass_references(index):
    """(float64 truth, float32 restatement) [npol_out][nchan_in][resolution] of case `index`"""
    form, ndim, res, npol_in, npol_out, several = BANDPASS[index]
    ref, f32 = _bandpass_references(form, ndim, res, npol_in, several)
    return ref[:npol_out], f32[:npol_out]


def bandpass_power(ref):
    """[1][nchan_in][resolution]: the total power of every bin, PP + QQ where both exist"""
    return (ref[0] + ref[1] if ref.shape[0] >= 2 else ref[0])[None]


def plfb_windows(nchan, several):
    tp = 8192 // nchan
    return 256 * tp + 1 if several else max(2 * tp + 1, 50)


@functools.lru_cache(maxsize=2)
def plfb_data(ndim, nchan, npol_in, several):
    """(rows float32 [nchan_in][npol_in][ndat * ndim], starts uint64, bins uint32, ndat): windows one sample apart, the last ending
    on the last sample"""
    rng = np.random.default_rng(_seed("plfb", ndim, nchan, npol_in, several))
    nwin = plfb_windows(nchan, several)
    starts = np.arange(nwin, dtype=np.uint64)
    ndat = nwin - 1 + nchan * (2 if ndim == 1 else 1)
    rows = rng.standard_normal((1 if several else PLFB_NCHAN_IN, npol_in, ndat * ndim)).astype(np.float32)
    return rows, starts, plfb_bins(nwin), ndat


@functools.lru_cache(maxsize=None)
def _plfb_references(ndim, nchan, npol_in, several, npol_out):
    rows, starts, bins, _ndat = plfb_data(ndim, nchan, npol_in, several)
    ref = pr.plfb_loop(rows, ndim, nchan, npol_out, PLFB_NBIN, starts, bins, np.float64)
    f32 = pr.plfb_loop(rows, ndim, nchan, npol_out, PLFB_NBIN, starts, bins, np.float32)
    assert ref.dtype == np.float64 and f32.dtype == np.float32
    ref.setflags(write=False)
    f32.setflags(write=False)
    return ref, f32


def plfb_references(index):
    """(float64 truth, float32 restatement) [nchan_in * nchan][npol_out][nbin] of case `index`; (2, 1) adds both polarisations into
    one sum as the reference does and has references of its own"""
    ndim, nchan, npol_in, npol_out, several = PLFB[index]
    ref, f32 = _plfb_references(ndim, nchan, npol_in, several, 1 if npol_out == 1 else 4)
    return ref[:, :npol_out], f32[:, :npol_out]


def plfb_power(ref):
    """[nchan_out][1][nbin]"""
    return (ref[:, 0] + ref[:, 1] if ref.shape[1] >= 2 else ref[:, 0])[:, None]


def figures(got, ref, power):
    """(max |got - ref| / max |ref| over the whole array, max over every product and bin of |got - ref| / that bin's total power)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return err.max() / np.abs(ref).max(), (err / power).max()
