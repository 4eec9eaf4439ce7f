"""Every instantiation of k_bandpass (csrc/bandpass.hip) and k_plfb (csrc/plfb.hip) on seeded noise against a float64 reference of its
own (tests/spectral_truth_cases.py): the error over the whole array and the error of every bin relative to that bin's own power, each
within four times the same figure of the float32 strict-order restatement; the input only read; the same call the same bits; phase
bins without a window +0.0.  Every line printed ends in the ratio e_gpu / e_f32; profiles/HISTORY.md holds the table.

Open finding, PLFB bin by bin at nchan >= 256 (PLFB_OPEN).  The windows of a case start one sample apart, so the ten or more windows
of a phase bin are nearly one window: a bin's sum is ten times ONE |X[k]|^2 and not an average, and among thousands of bins some hold
1e-2 (nchan 256) to 2e-4 (nchan 8192) of the mean power.  There the quotient measures the transform's amplitude error against an
amplitude near zero.  One transformed window on the MI355X is off by 1.0e-7 (nchan 256) to 1.4e-7 (nchan 8192) of the rms amplitude,
bit for bit the same in both kernels, growing evenly with the length, Nyquist a fifth above Analytic; the float32 restatement by
2.8e-8.  A float64 spectrum with that much noise added gives the quotients measured: no defect.  Largest bin_gpu / bin_f32 per nchan
(all below 4 at nchan <= 128): 256: 4.2, 512: 4.8, 1024: 5.0, 2048: 10.9, 4096: 18.7, 8192: 27.1 -- (1, 1) of Nyquist rows every time,
the form with the fewest terms per bin.  At these lengths the bins are held to the tolerance the project holds the tile transform to
(amplitude rms 2e-6 sqrt(log2 2C), tests/test_gpu_plain.py) and not to a margin fitted to the kernel; the whole-array figure keeps
four times the restatement's at every length, and so does every Bandpass case and every several-tile case bin by bin."""
import math

import numpy as np
import pytest

import spectral_truth_cases as cases
from bandpass_cases import RAW_SCALE
import dspsr_amd
from dspsr_amd import _lib

pytestmark = pytest.mark.gpu

LAYOUT = {"generic": _lib.RAW_GENERIC, "caspsr": _lib.RAW_CASPSR}
MARGIN = 4                      # the project's margin over the float32 restatement (test_gpu_plfb.py, test_gpu_bandpass.py)
PLFB_OPEN = (256, 512, 1024, 2048, 4096, 8192)      # bin by bin above MARGIN with no defect found: see above


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _placed(rows, off, pad):
    """the rows inside a NaN-filled buffer with one spare polarisation row and spare floats per row, `off` floats into the row:
    padded chan_stride and pol_stride (both even), nothing readable around the rows"""
    import torch
    nchan_in, npol_in, n = rows.shape
    length = off + n + pad
    buf = torch.full((nchan_in, npol_in + 1, length + length % 2), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :npol_in, off:off + n]
    view.copy_(torch.from_numpy(rows))
    return buf, view


def transform_tolerance(c):
    """the rms amplitude error the project allows its tile transform (tests/test_gpu_plain.py), relative to the rms amplitude"""
    return 2e-6 * math.sqrt(math.log2(2 * c))


def _judge(name, got, ref, f32, power, open_tol=None, mean_power=None):
    """the four-times rule over the whole array and bin by bin.  open_tol (a length named as an open finding): bin by bin the transform's
    tolerance instead.  With amplitude errors d_w of rms open_tol * sigma on the n windows X_w of a bin of power P = sum |X_w|^2, a
    detected sum is off by at most 2 sqrt(P) sqrt(sum |d_w|^2) = 2 sqrt(P) open_tol sqrt(M), M = n sigma^2 the mean power of the bins
    (Cauchy-Schwarz; the cross products the same with both polarisations' power): the quotient is at most 2 open_tol sqrt(M / P).
    And, as the project words it for a detected sum, twice the tolerance relative to the array's maximum."""
    e_gpu, q_gpu = cases.figures(got, ref, power)
    e_f32, q_f32 = cases.figures(f32, ref, power)
    print("%s e_gpu=%.3e e_f32=%.3e bin_gpu=%.3e bin_f32=%.3e bin_ratio=%.2f ratio=%.2f" %
          (name, e_gpu, e_f32, q_gpu, q_f32, q_gpu / q_f32, e_gpu / e_f32))
    assert np.isfinite(got).all()
    assert e_f32 > 0 and q_f32 > 0
    assert e_gpu <= MARGIN * e_f32, "e_gpu %.3e > %d x e_f32 %.3e" % (e_gpu, MARGIN, e_f32)
    if open_tol is None:
        assert q_gpu <= MARGIN * q_f32, "a bin is off by %.3e of its own power > %d x %.3e" % (q_gpu, MARGIN, q_f32)
    else:
        assert e_gpu <= 2 * open_tol
        worst = (np.abs(got.astype(np.float64) - ref) / power / (2 * open_tol * np.sqrt(mean_power / power))).max()
        assert worst <= 1, "a bin is off by %.3g times what the transform's tolerance allows it" % worst


@pytest.mark.parametrize("index", range(len(cases.BANDPASS)), ids=cases.BANDPASS_IDS)
def test_bandpass_every_bin_against_float64(ctx, index):
    import torch
    form, ndim, res, npol_in, npol_out, several = cases.BANDPASS[index]
    data, ndat = cases.bandpass_data(form, ndim, res, npol_in, several)
    ref, f32 = cases.bandpass_references(index)
    eng = dspsr_amd.BandpassEngine(ctx)
    eng.set_shape(cases.bandpass_nchan_in(form, several), npol_in, ndim, res, npol_out)
    if form == "float":
        buf, view = _placed(data, 1, 4 + index % 3)                            # an odd float address
        assert view.data_ptr() % 8 == 4
        add = lambda: eng.accumulate(view, ndat)
    else:
        buf = torch.from_numpy(data).cuda()
        add = lambda: eng.accumulate_raw(buf, ndat, LAYOUT[form], RAW_SCALE)
    before = buf.clone()
    assert not eng.synch().any()
    add()
    got = eng.synch()
    eng.zero()
    add()
    again = eng.synch()
    nsamp_fft = res * (2 if ndim == 1 else 1)
    assert eng.integration_samples == cases.bandpass_parts(res, several) * nsamp_fft
    eng.close()
    _judge(cases.BANDPASS_IDS[index], got, ref, f32, cases.bandpass_power(ref))
    assert np.array_equal(_bits(again), _bits(got))                            # the same call, the same bits
    # the input is only read: the same bytes, the same NaN count
    assert torch.equal(buf.view(torch.uint8).view(-1), before.view(torch.uint8).view(-1))
    if form == "float":
        assert int(buf.isnan().sum()) == buf.numel() - int(np.isfinite(data).sum())


@pytest.mark.parametrize("index", range(len(cases.PLFB)), ids=cases.PLFB_IDS)
def test_plfb_every_bin_against_float64(ctx, index):
    import torch
    ndim, nchan, npol_in, npol_out, several = cases.PLFB[index]
    rows, starts, bins, ndat = cases.plfb_data(ndim, nchan, npol_in, several)
    ref, f32 = cases.plfb_references(index)
    nbin = cases.PLFB_NBIN
    buf, view = _placed(rows, 2 if ndim == 2 else 1, 4 + index % 3)            # Analytic rows 8-byte aligned, Nyquist rows at any float
    assert view.data_ptr() % 8 == (0 if ndim == 2 else 4)
    eng = dspsr_amd.PhaseLockedFilterbankEngine(ctx)
    eng.set_shape(rows.shape[0], npol_in, ndim, nchan, npol_out, nbin)
    assert not eng.synch().any()
    eng.accumulate(view, ndat, starts, bins)
    got = eng.synch()
    eng.zero()
    eng.accumulate(view, ndat, starts, bins)
    again = eng.synch()
    # the same windows in a profile of two more phase bins, every bin one further on: the same sorted list and the same cut, so the
    # same bits, and the first and the last bin receive no window
    eng.set_shape(rows.shape[0], npol_in, ndim, nchan, npol_out, nbin + 2)
    eng.accumulate(view, ndat, starts, bins + np.uint32(1))
    wide = eng.synch()
    eng.close()
    power = cases.plfb_power(ref)
    if nchan in PLFB_OPEN and not several:
        _judge(cases.PLFB_IDS[index], got, ref, f32, power, transform_tolerance(nchan), power.mean(axis=0, keepdims=True))
    else:
        _judge(cases.PLFB_IDS[index], got, ref, f32, power)
    assert np.array_equal(_bits(again), _bits(got))                            # the same call, the same bits
    empty = np.setdiff1d(np.arange(nbin), bins)                                # (none of the five: every case has 50 windows or more)
    assert not _bits(got[:, :, empty]).any()
    assert not _bits(wide[:, :, [0, nbin + 1]]).any()                          # bins without a window stay +0.0
    assert np.array_equal(_bits(wide[:, :, 1:nbin + 1]), _bits(got))
    assert int(buf.isnan().sum()) == buf.numel() - rows.size                   # the input is only read
    assert torch.equal(view.cpu(), torch.from_numpy(rows))
