"""The passband kernels on the device (csrc/bandpass.hip) against the CPU restatement of Bandpass.C:122-162 (tests/rfi_reference.py):
exact data bit for bit at every transform length, polarisation form, input form and part count that changes the path; Gaussian
rows within four times the error of the float32 strict-order restatement."""
import numpy as np
import pytest

from bandpass_cases import EXACT, IDS, NOISE, RAW_SCALE, SENTINEL_UNITS, exact_case, noise_case, part_counts
import dspsr_amd
from dspsr_amd import _lib

pytestmark = pytest.mark.gpu

LAYOUT = {"generic": _lib.RAW_GENERIC, "caspsr": _lib.RAW_CASPSR}


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _device_rows(rows, pad):
    """the rows inside a NaN-filled buffer with one spare polarisation row and `pad` spare floats per row, at an odd float offset:
    padded chan_stride and pol_stride, nothing readable around the rows"""
    import torch
    nchan_in, npol_in, n = rows.shape
    buf = torch.full((nchan_in, npol_in + 1, n + pad + 1), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :npol_in, 1:1 + n]
    view.copy_(torch.from_numpy(rows.astype(np.float32)))
    assert view.data_ptr() % 8 == 4
    return buf, view


def _prefill(ctx, eng, value):
    host = np.full(eng.shape, value, dtype=np.float32)
    code = _lib.lib.dspsr_amd_copy(ctx.handle, eng.get_pass_ptr(), host.ctypes.data, host.nbytes, _lib.H2D)
    assert code == _lib.OK
    ctx.synchronize()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("index", range(len(EXACT)), ids=IDS)
def test_exact_rows_bit_for_bit(ctx, index):
    import torch
    form, ndim, res, npol_in, npol_out, nchan_in, _tone, _big = EXACT[index]
    eng = dspsr_amd.BandpassEngine(ctx)
    eng.set_shape(nchan_in, npol_in, ndim, res, npol_out)
    assert not eng.synch().any() and eng.integration_samples == 0       # a new shape starts from zero
    nsamp_fft = res * (2 if ndim == 1 else 1)
    sentinel = float(SENTINEL_UNITS * res * res)
    for npart in part_counts(index):
        data, ndat, ref = exact_case(index, npart)
        if form == "float":
            buf, view = _device_rows(data, pad=5 + 2 * index)
            add = lambda: eng.accumulate(view, ndat)
        else:
            dev = torch.from_numpy(data).cuda()
            add = lambda: eng.accumulate_raw(dev, ndat, LAYOUT[form], RAW_SCALE)
        # two calls onto a sentinel: the result is added to what is there
        eng.zero()
        _prefill(ctx, eng, sentinel)
        add()
        got = eng.synch()
        assert np.array_equal(_bits(got), _bits((ref + sentinel).astype(np.float32))), npart
        assert eng.integration_samples == npart * nsamp_fft                                  # the trailing samples are not counted
        add()
        assert np.array_equal(_bits(eng.synch()), _bits((2 * ref + sentinel).astype(np.float32))), npart
        assert eng.integration_samples == 2 * npart * nsamp_fft
        # zero clears the passband; the same call gives the same bits
        eng.zero()
        assert not eng.synch().any() and eng.integration_samples == 0
        add()
        once = eng.synch()
        assert np.array_equal(_bits(once), _bits(ref.astype(np.float32))), npart
        eng.zero()
        add()
        assert np.array_equal(_bits(eng.synch()), _bits(once))
        if form == "float":
            assert bool(buf.isnan().sum() == buf.numel() - np.isfinite(data).sum())         # the input is only read
    eng.close()


def test_refusals_launch_nothing(ctx):
    """the C-ABI's refusals through the engine: an error with the limit's name, and the passband as it was"""
    import torch
    eng = dspsr_amd.BandpassEngine(ctx)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="no shape"):
        eng.accumulate(torch.zeros((1, 2, 64), device="cuda"), 64)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="no shape"):
        eng.synch()
    for args, text in (((1, 2, 1, 24, 2), "resolution=24 must be a power of two"), ((1, 2, 1, 16384, 2), "resolution=16384"),
                       ((1, 2, 4, 16, 2), "detected input is not built"), ((1, 1, 1, 16, 4), "npol_out=4 must be npol_in=1"),
                       ((1, 2, 1, 0, 2), "number of output frequency channels == 0")):
        with pytest.raises(dspsr_amd.DspsrAmdError, match=text):
            eng.set_shape(*args)
    eng.set_shape(1, 2, 1, 16, 4)
    rows = torch.ones((1, 2, 64), device="cuda")
    raw = torch.zeros(256, dtype=torch.int8, device="cuda")
    _prefill(ctx, eng, 3.0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="error ndat=31 < nfft=32"):
        eng.accumulate(rows, 31)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="stride shorter than the row"):
        eng.accumulate(rows, 65)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="DSPSR_AMD_RAW_UWB16"):
        eng.accumulate_raw(raw, 64, _lib.RAW_UWB16, 1.0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="starts on an 8-byte group"):
        eng.accumulate_raw(raw[4:], 64, _lib.RAW_CASPSR, 1.0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="unknown raw_layout 9"):
        eng.accumulate_raw(raw, 64, 9, 1.0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="ndat=.* >= 2.31"):
        eng.accumulate_raw(raw, 1 << 31, _lib.RAW_GENERIC, 1.0)
    assert np.array_equal(eng.synch(), np.full((4, 1, 16), 3.0, np.float32)) and eng.integration_samples == 0
    eng.set_shape(3, 2, 1, 16, 2)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="DSPSR_AMD_RAW_CASPSR is one channel"):
        eng.accumulate_raw(raw, 32, _lib.RAW_CASPSR, 1.0)
    assert not eng.synch().any()
    eng.close()


@pytest.mark.parametrize("ndim,res,npart", NOISE, ids=["ndim%d-res%d-parts%d" % c for c in NOISE])
def test_noise_within_four_times_the_float32_restatement(ctx, ndim, res, npart):
    rows, ndat, ref, e_f32 = noise_case(ndim, res, npart)
    buf, view = _device_rows(rows, pad=4)
    eng = dspsr_amd.BandpassEngine(ctx)
    eng.set_shape(2, 2, ndim, res, 4)
    eng.accumulate(view, ndat)
    got = eng.synch().astype(np.float64)
    eng.close()
    e_gpu = np.abs(got - ref).max() / np.abs(ref).max()
    print("bandpass noise ndim=%d resolution=%d parts=%d e_gpu=%.3e e_f32=%.3e ratio=%.2f" % (ndim, res, npart, e_gpu, e_f32, e_gpu / e_f32))
    assert e_f32 > 0
    assert e_gpu <= 4 * e_f32, "e_gpu %.3e > 4 x e_f32 %.3e" % (e_gpu, e_f32)
