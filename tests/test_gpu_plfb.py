"""The phase-locked filterbank on the device (csrc/plfb.hip) against the CPU restatement of PhaseLockedFilterbank.C:254-297
(tests/plfb_reference.py): exact data bit for bit at every transform length, polarisation form, stride and window count per
bin that changes the path; Gaussian rows within four times the error of the float32 strict-order restatement."""
import numpy as np
import pytest

from plfb_cases import EXACT, IDS, NOISE, SENTINEL_UNITS, exact_case, noise_case
import dspsr_amd
from dspsr_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _device_rows(rows, ndim, pad):
    """the rows inside a NaN-filled buffer with one spare polarisation row and `pad` spare floats per row: padded chan_stride
    and pol_stride, nothing readable around the rows"""
    import torch
    nchan_in, npol_in, n = rows.shape
    length = n + pad + ((n + pad) % 2)
    buf = torch.full((nchan_in, npol_in + 1, length + 2), float("nan"), dtype=torch.float32, device="cuda")
    off = 2 if ndim == 2 else 1                             # Nyquist rows: any float address
    view = buf[:, :npol_in, off:off + n]
    view.copy_(torch.from_numpy(rows.astype(np.float32)))
    return buf, view


def _prefill(ctx, eng, value):
    host = np.full(eng.shape, value, dtype=np.float32)
    code = _lib.lib.dspsr_amd_copy(ctx.handle, eng.get_profile_ptr(), host.ctypes.data, host.nbytes, _lib.H2D)
    assert code == _lib.OK
    ctx.synchronize()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("index", range(len(EXACT)), ids=IDS)
def test_exact_rows_bit_for_bit(ctx, index):
    ndim, nchan, npol_in, npol_out, nchan_in, nbin, _tone_kind, _rot, _overlap = EXACT[index]
    rows, starts, bins, ref, ndat = exact_case(index)
    buf, view = _device_rows(rows, ndim, pad=6 + 2 * index)
    eng = dspsr_amd.PhaseLockedFilterbankEngine(ctx)
    eng.set_shape(nchan_in, npol_in, ndim, nchan, npol_out, nbin)
    assert not eng.synch().any()                            # a new shape starts from zero
    # one call onto a sentinel: bins with windows gain their sums, the others keep the sentinel's bits
    sentinel = float(SENTINEL_UNITS * nchan * nchan)
    _prefill(ctx, eng, sentinel)
    eng.accumulate(view, ndat, starts, bins)
    got = eng.synch()
    want = (ref + sentinel).astype(np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    empty = np.setdiff1d(np.arange(nbin), bins)
    assert np.array_equal(_bits(got[:, :, empty]), _bits(np.full((nchan_in * nchan, npol_out, len(empty)), sentinel, np.float32)))
    # zero clears the profile; the same call twice gives the same bits
    eng.zero()
    assert not eng.synch().any()
    eng.accumulate(view, ndat, starts, bins)
    once = eng.synch()
    assert np.array_equal(_bits(once), _bits(ref.astype(np.float32)))
    eng.zero()
    eng.accumulate(view, ndat, starts, bins)
    assert np.array_equal(_bits(eng.synch()), _bits(once))
    # two calls equal one call with both lists; the profile accumulates over calls
    cut = len(starts) // 3 + 1
    eng.zero()
    eng.accumulate(view, ndat, starts[:cut], bins[:cut])
    eng.accumulate(view, ndat, starts[cut:], bins[cut:])
    assert np.array_equal(_bits(eng.synch()), _bits(once))
    eng.accumulate(view, ndat, starts, bins)
    assert np.array_equal(_bits(eng.synch()), _bits((2 * ref).astype(np.float32)))
    assert bool(buf.isnan().sum() == buf.numel() - np.isfinite(rows).sum())          # the input is only read
    eng.close()


def test_refusals_launch_nothing(ctx):
    """the C-ABI's refusals through the engine: an error with the message, and the profile as it was"""
    import torch
    eng = dspsr_amd.PhaseLockedFilterbankEngine(ctx)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="no shape"):
        eng.accumulate(torch.zeros((1, 2, 64), device="cuda"), 32, [0], [0])
    with pytest.raises(dspsr_amd.DspsrAmdError, match=r"nchan=24 must be a power of two"):
        eng.set_shape(1, 2, 2, 24, 4, 8)
    eng.set_shape(1, 2, 2, 16, 4, 8)
    rows = torch.ones((1, 2, 64), device="cuda")
    _prefill(ctx, eng, 3.0)
    for starts, bins, text in (([0, 17], [0, 1], r"idat_start=17 \+ ndat_fft=16 > ndat=32"), ([0, 16], [0, 8], "bin=8 >= nbin=8"),
                               ([16, 0], [0, 1], "out of time order")):
        with pytest.raises(dspsr_amd.DspsrAmdError, match=text):
            eng.accumulate(rows, 32, starts, bins)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="8-byte aligned"):
        eng.accumulate(rows[:, :, 1:], 31, [0], [0])
    eng.accumulate(rows, 32, [], [])                        # no window: nothing to do
    assert np.array_equal(eng.synch(), np.full((16, 4, 8), 3.0, np.float32))
    eng.close()


@pytest.mark.parametrize("ndim,nchan", NOISE, ids=["ndim%d-nchan%d" % c for c in NOISE])
def test_noise_within_four_times_the_float32_restatement(ctx, ndim, nchan):
    rows, starts, bins, ref, ndat, e_f32 = noise_case(ndim, nchan)
    buf, view = _device_rows(rows, ndim, pad=4)
    eng = dspsr_amd.PhaseLockedFilterbankEngine(ctx)
    eng.set_shape(2, 2, ndim, nchan, 4, 5)
    eng.accumulate(view, ndat, starts, bins)
    got = eng.synch().astype(np.float64)
    eng.close()
    e_gpu = np.abs(got - ref).max() / np.abs(ref).max()
    print("plfb noise ndim=%d nchan=%d e_gpu=%.3e e_f32=%.3e ratio=%.2f" % (ndim, nchan, e_gpu, e_f32, e_gpu / e_f32))
    assert e_f32 > 0
    assert e_gpu <= 4 * e_f32, "e_gpu %.3e > 4 x e_f32 %.3e" % (e_gpu, e_f32)
