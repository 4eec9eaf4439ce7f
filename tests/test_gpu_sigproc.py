"""SIGPROC spectra on the device: the unpacker k_unpack_sigproc bit for bit against the restatement of tests/sigproc_cases.py
(SigProcUnpacker.C:98-153), for every sample size and number of polarisations, at spectra that start on every byte offset the
sample size allows, on rows cut from sentinel buffers at addresses that are and are not 16-byte aligned; the empty call and every
refusal of the C-ABI."""
import numpy as np
import pytest

import sigproc_cases as sc
from device_buffers import SENTINEL, OutputLayout, describe_float, place_parts, sentinel_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


@pytest.mark.parametrize("nbit", sc.NBITS)
def test_unpack_sigproc_bit_for_bit(gpu, nbit):
    """every case of sigproc_cases.kernel_cases: the rows hold the restatement's bits (nbit 32: NaN, infinities, negative zero and a
    denormal among them) and no other float of the buffer is touched.  The raw buffer starts `off` bytes into its allocation and
    ends with the last byte of the last spectrum."""
    dspsr_amd, ctx = gpu
    for nchan, npol, ndat, off, row_offset, row_pad in sc.kernel_cases(nbit):
        what = "nbit %d nchan %d npol %d ndat %d raw offset %d row offset %d pad %d" % (nbit, nchan, npol, ndat, off, row_offset, row_pad)
        raw = sc.random_spectra(nbit, nchan, npol, ndat)
        want = sc.unpack_fpt(raw, nbit, nchan, npol, ndat)
        alloc = torch.zeros(off + raw.size, dtype=torch.uint8, device="cuda")
        d_raw = alloc[off:]
        d_raw.copy_(torch.from_numpy(raw))
        assert alloc.data_ptr() % 16 == 0 and d_raw.data_ptr() % 16 == off and d_raw.numel() == ndat * sc.spectrum_bytes(nbit, nchan, npol)
        lay = OutputLayout(nchan, npol, ndat, offset=row_offset, row_pad=row_pad)
        buf, rows = sentinel_rows(lay)
        dspsr_amd.unpack_sigproc_fpt(ctx, d_raw, rows, nbit, nchan, npol, ndat)
        ctx.synchronize()
        got = buf.cpu().numpy()
        exp = place_parts(lay, np.full(lay.size, SENTINEL, np.int32), want.view(np.int32).reshape(nchan, npol, 1, ndat), 0)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, "%s: %d floats differ, the first: %s (got %#x, expected %#x)" % (
            what, bad.size, describe_float(lay, int(bad[0]), 1, 0, ndat), got[bad[0]] & 0xffffffff, exp[bad[0]] & 0xffffffff)


def test_unpack_sigproc_empty_call_and_refusals(gpu):
    dspsr_amd, ctx = gpu
    from dspsr_amd import _lib
    nchan, npol, ndat = 24, 2, 100
    block = torch.from_numpy(sc.random_spectra(32, nchan, npol, ndat)).cuda()
    lay = OutputLayout(nchan, npol, ndat)
    buf, rows = sentinel_rows(lay)
    ocs, ops = rows.stride(0), rows.stride(1)
    ptr = block.data_ptr()

    def call(raw_ptr=ptr, nbit=8, nchan_=nchan, npol_=npol, n=ndat, out_ptr=rows.data_ptr(), ocs_=ocs, ops_=ops, ctx_=ctx.handle):
        return _lib.lib.dspsr_amd_unpack_sigproc_fpt(ctx_, raw_ptr, nbit, nchan_, npol_, n, out_ptr, ocs_, ops_)

    def message():
        return _lib.lib.dspsr_amd_last_error(ctx.handle).decode()

    assert call(n=0) == _lib.OK                                                          # ndat = 0: nothing to do
    assert call(n=0, raw_ptr=None, out_ptr=None) == _lib.OK
    assert call(ctx_=None) == _lib.EINVAL
    for bad in (0, 3, 5, 7, 12, 24, 64):
        assert call(nbit=bad) == _lib.EINVAL and "nbit" in message()
    assert call(nchan_=0) == _lib.EINVAL and "nchan" in message()
    for bad in (0, 3, 5, 8):
        assert call(npol_=bad) == _lib.EINVAL and "npol" in message()
    for nbit, bad in ((1, 4), (1, 12), (2, 2), (2, 6), (4, 1), (4, 3)):
        assert call(nbit=nbit, nchan_=bad) == _lib.EINVAL and "whole bytes" in message()
    assert call(nbit=16, raw_ptr=ptr + 1) == _lib.EINVAL and "raw_dev" in message()
    for skew in (1, 2, 3):
        assert call(nbit=32, raw_ptr=ptr + skew) == _lib.EINVAL and "raw_dev" in message()
    assert call(n=1 << 61) == _lib.EINVAL and "too large" in message()
    assert call(ops_=ndat - 1) == _lib.EINVAL and "overlap" in message()
    assert call(ocs_=ops + ndat - 1) == _lib.EINVAL and "overlap" in message()
    assert call(npol_=1, ocs_=ndat - 1) == _lib.EINVAL and "overlap" in message()
    assert call(raw_ptr=None) == _lib.EINVAL and "null" in message()
    assert call(out_ptr=None) == _lib.EINVAL and "null" in message()
    ctx.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all(), "a refused or empty call wrote"
    # one polarisation, one channel: the strides play no part
    assert call(nchan_=1, npol_=1, ocs_=0, ops_=0) == _lib.OK
    # the Python mirror refuses a block that is too short and rows of another shape before the library is called
    with pytest.raises(dspsr_amd.DspsrAmdError, match="bytes"):
        dspsr_amd.unpack_sigproc_fpt(ctx, block[:10], rows, 8, nchan, npol, ndat)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="rows"):
        dspsr_amd.unpack_sigproc_fpt(ctx, block, rows, 8, nchan, 1, ndat)
    ctx.synchronize()
