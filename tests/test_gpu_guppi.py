"""GUPPI raw blocks on the device: the unpacker k_unpack_guppi bit for bit against the restatement of tests/guppi_cases.py, on rows
cut from sentinel buffers, at runs that are and are not 16-byte aligned; the empty call and every refusal; and the RAW_GUPPI form of
the engine's raw entry points against the float entry points on the restatement's rows, through the one-pass convolution (M = 1024)
and the three-pass one (M = 16384)."""
import ctypes as C

import numpy as np
import pytest

import guppi_cases as gc
from device_buffers import SENTINEL, OutputLayout, describe_float, place_parts, sentinel_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NBLK = 5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


def _windows(bn):
    return [(0, bn), (0, 2 * bn + 1), (1, bn - 1), (bn - 1, 2), (37, 1000)]          # (first, ndat)


# (block_nsamp, OVERLAP, bytes between the data sections beyond nchan * chan_stride, bytes the raw tensor starts into its allocation)
CASES = [(bn, ovl, 0, 0) for bn, ovl in gc.GEOMETRIES] + [(259, 5, 72, 0), (256, 0, 0, 4), (255, 2, 0, 4)]


@pytest.mark.parametrize("bn,ovl,gap,skew", CASES)
@pytest.mark.parametrize("npol", [1, 2])
@pytest.mark.parametrize("nchan", [1, 3, 64])
def test_unpack_guppi_bit_for_bit(gpu, nchan, npol, bn, ovl, gap, skew):
    """every window at every row offset 0-3 (floats past a 256-byte boundary), the paddings 0, 1 and 3 in turn: the rows hold the
    restatement's bits and no other float of the buffer is touched.  The block is random everywhere -- overlap samples and the bytes
    between data sections included -- so a byte read from the wrong place shows."""
    dspsr_amd, ctx = gpu
    cs = gc.chan_stride_of(bn, ovl, npol)
    bs = nchan * cs + gap
    assert gap % (2 * npol) == 0 and skew % (2 * npol) == 0
    block = gc.random_blocks(NBLK * bs, seed=nchan + npol + bn)
    stream = gc.stream_from_blocks(block, nchan, npol, bn, ovl, chan_stride=cs, block_stride=bs)
    alloc = torch.zeros(skew + block.size, dtype=torch.int8, device="cuda")
    d_block = alloc[skew:]
    d_block.copy_(torch.from_numpy(block))
    assert alloc.data_ptr() % 16 == 0 and d_block.data_ptr() % 16 == skew
    k = 0
    for first, ndat in _windows(bn):
        want = gc.rows_of(stream, first, ndat)
        nblk = -(-(first + ndat) // bn)
        need = (nblk - 1) * bs + (nchan - 1) * cs + bn * 2 * npol
        for offset in range(4):
            pad = (0, 1, 3)[k % 3]
            k += 1
            lay = OutputLayout(nchan, npol, 2 * ndat, offset=offset, row_pad=pad)
            buf, rows = sentinel_rows(lay)
            # the block is cut behind the last kept sample the call may read
            dspsr_amd.unpack_guppi_fpt(ctx, d_block[:need], rows, dspsr_amd.GuppiLayout(nchan, npol, bn, first, cs, bs), ndat)
            ctx.synchronize()
            got = buf.cpu().numpy()
            exp = place_parts(lay, np.full(lay.size, SENTINEL, np.int32), want.view(np.int32).reshape(nchan, npol, 1, 2 * ndat), 0)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, "nchan %d npol %d block_nsamp %d first %d ndat %d offset %d pad %d: %d floats differ, the first: %s" % (
                nchan, npol, bn, first, ndat, offset, pad, bad.size, describe_float(lay, int(bad[0]), 1, 0, 2 * ndat))


def test_unpack_guppi_empty_call_and_refusals(gpu):
    dspsr_amd, ctx = gpu
    from dspsr_amd import _lib
    nchan, npol, bn, ovl = 3, 2, 259, 5
    cs = gc.chan_stride_of(bn, ovl, npol)
    bs = nchan * cs
    block = torch.from_numpy(gc.random_blocks(3 * bs)).cuda()
    ndat = 300
    lay = OutputLayout(nchan, npol, 2 * ndat)
    buf, rows = sentinel_rows(lay)
    ocs, ops = rows.stride(0), rows.stride(1)
    ptr = block.data_ptr()

    def call(raw_ptr=ptr, n=ndat, out_ptr=rows.data_ptr(), ocs_=ocs, ops_=ops, null_layout=False, ctx_=ctx.handle, **over):
        g = dict(nchan=nchan, npol=npol, block_nsamp=bn, first=7, chan_stride=cs, block_stride=bs)
        g.update(over)
        lay_ = _lib.GuppiLayout(g["nchan"], g["npol"], g["block_nsamp"], g["first"], g["chan_stride"], g["block_stride"])
        return _lib.lib.dspsr_amd_unpack_guppi_fpt(ctx_, raw_ptr, None if null_layout else C.byref(lay_), n, out_ptr, ocs_, ops_)

    def message():
        return _lib.lib.dspsr_amd_last_error(ctx.handle).decode()

    assert call(n=0) == _lib.OK                                                          # ndat = 0: nothing to do
    assert call(ctx_=None) == _lib.EINVAL
    assert call(null_layout=True) == _lib.EINVAL and "layout" in message()
    assert call(nchan=0) == _lib.EINVAL and "nchan" in message()
    for bad in (0, 3, 4):
        assert call(npol=bad) == _lib.EINVAL and "npol" in message()
    assert call(block_nsamp=0) == _lib.EINVAL and "block_nsamp" in message()
    assert call(first=bn) == _lib.EINVAL and "first" in message()
    assert call(chan_stride=bn * 4 - 4) == _lib.EINVAL and "chan_stride" in message()
    assert call(block_stride=2 * cs + bn * 4 - 4) == _lib.EINVAL and "block_stride" in message()
    assert call(chan_stride=cs + 2) == _lib.EINVAL and "multiple of one sample" in message()
    assert call(block_stride=bs + 2) == _lib.EINVAL and "multiple of one sample" in message()
    assert call(raw_ptr=ptr + 2) == _lib.EINVAL and "raw_dev" in message()
    assert call(raw_ptr=ptr + 1, npol=1, chan_stride=2 * bn, block_stride=6 * bn) == _lib.EINVAL and "raw_dev" in message()
    assert call(n=1 << 60) == _lib.EINVAL and "ndat" in message()
    assert call(ocs_=ops) == _lib.EINVAL and "overlap" in message()                      # channel rows inside each other
    assert call(ops_=2 * ndat - 2) == _lib.EINVAL and "overlap" in message()
    assert call(raw_ptr=None) == _lib.EINVAL and "null" in message()
    assert call(out_ptr=None) == _lib.EINVAL and "null" in message()
    ctx.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused or empty call wrote"
    # the binding checks the bytes of the block: one byte short of the last kept sample is refused
    g = dspsr_amd.GuppiLayout(nchan, npol, bn, 7, cs, bs)
    need = bs + 2 * cs + bn * 4                                                          # 7 + 300 samples: two blocks
    with pytest.raises(dspsr_amd.DspsrAmdError, match="%d needed" % need):
        dspsr_amd.unpack_guppi_fpt(ctx, block[:need - 1], rows, g, ndat)
    dspsr_amd.unpack_guppi_fpt(ctx, block[:need], rows, g, ndat)
    ctx.synchronize()
    want = gc.rows_of(gc.stream_from_blocks(block.cpu().numpy(), nchan, npol, bn, ovl), 7, ndat)
    assert np.array_equal(rows.cpu().numpy().view(np.int32), want.view(np.int32))


# ---- the engine: RAW_GUPPI blocks through the raw entry points -----------------------------------------------------------------------
NCHAN = 4


@pytest.mark.parametrize("M", [1024, 16384])
def test_engine_takes_guppi_blocks_like_the_float_rows(gpu, M):
    """-F 4:D on 4 input channels (the convolution of every channel): perform_raw and perform_detect on RAW_GUPPI blocks == perform and
    perform_detect on the restatement's float rows, bit for bit; the second call starts inside a GUPPI block"""
    dspsr_amd, ctx = gpu
    from dspsr_amd import _lib
    bn, ovl, npol = 4099, 13, 2
    nfilt = (M // 8 + 1, M // 16)
    step = M - sum(nfilt)
    calls = (2, 1)
    cs = gc.chan_stride_of(bn, ovl, npol)
    bs = NCHAN * cs
    nsamp_all = sum(calls) * step + sum(nfilt)
    nblk_all = -(-nsamp_all // bn)
    block = gc.random_blocks(nblk_all * bs, seed=M)
    stream = gc.stream_from_blocks(block, NCHAN, npol, bn, ovl)
    d_block = torch.from_numpy(block).cuda()
    kernel = np.exp(1j * np.random.default_rng(M).uniform(-np.pi, np.pi, NCHAN * M)).astype(np.complex64)
    eng = dspsr_amd.FilterbankEngine(ctx).setup(1, M, nfilt[0], nfilt[1], NCHAN, npol, False, kernel, max_parts=2)
    ref = dspsr_amd.FilterbankEngine(ctx).setup(1, M, nfilt[0], nfilt[1], NCHAN, npol, False, kernel, max_parts=2)
    assert eng.npass(False) == (1 if M == 1024 else 3) and (eng.nsamp_step, eng.nkeep) == (step, step)
    out0 = torch.zeros((NCHAN, npol, 2 * step), dtype=torch.float32, device="cuda")
    with pytest.raises(dspsr_amd.DspsrAmdError, match="set_guppi"):                      # a RAW_GUPPI block before set_guppi
        eng.perform_raw(d_block, dspsr_amd.guppi_at(0), 1.0, out0, 1)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="contradict"):
        eng.set_guppi(bn, bn * 4 - 4, bs)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="input_nchan=4"):
        eng.set_guppi(bn, cs, 3 * cs)
    eng.set_guppi(bn, cs, bs)
    pos = 0
    for npart in calls:
        s0 = pos * step
        first, k0 = s0 % bn, s0 // bn
        assert (pos == 0) == (first == 0)                                               # the second call starts inside a block
        nsamp = npart * step + sum(nfilt)
        raw = d_block[k0 * bs:(k0 + -(-(first + nsamp) // bn)) * bs]
        layout = dspsr_amd.guppi_at(first)
        assert _lib.is_guppi(layout) and layout & 0xff == dspsr_amd.RAW_GUPPI
        x = torch.from_numpy(gc.rows_of(stream, s0, nsamp)).cuda()
        lay = OutputLayout(NCHAN, npol, 2 * npart * step, offset=2, row_pad=3)
        outs = []
        for how in ("float", "guppi"):
            buf, rows = sentinel_rows(lay)
            if how == "float":
                ref.perform(x, rows, npart, 2 * step, 2 * step)
            else:
                eng.perform_raw(raw, layout, 123.0, rows, npart)                         # (the scale is ignored for this layout)
            ctx.synchronize()
            outs.append(buf.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]), "perform_raw(RAW_GUPPI) differs from perform on the restatement's rows"
        assert bool((outs[0] != SENTINEL).any())
        for state, ndim in ((dspsr_amd.COHERENCE, 4), (dspsr_amd.STOKES, 2)):
            dlay = OutputLayout(NCHAN, 4 // ndim, npart * step * ndim, offset=1, row_pad=1)
            dets = []
            for how in ("float", "guppi"):
                buf, rows = sentinel_rows(dlay)
                if how == "float":
                    ref.perform_detect(rows, npart, state, ndim, inp=x, in_step=2 * step)
                else:
                    eng.perform_detect(rows, npart, state, ndim, raw=raw, layout=layout, scale=1.0)
                ctx.synchronize()
                dets.append(buf.cpu().numpy())
            assert np.array_equal(dets[0], dets[1]), "perform_detect(RAW_GUPPI) differs, ndim %d" % ndim
        # a block one byte short of the last kept sample is refused by the binding
        with pytest.raises(dspsr_amd.DspsrAmdError, match="needed"):
            eng.perform_raw(raw[:(-(-(first + nsamp) // bn) - 1) * bs + 3 * cs + bn * 4 - 1], layout, 1.0, out0, npart)
        pos += npart
    eng.close()
    ref.close()
    real = dspsr_amd.FilterbankEngine(ctx).setup(32, 256, 100, 92, 1, 2, True, None, max_parts=2)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="real input"):
        real.set_guppi(bn, cs, bs)
    real.close()
