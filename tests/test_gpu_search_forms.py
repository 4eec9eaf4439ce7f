"""GPU parity of the stand-alone search-mode operations -- dsp::TScrunch, FScrunch, SampleDelay, Rescale, PScrunch, SigProcDigitizer
(csrc/scrunch.hip, csrc/sample_delay.hip, csrc/rescale.hip) -- on rows placed as dsp::TimeSeries places them, bit for bit.

host/dspsr_amd_engines.h hands these calls get_datptr(0, 0) and the pointer differences of a real TimeSeries: rows at any float
address, padded strides, channel-major or plane-major.  Inputs are placed with device_buffers.device_rows (plane-major ones are cut
from a sentinel buffer), outputs are cut from a buffer that holds one bit pattern; after each call the floats a correct writer touches
hold the reference's BITS and every other int32 of the buffer still holds the pattern: guards, row padding, the floats behind nout.
Packed bytes go into a byte buffer with a guard pattern in front and behind, at their natural alignment.

Rescale and the digitisers run on search_forms.exact_block data, on which the order of the sums cannot matter (the argument is in
tests/search_forms.py, the reference's side of it is proved by tests/test_search_forms_host.py): offset, scale, every output float and
every packed byte equal the oracle's -- there is NO tolerance in this module.  The cases are data in tests/search_forms.py, each with
the kernel and line it is there for."""
import numpy as np
import pytest

import search_forms as forms
from device_buffers import SENTINEL, OutputLayout, describe_float, device_rows, place_parts, sentinel_rows, written_mask

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD_BYTE = 0xA5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _place_in(x, place):
    """float32 [nchan][npol][n] on the device at a placement of search_forms.PLACEMENTS (input side)"""
    offset, row_pad, plane_major = place
    x = np.ascontiguousarray(x, np.float32)
    if not plane_major:
        return device_rows(x, offset, row_pad)
    _, rows = sentinel_rows(forms.layout(x.shape[0], x.shape[1], x.shape[2], place))
    rows.copy_(torch.from_numpy(x))
    return rows


def _assert_rows(buf, lay, want, n, what=""):
    """buf (int32 [lay.size], after the call) against want (float32 [nchan][nplanes][n]): the first n floats of every row hold
    want's bits, every other float of the buffer the pattern"""
    got = buf.cpu().numpy()
    npart = 1 if n else 0
    mask = written_mask(lay, npart, n, n)
    where = lambda i: describe_float(lay, int(i), npart, n, n)
    stray = np.flatnonzero((got != SENTINEL) & ~mask)
    assert stray.size == 0, "%s: %d floats written outside the output; the first: %s, bits 0x%08x" % (
        what, stray.size, where(stray[0]), got[stray[0]] & 0xffffffff)
    exp = place_parts(lay, np.full(lay.size, SENTINEL, np.int32), _bits(want).reshape(lay.nchan, lay.nplanes, 1, n), n)
    diff = np.flatnonzero(got != exp)
    assert diff.size == 0, "%s: %d output floats differ from the reference's bits; the first: %s, bits 0x%08x for 0x%08x" % (
        what, diff.size, where(diff[0]), got[diff[0]] & 0xffffffff, exp[diff[0]] & 0xffffffff)


def _byte_out(nbytes, nbit):
    """(buffer, view of nbytes at the natural alignment of the unit -- 1, 2 (16 bit) or 4 (-32) bytes, no more --, bytes in front)"""
    front = 64 + (4 if nbit == -32 else 2 if nbit == 16 else 1)
    buf = torch.full((front + nbytes + 64,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 64 == 0
    return buf, buf[front:front + nbytes], front


def _assert_bytes(buf, front, want, what=""):
    got = buf.cpu().numpy()
    want = np.ascontiguousarray(want).view(np.uint8).ravel()
    assert (got[:front] == GUARD_BYTE).all() and (got[front + want.size:] == GUARD_BYTE).all(), "%s: bytes written outside the block" % what
    diff = np.flatnonzero(got[front:front + want.size] != want)
    assert diff.size == 0, "%s: %d of %d bytes differ from the oracle's; the first: byte %d, 0x%02x for 0x%02x" % (
        what, diff.size, want.size, diff[0], got[front + diff[0]], want[diff[0]])


# ---- dsp::TScrunch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", forms.TSCRUNCH_CASES, ids=[c[0] for c in forms.TSCRUNCH_CASES])
def test_tscrunch_fpt_streams_on_placed_rows(gpu, case):
    """k_tscrunch_fpt with ndim 1, 2 and 4 over streams of calls: nout, carry_count, every output float and the carry [row][ndim] equal
    search_forms.stream_reference bit for bit; the float behind the last output of every row, the padding and the guards keep the
    pattern; the carry buffer is cut from a sentinel buffer as well and a call that leaves rem == 0 does not touch it."""
    dspsr_amd, ctx = gpu
    name, nchan, npol, ndim, sf, blocks, place = case
    rng = np.random.default_rng(forms.hash_name(name))
    x = (rng.standard_normal((nchan, npol, sum(blocks) * ndim)).astype(np.float32) ** 2 * 100).astype(np.float32)
    calls = forms.stream_reference(x, blocks, sf, ndim)
    clay = forms.layout(nchan, npol, ndim, (1, 0, False))
    assert (clay.chan_stride, clay.pol_stride) == (npol * ndim, ndim)                 # dense [row][ndim]
    cbuf, carry = sentinel_rows(clay)
    carry_want, cc, pos = None, 0, 0
    for k, (n, c) in enumerate(zip(blocks, calls)):
        what = "%s call %d (c0 %d, %d samples, nout %d, rem %d)" % (name, k, c["c0"], n, c["nout"], c["carry_count"])
        inp = _place_in(x[:, :, pos * ndim:(pos + n) * ndim], forms.PLACEMENTS[place][0])
        lay = forms.layout(nchan, npol, (c["nout"] + 1) * ndim, forms.PLACEMENTS[place][1])
        buf, rows = sentinel_rows(lay)
        nout, cc = dspsr_amd.tscrunch_fpt(ctx, inp, rows, sf, carry, cc, ndim)
        ctx.synchronize()
        assert (nout, cc) == (c["nout"], c["carry_count"]), what
        _assert_rows(buf, lay, c["out"], nout * ndim, what)
        if c["carry"] is not None:
            carry_want = c["carry"]
        if carry_want is None:
            assert (cbuf == SENTINEL).all(), what
        else:
            _assert_rows(cbuf, clay, carry_want, ndim, what + " carry")
        pos += n


# ---- dsp::FScrunch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", forms.FSCRUNCH_CASES, ids=[c[0] for c in forms.FSCRUNCH_CASES])
def test_fscrunch_fpt_on_placed_rows(oracle, gpu, case):
    dspsr_amd, ctx = gpu
    name, nchan, npol, nfloat, sf, place = case
    rng = np.random.default_rng(forms.hash_name(name))
    x = (rng.standard_normal((nchan, npol, nfloat)).astype(np.float32) ** 2 * 100).astype(np.float32)
    inp = _place_in(x, forms.PLACEMENTS[place][0])
    lay = forms.layout(nchan // sf, npol, nfloat + 2, forms.PLACEMENTS[place][1])
    assert inp.stride(0) != lay.chan_stride                                           # (a kernel that mixed the two would be seen)
    buf, rows = sentinel_rows(lay)
    dspsr_amd.fscrunch_fpt(ctx, inp, rows[:, :, :nfloat], sf)
    ctx.synchronize()
    _assert_rows(buf, lay, oracle.fscrunch_fpt(x, sf), nfloat, name)


# ---- dsp::SampleDelay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", forms.SAMPLE_DELAY_CASES, ids=[c[0] for c in forms.SAMPLE_DELAY_CASES])
def test_sample_delay_on_placed_rows(oracle, gpu, case):
    """out of place: nout * ndim floats of every output row hold the shifted input, the floats behind them the pattern; in place: the
    floats [nout * ndim, ndat * ndim) of every row keep their input bits, the padding the pattern"""
    dspsr_amd, ctx = gpu
    name, nchan, npol, ndim, nout, absolute, inplace, place = case
    rng = np.random.default_rng(forms.hash_name(name))
    delays = forms.sample_delays(rng, nchan, npol, absolute)
    ndat = nout + forms.SAMPLE_DELAY_MAX
    x = rng.standard_normal((nchan, npol, ndat * ndim)).astype(np.float32)
    want, zero, total = oracle.sample_delay(x.reshape(nchan, npol, ndat, ndim), delays, absolute)
    want = want.reshape(nchan, npol, nout * ndim)
    sd = dspsr_amd.SampleDelay(ctx, delays, npol, absolute)
    assert (sd.zero_delay, sd.total_delay) == (zero, total) and total == forms.SAMPLE_DELAY_MAX
    if inplace:
        lay = forms.layout(nchan, npol, ndat * ndim, forms.PLACEMENTS[place][1])
        buf, rows = sentinel_rows(lay)
        rows.copy_(torch.from_numpy(x))
        assert sd.transform(rows.unflatten(2, (ndat, ndim))) == nout
        ctx.synchronize()
        _assert_rows(buf, lay, np.concatenate([want, x[:, :, nout * ndim:]], axis=2), ndat * ndim, name)
    else:
        inp = _place_in(x, forms.PLACEMENTS[place][0])
        lay = forms.layout(nchan, npol, (nout + 1) * ndim, forms.PLACEMENTS[place][1])
        buf, rows = sentinel_rows(lay)
        assert sd.transform(inp.unflatten(2, (ndat, ndim)), rows) == nout
        ctx.synchronize()
        _assert_rows(buf, lay, want, nout * ndim, name)
        assert np.array_equal(_bits(inp.cpu().numpy()), _bits(x))
    sd.close()


# ---- dsp::Rescale, dsp::PScrunch, dsp::SigProcDigitizer on exact data -----------------------------------------------------------------
def _tfp_in(x, offset):
    """a TFP block as one run of floats, `offset` floats past a 256-byte boundary"""
    return device_rows(np.ascontiguousarray(x, np.float32).reshape(1, 1, -1), offset, 0)[0, 0]


def _tfp_out(n, offset):
    lay = OutputLayout(1, 1, n, offset, 0)
    buf, rows = sentinel_rows(lay)
    return lay, buf, rows[0, 0]


def _assert_state(r, ro, what):
    off, sc = r.get()
    assert np.array_equal(_bits(off), _bits(ro.offset)), "%s: offsets differ from the oracle's in %d columns" % (
        what, int((_bits(off) != _bits(ro.offset)).sum()))
    assert np.array_equal(_bits(sc), _bits(ro.scale)), "%s: scales differ from the oracle's in %d columns" % (
        what, int((_bits(sc) != _bits(ro.scale)).sum()))


def _digi_options(npol):
    """(use_digi_scales, input_scale) the separate digitiser runs with: behind Rescale; npol 4 also without digi scales (xpol_offset)"""
    return [(True, 1.0)] + ([(False, 1.5)] if npol == 4 else [])


@pytest.mark.parametrize("name", list(forms.RESCALE_CASES))
def test_rescale_and_digitisers_tfp_exact(oracle, gpu, name):
    """transform (into a differently placed block, and in place), pscrunch_tfp, sigproc_digitize (nbit 1-16 and -32) and the fused
    pscrunch_digitize over the blocks of a case: Rescale.get(), every float and every byte equal the oracle's"""
    dspsr_amd, ctx = gpu
    nchan, npol, blocks, interval, constant, flip, swap, _, _ = forms.RESCALE_CASES[name]
    ro = oracle.Rescale(interval, constant)
    r_out, r_in = (dspsr_amd.Rescale(ctx, nchan, npol, interval, constant) for _ in range(2))
    fused = {nbit: dspsr_amd.Rescale(ctx, nchan, npol, interval, constant) for nbit in forms.NBITS} if npol == 2 else {}
    for b, x in enumerate(forms.rescale_blocks(name)):
        what = "%s block %d" % (name, b)
        ndat, n = x.shape[0], x.size
        want = ro.transform(x)
        d_in = _tfp_in(x, (1, 2, 3, 0)[b % 4])
        lay, buf, out = _tfp_out(n, (3, 0, 1, 2)[b % 4])
        r_out.transform(d_in, out)
        _assert_state(r_out, ro, what)
        _assert_rows(buf, lay, want.reshape(1, 1, n), n, what + " transform")
        lay_i, buf_i, io = _tfp_out(n, (2, 3, 0, 1)[b % 4])
        io.copy_(torch.from_numpy(x.ravel()))
        r_in.transform(io)
        _assert_state(r_in, ro, what + " in place")
        _assert_rows(buf_i, lay_i, want.reshape(1, 1, n), n, what + " transform in place")
        for nbit in forms.NBITS + (-32,):
            for digi, iscale in _digi_options(npol):
                bbuf, bout, front = _byte_out(forms.packed_bytes(ndat, nchan, npol, nbit), nbit)
                dspsr_amd.sigproc_digitize(ctx, out, bout, nchan, npol, nbit, digi, iscale, 0.75, flip, swap)
                _assert_bytes(bbuf, front, oracle.sigproc_digitize(want, nbit, digi, iscale, 0.75, flip, swap),
                              "%s sigproc_digitize nbit %d digi %d" % (what, nbit, digi))
        if npol == 2:
            inten = oracle.pscrunch_tfp(want)
            lay_p, buf_p, pout = _tfp_out(ndat * nchan, (1, 3)[b % 2])
            dspsr_amd.pscrunch_tfp(ctx, out, pout, nchan, 2)
            ctx.synchronize()
            _assert_rows(buf_p, lay_p, inten.reshape(1, 1, -1), ndat * nchan, what + " pscrunch_tfp")
            d8 = _tfp_in(x, (0, 2)[b % 2])
            for nbit in forms.NBITS:
                bbuf, bout, front = _byte_out(forms.packed_bytes(ndat, nchan, 1, nbit), nbit)
                fused[nbit].pscrunch_digitize(d8, bout, nbit, 0.75, flip, swap)
                _assert_state(fused[nbit], ro, what + " pscrunch_digitize nbit %d" % nbit)
                _assert_bytes(bbuf, front, oracle.sigproc_digitize(inten, nbit, True, 1.0, 0.75, flip, swap),
                              "%s pscrunch_digitize nbit %d" % (what, nbit))
    assert ro.scale[0, 0] == 1.0 or len(forms.rescale_intervals(blocks, interval)) > 1
    for r in [r_out, r_in] + list(fused.values()):
        r.close()


@pytest.mark.parametrize("name", list(forms.RESCALE_CASES))
def test_rescale_and_digitisers_fpt_exact(oracle, gpu, name):
    """transform_fpt (into differently placed rows, and in place), sigproc_digitize_fpt (nbit 1-16 and -32) and the fused digitize_fpt
    on placed rows: the same statistics per (chan, pol) as the TFP form, so the same oracle, bit for bit"""
    dspsr_amd, ctx = gpu
    nchan, npol, blocks, interval, constant, flip, swap, _, _ = forms.RESCALE_CASES[name]
    ro = oracle.Rescale(interval, constant)
    r_out, r_in = (dspsr_amd.Rescale(ctx, nchan, npol, interval, constant) for _ in range(2))
    fused = {nbit: dspsr_amd.Rescale(ctx, nchan, npol, interval, constant) for nbit in forms.NBITS}
    first = list(forms.RESCALE_CASES).index(name)
    for b, x in enumerate(forms.rescale_blocks(name)):
        what = "%s block %d" % (name, b)
        ndat = x.shape[0]
        want = ro.transform(x)
        xf, wf = np.ascontiguousarray(x.transpose(1, 2, 0)), np.ascontiguousarray(want.transpose(1, 2, 0))
        pin, pout = forms.PLACEMENTS[(first + b) % 4]
        inp = _place_in(xf, pin)
        lay = forms.layout(nchan, npol, ndat + 1, pout)
        buf, rows = sentinel_rows(lay)
        r_out.transform_fpt(inp, rows[:, :, :ndat])
        _assert_state(r_out, ro, what)
        _assert_rows(buf, lay, wf, ndat, what + " transform_fpt")
        lay_i = forms.layout(nchan, npol, ndat, forms.PLACEMENTS[(first + b + 1) % 4][1])
        buf_i, io = sentinel_rows(lay_i)
        io.copy_(torch.from_numpy(xf))
        r_in.transform_fpt(io)
        _assert_state(r_in, ro, what + " in place")
        _assert_rows(buf_i, lay_i, wf, ndat, what + " transform_fpt in place")
        for nbit in forms.NBITS + (-32,):
            for digi, iscale in _digi_options(npol):
                bbuf, bout, front = _byte_out(forms.packed_bytes(ndat, nchan, npol, nbit), nbit)
                dspsr_amd.sigproc_digitize_fpt(ctx, rows[:, :, :ndat], bout, nbit, digi, iscale, 0.75, flip, swap)
                _assert_bytes(bbuf, front, oracle.sigproc_digitize_fpt(wf, nbit, use_digi_scales=digi, input_scale=iscale, scale_fac=0.75,
                                                                       flip_band=flip, swap_band=swap),
                              "%s sigproc_digitize_fpt nbit %d digi %d" % (what, nbit, digi))
        for nbit in forms.NBITS:
            bbuf, bout, front = _byte_out(forms.packed_bytes(ndat, nchan, npol, nbit), nbit)
            fused[nbit].digitize_fpt(inp, bout, nbit, 0.75, flip, swap)
            _assert_state(fused[nbit], ro, what + " digitize_fpt nbit %d" % nbit)
            _assert_bytes(bbuf, front, oracle.sigproc_digitize_fpt(wf, nbit, use_digi_scales=True, input_scale=1.0, scale_fac=0.75,
                                                                   flip_band=flip, swap_band=swap), "%s digitize_fpt nbit %d" % (what, nbit))
    for r in [r_out, r_in] + list(fused.values()):
        r.close()


# ---- beyond the grid caps -----------------------------------------------------------------------------------------------------------
def test_tfp_digitisers_and_pscrunch_beyond_their_grid_caps(oracle, gpu):
    """more than 8192 x 256 units through k_pscrunch_tfp, k_sigproc_digitize and k_sigproc_float: the grid-stride loops take a second
    trip"""
    dspsr_amd, ctx = gpu
    nchan, npol, ndat = (forms.DIGITIZE_BIG[k] for k in ("nchan", "npol", "ndat"))
    rng = np.random.default_rng(77)
    x = forms.exact_block(rng, (ndat, nchan, npol), 2.0, 8, 7) - np.float32(3.0)
    d = _tfp_in(x, 2)
    inten = oracle.pscrunch_tfp(x)
    lay, buf, pout = _tfp_out(ndat * nchan, 1)
    dspsr_amd.pscrunch_tfp(ctx, d, pout, nchan, npol)
    ctx.synchronize()
    _assert_rows(buf, lay, inten.reshape(1, 1, -1), ndat * nchan, "pscrunch_tfp")
    for nbit in (8, 16, -32):
        bbuf, bout, front = _byte_out(forms.packed_bytes(ndat, nchan, 1, nbit), nbit)
        dspsr_amd.sigproc_digitize(ctx, pout, bout, nchan, 1, nbit, True, 1.0, 0.75, True, True)
        _assert_bytes(bbuf, front, oracle.sigproc_digitize(inten, nbit, True, 1.0, 0.75, True, True), "sigproc_digitize nbit %d" % nbit)
    bbuf, bout, front = _byte_out(forms.packed_bytes(ndat, nchan, npol, 4), 4)           # sub-byte: 8192 x 256 bytes of two samples
    dspsr_amd.sigproc_digitize(ctx, d, bout, nchan, npol, 4, True, 1.0, 1.0, False, True)
    _assert_bytes(bbuf, front, oracle.sigproc_digitize(x, 4, True, 1.0, 1.0, False, True), "sigproc_digitize nbit 4")


@pytest.mark.parametrize("name", list(forms.RESCALE_BIG))
def test_rescale_beyond_its_grid_caps_exact(oracle, gpu, name):
    dspsr_amd, ctx = gpu
    nchan, npol, blocks, interval, constant, flip, swap, _, why = forms.RESCALE_BIG[name]
    ro = oracle.Rescale(interval, constant)
    r = dspsr_amd.Rescale(ctx, nchan, npol, interval, constant)
    r2 = dspsr_amd.Rescale(ctx, nchan, npol, interval, constant)
    for b, x in enumerate(forms.rescale_blocks(name)):
        what = "%s block %d (%s)" % (name, b, why)
        ndat, n = x.shape[0], x.size
        want = ro.transform(x)
        if name == "tfp-slices-double":
            lay, buf, out = _tfp_out(n, 1)
            r.transform(_tfp_in(x, 3), out)
            _assert_state(r, ro, what)
            _assert_rows(buf, lay, want.reshape(1, 1, n), n, what)
        elif name == "fused-rows-cap":
            inten = oracle.pscrunch_tfp(want)
            for rr, nbit in ((r, 8), (r2, 2)):
                bbuf, bout, front = _byte_out(forms.packed_bytes(ndat, nchan, 1, nbit), nbit)
                rr.pscrunch_digitize(_tfp_in(x, 2), bout, nbit, 0.75, flip, swap)
                _assert_state(rr, ro, what)
                _assert_bytes(bbuf, front, oracle.sigproc_digitize(inten, nbit, True, 1.0, 0.75, flip, swap), what + " nbit %d" % nbit)
        else:                                                   # FPT rows, in place
            wf = np.ascontiguousarray(want.transpose(1, 2, 0))
            lay = forms.layout(nchan, npol, ndat, (1, 3, False))
            buf, io = sentinel_rows(lay)
            io.copy_(torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0))))
            if name == "apply-fpt-cap":
                bbuf, bout, front = _byte_out(forms.packed_bytes(ndat, nchan, npol, 8), 8)
                r2.digitize_fpt(io, bout, 8, 0.75, flip, swap)
                _assert_state(r2, ro, what + " digitize_fpt")
                _assert_bytes(bbuf, front, oracle.sigproc_digitize_fpt(wf, 8, use_digi_scales=True, input_scale=1.0, scale_fac=0.75,
                                                                       flip_band=flip, swap_band=swap), what + " digitize_fpt")
            r.transform_fpt(io)
            _assert_state(r, ro, what)
            _assert_rows(buf, lay, wf, ndat, what)
            del buf, io
    r.close()
    r2.close()


# ---- the float2 read of k_rescale_pscrunch_digitize ---------------------------------------------------------------------------------
def test_fused_output_stage_refuses_a_block_that_is_not_8_byte_aligned(oracle, gpu):
    """include/dspsr_amd.h: dspsr_amd_rescale_pscrunch_digitize reads a channel's two polarisations as one float2; a PPQQ block that is
    4-byte but not 8-byte aligned is refused with DSPSR_AMD_EINVAL before any launch -- the output keeps its pattern, and the object
    then gives the bytes and the state of an object that never saw the refused call."""
    dspsr_amd, ctx = gpu
    nchan, ndat = 16, 300
    rng = np.random.default_rng(8)
    xs = [forms.exact_block(rng, (ndat, nchan, 2), 3.0, 8, 7, ndat) for _ in range(2)]
    ro = oracle.Rescale(200, False)
    ra, rb = dspsr_amd.Rescale(ctx, nchan, 2, 200, False), dspsr_amd.Rescale(ctx, nchan, 2, 200, False)
    for b, x in enumerate(xs):
        want = oracle.sigproc_digitize(oracle.pscrunch_tfp(ro.transform(x)), 8, True, 1.0, 1.0, True, False)
        abuf, aout, front = _byte_out(ndat * nchan, 8)
        ra.pscrunch_digitize(_tfp_in(x, 2), aout, 8, 1.0, True, False)
        _assert_bytes(abuf, front, want, "aligned, block %d" % b)
        bbuf, bout, _ = _byte_out(ndat * nchan, 8)
        for odd in (1, 3):
            blk = _tfp_in(x, odd)
            assert blk.data_ptr() % 8 == 4
            with pytest.raises(dspsr_amd.DspsrAmdError, match=r"\(-1\): dspsr_amd_rescale_pscrunch_digitize: the block must be 8-byte aligned"):
                rb.pscrunch_digitize(blk, bout, 8, 1.0, True, False)
        ctx.synchronize()
        assert (bbuf == GUARD_BYTE).all()
        rb.pscrunch_digitize(_tfp_in(x, 0), bout, 8, 1.0, True, False)
        _assert_bytes(bbuf, front, want, "after the refusals, block %d" % b)
        _assert_state(rb, ro, "after the refusals, block %d" % b)
    ra.close()
    rb.close()


# ---- what the C-ABI refuses, with nothing touched -----------------------------------------------------------------------------------
def test_refused_calls_leave_buffers_and_state_untouched(oracle, gpu):
    dspsr_amd, ctx = gpu
    rng = np.random.default_rng(9)
    Err = dspsr_amd.DspsrAmdError
    # nchan * npol > 65535 through the FPT Rescale calls (one workgroup row per column); the object then runs its first TFP block as a
    # fresh one does
    nchan, ndat = 65536, 2
    x = forms.exact_block(rng, (ndat, nchan, 1), 3.0, 8, 7, ndat)
    r = dspsr_amd.Rescale(ctx, nchan, 1, 0, False)
    lay = OutputLayout(nchan, 1, ndat, 1, 1)
    buf, rows = sentinel_rows(lay)
    bbuf, bout, front = _byte_out(ndat * nchan, 8)
    inp = device_rows(np.ascontiguousarray(x.transpose(1, 2, 0)), 0, 0)
    with pytest.raises(Err, match="dspsr_amd_rescale_transform_fpt: nchan\\*npol=65536 exceeds the grid limit"):
        r.transform_fpt(inp, rows)
    with pytest.raises(Err, match="dspsr_amd_rescale_digitize_fpt: nchan\\*npol=65536 exceeds the grid limit"):
        r.digitize_fpt(inp, bout, 8)
    ctx.synchronize()
    assert (buf == SENTINEL).all() and (bbuf == GUARD_BYTE).all()
    ro = oracle.Rescale(0, False)
    lay_t, buf_t, out = _tfp_out(x.size, 1)
    r.transform(_tfp_in(x, 0), out)
    want = ro.transform(x)
    _assert_state(r, ro, "after the refused FPT calls")
    _assert_rows(buf_t, lay_t, want.reshape(1, 1, -1), x.size, "after the refused FPT calls")
    r.close()
    # nbit -32 through the fused FPT call; sub-byte samples that do not fill a byte (nchan 12, 8 samples per byte), every entry point
    nchan, ndat = 12, 50
    x = forms.exact_block(rng, (ndat, nchan, 2), 3.0, 8, 7, ndat)
    xf = np.ascontiguousarray(x.transpose(1, 2, 0))
    r = dspsr_amd.Rescale(ctx, nchan, 2, 0, False)
    inp, tfp = device_rows(xf, 2, 1), _tfp_in(x, 0)
    bbuf, bout, front = _byte_out(ndat * nchan * 2 * 4, -32)
    with pytest.raises(Err, match="nbit -32 takes the separate operations"):
        r.digitize_fpt(inp, bout, -32)
    for call in (lambda: r.digitize_fpt(inp, bout, 1), lambda: r.pscrunch_digitize(tfp, bout, 1),
                 lambda: dspsr_amd.sigproc_digitize(ctx, tfp, bout, nchan, 2, 1), lambda: dspsr_amd.sigproc_digitize_fpt(ctx, inp, bout, 1)):
        with pytest.raises(Err, match="nchan=12 not a multiple of 8 samples per byte"):
            call()
    ctx.synchronize()
    assert (bbuf == GUARD_BYTE).all()
    ro = oracle.Rescale(0, False)
    want = ro.transform(x)
    r.digitize_fpt(inp, bout[:ndat * nchan * 2], 8)
    _assert_state(r, ro, "after the refused digitiser calls")
    assert np.array_equal(bout[:ndat * nchan * 2].cpu().numpy().reshape(ndat, 2, nchan), oracle.sigproc_digitize(want, 8))
    r.close()
    # SampleDelay: rows that overlap without being the same rows
    nchan, npol, ndat = 3, 2, 100
    lay = OutputLayout(nchan, npol, ndat + 8, 0, 0)
    buf, rows = sentinel_rows(lay)
    rows.copy_(torch.from_numpy(rng.standard_normal((nchan, npol, ndat + 8)).astype(np.float32)))
    before = buf.clone()
    sd = dspsr_amd.SampleDelay(ctx, np.array([0, 3, 5]), npol)
    with pytest.raises(Err, match="input and output overlap without being the same buffer"):
        sd.transform(rows[:, :, :ndat], rows[:, :, 5:])
    with pytest.raises(Err, match="in place needs equal strides"):
        sd.transform(rows[:, :, :ndat], torch.as_strided(rows, (nchan, npol, ndat), (rows.stride(0), rows.stride(1) - 1, 1)))
    # in-place TScrunch and FScrunch
    carry_lay = OutputLayout(nchan, npol, 1, 1, 0)
    cbuf, carry = sentinel_rows(carry_lay)
    with pytest.raises(Err, match="dspsr_amd_tscrunch_fpt: in place is not supported"):
        dspsr_amd.tscrunch_fpt(ctx, rows, rows, 3, carry, 0)
    with pytest.raises(Err, match="dspsr_amd_fscrunch_fpt: in place is not supported"):
        dspsr_amd.fscrunch_fpt(ctx, rows, rows, 3)
    ctx.synchronize()
    assert torch.equal(buf, before) and (cbuf == SENTINEL).all()
    sd.close()
