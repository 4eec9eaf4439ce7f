"""GPU parity of the filterbank's output writers at every address, stride and layout the C-ABI accepts.

The adaptors hand over out->get_datptr(0, 0) and the pointer differences to the next channel and polarisation
(host/dspsr_amd_engines.h); dsp::TimeSeries puts its rows at buffer + reserve and pads them (TimeSeries.C:146-179).  So an output row
is 4-byte aligned (as a rule 8, seldom 16), its strides are any number of floats, out_step may exceed 2 * nkeep, and detected rows
come channel-major or plane-major.  Every case here runs one call twice on the same object: into the contiguous, aligned tensor
every other test uses -- that result is checked against the float64 oracle at the bounds of test_gpu_parity.py -- and into rows cut
from a buffer that holds one bit pattern (tests/device_buffers.py sentinel_rows).  The floats a correct writer touches must hold the
bits of the contiguous run (fb_run takes no decision from the output address: filterbank.hip has no branch on FbOut::base or its
strides), and EVERY other float of the buffer must still hold the pattern: guards, row padding, the gaps between parts.

The cases are data in tests/output_forms.py (each family there names the writer, file:line, it is there for); tests/test_output_mask.py
checks their masks without a GPU."""
import math

import numpy as np
import pytest

import output_forms as forms
from device_buffers import SENTINEL, describe_float, place_parts, sentinel_rows, written_mask
from test_gpu_parity import _fb_block

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


@pytest.fixture(scope="module")
def objects(gpu):
    """one object, input block and oracle output per family, and its contiguous results once they have met the oracle"""
    cache = {}
    yield cache
    for b in cache.values():
        b.eng.close()


def _family(oracle, gpu, objects, family):
    if family not in objects:
        C, M, nfilt, npart, kw, calls, (raw_input, npass) = forms.FAMILIES[family]
        b = _fb_block(oracle, gpu, C, M, nfilt, npart, **kw)
        assert b.eng.npass(bool(raw_input)) == npass, "the object is not of the family %s" % family
        if "rows" in calls and b.inp is None:           # the same block as unpacked float rows (aligned: only the output varies)
            nbytes = b.eng._raw_bytes(npart)
            b.inp = torch.from_numpy(oracle.unpack_8bit(b.raw[:nbytes].cpu().numpy(), b.obs)).cuda()
            b.in_step = b.plan.nsamp_step * b.obs.ndim
        b.tol = 2e-6 * math.sqrt(math.log2(2 * C * M))
        b.rms = math.sqrt(np.mean(np.abs(b.ref) ** 2))
        b.results = {}
        objects[family] = b
    return objects[family]


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _run_complex(b, call, out, npart, out_step):
    if call == "raw":
        b.eng.perform_raw(b.raw, b.layout, b.scale, out, npart, out_step)
    else:
        b.eng.perform(b.inp, out, npart, b.in_step, out_step)
    b.eng.finish()


def _contiguous_complex(b, call):
    """int32 bits [nchan][npol][npart][2 * nkeep] of the call into an aligned contiguous tensor, checked against the float64 oracle
    (test_gpu_parity._fb_case: rms <= 2e-6 sqrt(log2 2N), max <= 8 times that)"""
    key = ("complex", call)
    if key not in b.results:
        out = torch.zeros((b.nchan, b.npol, 2 * b.npart * b.plan.nkeep), dtype=torch.float32, device="cuda")
        _run_complex(b, call, out, b.npart, 2 * b.plan.nkeep)
        got = out.cpu().numpy().view(np.complex64).astype(np.complex128)
        err = got - b.ref
        assert np.isfinite(got).all()
        assert math.sqrt(np.mean(np.abs(err) ** 2)) / b.rms <= b.tol and np.abs(err).max() <= 8 * b.tol * b.rms
        b.results[key] = _bits(out).reshape(b.nchan, b.npol, b.npart, 2 * b.plan.nkeep)
    return b.results[key]


def _run_detect(dspsr_amd, b, det, npart, state, ndim):
    st = dspsr_amd.STOKES if state == "Stokes" else dspsr_amd.COHERENCE
    if b.raw is not None:
        b.eng.perform_detect(det, npart, st, ndim, raw=b.raw, layout=b.layout, scale=b.scale)
    else:
        b.eng.perform_detect(det, npart, st, ndim, inp=b.inp, in_step=b.in_step)
    b.eng.finish()


def _contiguous_detect(oracle, dspsr_amd, b, state, ndim):
    """int32 bits [nchan][4 / ndim][npart * nkeep * ndim] of perform_detect into an aligned contiguous tensor, checked against
    Detection::polarimetry of the float64 filterbank output to 1e-5 of the largest value"""
    key = ("detect", state, ndim)
    if key not in b.results:
        det = torch.zeros((b.nchan, 4 // ndim, b.npart * b.plan.nkeep * ndim), dtype=torch.float32, device="cuda")
        _run_detect(dspsr_amd, b, det, b.npart, state, ndim)
        want = oracle.detect_layout(oracle.detect_products(b.ref, state), ndim)
        got = det.cpu().numpy().reshape(want.shape)
        assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
        b.results[key] = _bits(det)
    return b.results[key]


def _assert_buffer(buf, lay, want, npart, part_step, part_floats):
    """buf (int32 [lay.size], after the call) against `want` (int32 [nchan][nplanes][npart][part_floats], the contiguous run): (a) the
    masked floats hold want's bits, (b) none of them still holds the pattern, (c) every other float still holds it"""
    got = buf.cpu().numpy()
    mask = written_mask(lay, npart, part_step, part_floats)
    where = lambda i: describe_float(lay, int(i), npart, part_step, part_floats)
    stray = np.flatnonzero((got != SENTINEL) & ~mask)
    assert stray.size == 0, "%d floats written outside the output; the first: %s, bits 0x%08x" % (
        stray.size, where(stray[0]), got[stray[0]] & 0xffffffff)
    missing = np.flatnonzero((got == SENTINEL) & mask)
    assert missing.size == 0, "%d output floats never written; the first: %s" % (missing.size, where(missing[0]))
    exp = place_parts(lay, np.full(lay.size, SENTINEL, np.int32), want, part_step)
    diff = np.flatnonzero(got != exp)
    assert diff.size == 0, "%d output floats differ from the run into contiguous rows; the first: %s, bits 0x%08x for 0x%08x" % (
        diff.size, where(diff[0]), got[diff[0]] & 0xffffffff, exp[diff[0]] & 0xffffffff)


# ---- complex rows -----------------------------------------------------------------------------------------------------------
# the 8-byte aligned rows first (offsets 0 and 2): `-k "off0 or off2"` / `-k "off1 or off3"` select by alignment
@pytest.mark.parametrize("family,call,offset,row_pad,extra", forms.COMPLEX_CASES,
                         ids=["%s-%s-off%d-pad%d-step+%s" % c for c in forms.COMPLEX_CASES])
def test_complex_rows(oracle, gpu, objects, family, call, offset, row_pad, extra):
    b = _family(oracle, gpu, objects, family)
    want = _contiguous_complex(b, call)
    lay, npart, step, n = forms.complex_layout(family, offset, row_pad, extra)
    if extra == "in_step":
        assert step == b.in_step                      # (what ConvolutionEngine::perform passes; at these shapes 2 * nkeep)
    buf, rows = sentinel_rows(lay)
    _run_complex(b, call, rows, npart, step)
    _assert_buffer(buf, lay, want, npart, step, n)


@pytest.mark.parametrize("family", ["inv_chan", "conv3_14"])
def test_fewer_parts_than_the_rows_hold_and_empty_calls(oracle, gpu, objects, family):
    """rows with room for four parts: a call of three leaves the fourth alone, npart = 0 leaves everything alone -- complex and
    detected rows"""
    dspsr_amd, ctx = gpu
    b = _family(oracle, gpu, objects, family)
    call = forms.FAMILIES[family][5][0]
    want = _contiguous_complex(b, call)
    lay, npart, step, n = forms.complex_layout(family, 2, 1, 2, nparts_room=4)
    buf, rows = sentinel_rows(lay)
    _run_complex(b, call, rows, 0, step)
    assert (buf == SENTINEL).all()
    _run_complex(b, call, rows, npart, step)
    _assert_buffer(buf, lay, want, npart, step, n)
    wdet = _contiguous_detect(oracle, dspsr_amd, b, "Stokes", 4)
    lay, _, row, _ = forms.detect_layout(family, 4, 2, 1, False, nparts_room=4)
    buf, rows = sentinel_rows(lay)
    _run_detect(dspsr_amd, b, rows, 0, "Stokes", 4)
    assert (buf == SENTINEL).all()
    _run_detect(dspsr_amd, b, rows, b.npart, "Stokes", 4)
    _assert_buffer(buf, lay, wdet[:, :, None, :], 1, row, row)


# ---- detected rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,ndim,state,offset,row_pad,plane_major", forms.DETECT_CASES,
                         ids=["%s-ndim%d-%s-off%d-pad%d-%s" % (c[:5] + ("planes" if c[5] else "chans",)) for c in forms.DETECT_CASES])
def test_detected_rows(oracle, gpu, objects, family, ndim, state, offset, row_pad, plane_major):
    dspsr_amd, ctx = gpu
    b = _family(oracle, gpu, objects, family)
    want = _contiguous_detect(oracle, dspsr_amd, b, state, ndim)
    lay, _, row, _ = forms.detect_layout(family, ndim, offset, row_pad, plane_major)
    buf, rows = sentinel_rows(lay)
    _run_detect(dspsr_amd, b, rows, b.npart, state, ndim)
    _assert_buffer(buf, lay, want[:, :, None, :], 1, row, row)


# ---- search rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,state,sf", forms.SEARCH_CASES, ids=["%s-%s-t%d" % c for c in forms.SEARCH_CASES])
def test_search_rows(oracle, gpu, objects, family, state, sf):
    """fb_common.h:146-185 (FbOut kind 5): two calls of 2 and 3 parts as one stream.  The contiguous run equals square_law +
    tscrunch_fpt of the same object's (oracle-checked) complex output bit for bit, as tests/test_gpu_search.py asserts for the same
    call; the rows with offset 1 and row_pad 1 hold the same bits, the float behind the last complete output of every row -- where
    a writer that treated the open group as complete would put it -- and everything else keeps the pattern; so does the carry."""
    dspsr_amd, ctx = gpu
    b = _family(oracle, gpu, objects, family)
    assert b.eng.search_is_fused() == (family != "four_pass_forced")
    npo = 2 if state == "PPQQ" else 1
    st = dspsr_amd.PPQQ if npo == 2 else dspsr_amd.INTENSITY
    cplx = _contiguous_complex(b, "raw").view(np.float32).reshape(b.nchan, b.npol, -1).view(np.complex64)
    nkeep = b.plan.nkeep
    stream = np.concatenate([oracle.square_law(cplx[:, :, :k * nkeep], state) for k in forms.SEARCH_PARTS], axis=2)
    want = oracle.tscrunch_fpt(stream, sf)
    layouts = forms.search_layouts(family, state, sf)

    def calls(make_rows):
        carry = torch.zeros((b.nchan, npo), dtype=torch.float32, device="cuda")
        cc, res = 0, []
        for npart, (lay, _, nout_want, _) in zip(forms.SEARCH_PARTS, layouts):
            buf, rows = make_rows(lay)
            nout, cc = b.eng.perform_search(rows, carry, cc, npart, sf, st, raw=b.raw, layout=b.layout, scale=b.scale)
            b.eng.finish()
            assert nout == nout_want
            res.append((buf, rows, nout))
        return res, cc, _bits(carry)

    plain, cc0, carry0 = calls(lambda lay: (None, torch.full((lay.nchan, lay.nplanes, lay.row), -1.0, dtype=torch.float32, device="cuda")))
    got = np.concatenate([rows[:, :, :nout].cpu().numpy() for _, rows, nout in plain], axis=2)
    assert got.shape == want.shape and want.shape[2] > 0 and np.array_equal(got, want)
    assert cc0 == sum(forms.SEARCH_PARTS) * nkeep % sf and (sf == 1 or 2 * nkeep % sf != 0)        # the second call began with a carry
    placed, cc1, carry1 = calls(sentinel_rows)
    assert cc1 == cc0 and np.array_equal(carry1, carry0)
    for (buf, _, nout), (_, crows, _), (lay, _, _, _) in zip(placed, plain, layouts):
        _assert_buffer(buf, lay, _bits(crows[:, :, :nout])[:, :, None, :], 1, nout, nout)


# ---- what the C-ABI refuses ---------------------------------------------------------------------------------------------------
def test_overlapping_and_short_output_rows_are_refused(oracle, gpu, objects):
    """dspsr_amd_filterbank_perform and _perform_raw: out_step < 2 * nkeep and rows that overlap; _perform_detect and _perform_search:
    rows that overlap.  Refused before any launch (the buffer keeps the pattern), and the object works afterwards."""
    dspsr_amd, ctx = gpu
    b = _family(oracle, gpu, objects, "inv_chan")
    nkeep, npart = b.plan.nkeep, b.npart
    want = _contiguous_complex(b, "raw")
    lay, _, step, n = forms.complex_layout("inv_chan", 2, 1, 0)
    buf, rows = sentinel_rows(lay)
    flat = buf[lay.first:].view(torch.float32)
    overlap = torch.as_strided(flat, (b.nchan, 2, lay.row), (lay.chan_stride, lay.row - 2, 1))                 # pol rows 2 floats short
    chan_overlap = torch.as_strided(flat, (b.nchan, 2, lay.row), (2 * lay.row - 2, lay.row, 1))               # channel rows likewise
    for call, fn in (("raw", "dspsr_amd_filterbank_perform_raw"), ("rows", "dspsr_amd_filterbank_perform")):
        with pytest.raises(dspsr_amd.DspsrAmdError, match=r"%s: out_step=%d < 2\*nkeep=%d" % (fn, 2 * nkeep - 2, 2 * nkeep)):
            _run_complex(b, call, rows, 1, 2 * nkeep - 2)
        for bad in (overlap, chan_overlap):
            with pytest.raises(dspsr_amd.DspsrAmdError, match="%s: output rows of %d floats overlap" % (fn, lay.row)):
                _run_complex(b, call, bad, npart, step)
    drow = npart * nkeep * 2
    det = torch.as_strided(flat, (b.nchan, 2, drow), (2 * drow, drow - 2, 1))
    with pytest.raises(dspsr_amd.DspsrAmdError, match="detected rows of %d floats overlap" % drow):
        _run_detect(dspsr_amd, b, det, npart, "Coherence", 2)
    nout = npart * nkeep // 3
    srows = torch.as_strided(flat, (b.nchan, 2, nout), (2 * nout, nout - 1, 1))
    carry = torch.zeros((b.nchan, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(dspsr_amd.DspsrAmdError, match="output rows of %d floats overlap" % nout):
        b.eng.perform_search(srows, carry, 0, npart, 3, dspsr_amd.PPQQ, raw=b.raw, layout=b.layout, scale=b.scale)
    b.eng.finish()
    assert (buf == SENTINEL).all() and not carry.any()
    _run_complex(b, "raw", rows, npart, step)
    _assert_buffer(buf, lay, want, npart, step, n)
