"""Two-bit voltages on the device: dspsr_amd_twobit_unpack (k_twobit_levels + k_twobit_unpack) bit for bit against the loop
restatement of tests/twobit_cases.py, given the same level table -- rows, per-digitiser weights and n_low; three table types x
npol 1, 2 x nsample 4, 8, 64, 512 over nine windows (every excision cause, both kept edges of the limits, one polarisation bad where
the other is good); calls of three to nine windows starting at first_sample 0 ... 4 and nsample - 1 and ending on a window, inside
one and inside a byte; output rows at float offsets 0 ... 3 from a 16-byte boundary, cut from a sentinel buffer; the call split in
two at every phase of a window."""
import numpy as np
import pytest

import twobit_cases as tc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0x7FC0BEEF      # a NaN payload no unpacked value has


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


_REFERENCE = {}


def reference(case):
    """the case's block and its restated unpacking, computed once and shared (never written)"""
    if case not in _REFERENCE:
        from dspsr_amd import twobit
        table_type, npol, nsample = case
        block, nlow_min, nlow_max = tc.stream(*case)
        levels = twobit.levels(nsample, nlow_min, nlow_max)
        rows, weights, n_low = tc.unpack_restated(block, table_type, npol, nsample, nlow_min, nlow_max, levels)
        for a in (block, levels, rows, weights, n_low):
            a.setflags(write=False)
        _REFERENCE[case] = (block, nlow_min, nlow_max, levels, rows, weights, n_low)
    return _REFERENCE[case]


def calls_of(nsample, nwindow):
    """(first window, first_sample, ndat): three to nine windows, every first_sample asked, ends on a window, inside one and inside
    a byte"""
    firsts = sorted({0, 1, 2, 3, 4 % nsample, nsample - 1})
    out = []
    for k, first in enumerate(firsts):
        w0 = k % 3
        room = (nwindow - w0) * nsample - first
        ends = [room,                                              # the last sample of the block: ends on a window
                room - nsample // 2 if nsample > 4 else room - 4,  # mid-window, on a byte
                room - nsample - 1]                                # mid-byte
        if first == 0:
            ends.append(3 * nsample)                               # three whole windows
        for ndat in ends:
            if ndat > 2 * nsample:
                out.append((w0, first, ndat))
    return out


def _unpack(dspsr_amd, ctx, d_block, case, ref, w0, first, ndat, offset):
    """one call on rows `offset` floats behind a 16-byte boundary of a sentinel buffer: (buffer as int32, row starts, weights, n_low)"""
    table_type, npol, nsample = case
    _, nlow_min, nlow_max, levels, _, _, _ = ref
    per = (nsample // 4) * npol
    nwin = -(-(first + ndat) // nsample)
    stride = (ndat + 3) // 4 * 4 + 8                                # rows keep the offset: the stride is a multiple of 4 floats
    buf = torch.full((8 + npol * stride,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    rows = buf.view(torch.float32)[4 + offset:4 + offset + npol * stride].view(npol, stride)[:, :ndat]
    weights = torch.full((npol, nwin), 77, dtype=torch.int32, device="cuda")
    n_low = torch.full((npol, nwin), 77, dtype=torch.int32, device="cuda")
    raw = d_block[w0 * per:(w0 + nwin) * per]
    assert raw.data_ptr() % 4 == 0 or per % 4, "the case's windows start on words"
    if raw.data_ptr() % 4:                                          # (short windows of one digitiser: move the call's block to a word)
        raw = raw.clone()
    dspsr_amd.twobit_unpack(ctx, raw, rows, torch.from_numpy(np.array(levels)).cuda(), weights, nsample, nlow_min, nlow_max, table_type,
                            first, ndat, nlow=n_low)
    ctx.synchronize()
    starts = [4 + offset + p * stride for p in range(npol)]
    return buf.cpu().numpy(), starts, weights.cpu().numpy(), n_low.cpu().numpy()


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_twobit_unpack_bit_for_bit(gpu, case):
    dspsr_amd, ctx = gpu
    table_type, npol, nsample = case
    ref = reference(case)
    block, _, _, _, want_rows, want_w, want_n = ref
    nwindow = want_w.shape[1]
    d_block = torch.from_numpy(np.array(block)).cuda()
    k = 0
    for w0, first, ndat in calls_of(nsample, nwindow):
        nwin = -(-(first + ndat) // nsample)
        assert 3 <= nwin <= 9
        for offset in ((0, 1, 2, 3) if k % 2 == 0 else (k % 4,)):       # every offset on every other call, one on the rest
            got, starts, w, n = _unpack(dspsr_amd, ctx, d_block, case, ref, w0, first, ndat, offset)
            exp = np.full(got.size, SENTINEL, np.int32)
            for p, s in enumerate(starts):
                exp[s:s + ndat] = want_rows[p, w0 * nsample + first:w0 * nsample + first + ndat].view(np.int32)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, "%s w0 %d first %d ndat %d offset %d: %d floats differ, the first at %d (row starts %s): %#x, want %#x" % (
                tc.case_id(case), w0, first, ndat, offset, bad.size, bad[0], starts, got[bad[0]] & 0xffffffff, exp[bad[0]] & 0xffffffff)
            assert np.array_equal(w.view(np.uint32), want_w[:, w0:w0 + nwin]), "weights, first %d ndat %d" % (first, ndat)
            assert np.array_equal(n.view(np.uint32), want_n[:, w0:w0 + nwin]), "n_low, first %d ndat %d" % (first, ndat)
        k += 1


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[2] in (8, 64)], ids=tc.case_id)
def test_twobit_two_calls_equal_one(gpu, case):
    """the stream cut at every phase of a window (and so of a byte): the two calls' rows, laid end to end, are the one call's"""
    dspsr_amd, ctx = gpu
    table_type, npol, nsample = case
    ref = reference(case)
    _, nlow_min, nlow_max, levels, want_rows, want_w, _ = ref
    per = (nsample // 4) * npol
    d_block = torch.from_numpy(np.array(ref[0])).cuda()
    d_levels = torch.from_numpy(np.array(levels)).cuda()
    first, ndat = 3, 6 * nsample + 1
    whole = torch.zeros((npol, ndat), dtype=torch.float32, device="cuda")
    nwin = -(-(first + ndat) // nsample)
    dspsr_amd.twobit_unpack(ctx, d_block, whole, d_levels, torch.empty((npol, nwin), dtype=torch.int32, device="cuda"), nsample, nlow_min,
                            nlow_max, table_type, first, ndat)
    ctx.synchronize()
    one = whole.cpu().numpy()
    assert np.array_equal(one.view(np.int32), want_rows[:, first:first + ndat].view(np.int32))
    for phase in range(nsample):
        cut = 2 * nsample + phase                                    # samples of the first call
        two = torch.zeros((npol, ndat), dtype=torch.float32, device="cuda")
        s1 = first + cut                                             # stream sample of the second call's first
        w1 = s1 // nsample
        parts = ((0, first, cut, two[:, :cut]), (w1, s1 % nsample, ndat - cut, two[:, cut:]))
        ws = []
        for w0, f, n, rows in parts:
            nw = -(-(f + n) // nsample)
            raw = d_block[w0 * per:(w0 + nw) * per]
            if raw.data_ptr() % 4:
                raw = raw.clone()
            ws.append(torch.empty((npol, nw), dtype=torch.int32, device="cuda"))
            dspsr_amd.twobit_unpack(ctx, raw, rows, d_levels, ws[-1], nsample, nlow_min, nlow_max, table_type, f, n)
        ctx.synchronize()
        assert np.array_equal(two.cpu().numpy().view(np.int32), one.view(np.int32)), "cut at window phase %d" % phase
        assert np.array_equal(ws[1].cpu().numpy().view(np.uint32), want_w[:, w1:w1 + ws[1].shape[1]])


def test_twobit_refusals_and_empty_call_write_nothing(gpu):
    dspsr_amd, ctx = gpu
    from dspsr_amd import _lib
    case = (tc.OFFSET_BINARY, 2, 64)
    block, nlow_min, nlow_max, levels, _, _, _ = reference(case)
    d_block = torch.from_numpy(np.array(block)).cuda()
    d_levels = torch.from_numpy(np.array(levels)).cuda()
    ndat = 200
    buf = torch.full((2 * ndat + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    weights = torch.full((2, 4), 77, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = dict(raw=d_block.data_ptr(), table_type=0, npol=2, nsample=64, first=0, ndat=ndat, nlow_min=nlow_min, nlow_max=nlow_max,
                 out=buf.data_ptr() + 16, stride=ndat)
        a.update(kw)
        return _lib.lib.dspsr_amd_twobit_unpack(ctx.handle, a["raw"], a["table_type"], a["npol"], a["nsample"], a["first"], a["ndat"],
                                                a["nlow_min"], a["nlow_max"], d_levels.data_ptr(), a["out"], a["stride"],
                                                weights.data_ptr(), None)

    def message():
        return _lib.lib.dspsr_amd_last_error(ctx.handle).decode()

    assert call(ndat=0) == _lib.OK
    for kw, words in ((dict(nsample=62), "multiple of 4"), (dict(nsample=0), "multiple of 4"), (dict(nsample=65540), "65536"),
                      (dict(nlow_max=nlow_min), "nlow_min"), (dict(nlow_max=65), "nsample"), (dict(first=64), "first_sample"),
                      (dict(npol=3), "npol"), (dict(raw=d_block.data_ptr() + 2), "4 bytes"), (dict(stride=ndat - 1), "overlap"),
                      (dict(table_type=3), "table_type")):
        assert call(**kw) == _lib.EINVAL and words in message(), (kw, message())
    ctx.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((weights == 77).all()), "a refused or empty call wrote"
