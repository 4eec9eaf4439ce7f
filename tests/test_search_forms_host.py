"""What tests/test_gpu_search_forms.py relies on, checked without a GPU: the exact data of tests/search_forms.py is exact, the
reference (oracle.Rescale) gives the same statistics and output on every Rescale case whatever the order its sums are taken in -- so
"zero differing bits" asks of the GPU only what the reference itself keeps --, tscrunch_ref and stream_reference restate the
reference's loops, and the sentinel masks cover exactly what a correct writer touches."""
import math

import numpy as np
import pytest

import search_forms as forms
from device_buffers import SENTINEL, place_parts, written_mask


def test_exact_block_values_and_squares_lie_on_the_stated_granule():
    rng = np.random.default_rng(1)
    for gran, maxb in ((8, 7), (8, 5), (4, 10)):
        x = forms.exact_block(rng, (5000, 3, 2), np.float32(2.0 ** maxb / 8), gran, maxb, nsum=5000)
        assert x.dtype == np.float32 and np.abs(x).max() < 2.0 ** maxb and (np.abs(x) >= 2.0 ** maxb - 1).any()       # the clip is reached
        xd = x.astype(np.float64)
        assert np.array_equal(xd * 2.0 ** gran, np.rint(xd * 2.0 ** gran))
        sq = (x * x).astype(np.float64)                                   # the float32 product, as the kernel and the reference take it
        assert np.array_equal(sq * 4.0 ** gran, np.rint(sq * 4.0 ** gran)) and sq.max() < 4.0 ** maxb
        # sums of x and of x*x: forward, reversed and exactly rounded agree
        for v in (xd, sq):
            col = v[:, 1, 1]
            assert np.cumsum(col)[-1] == np.cumsum(col[::-1])[-1] == math.fsum(col)


def test_the_bit_budget_assertion_fires():
    rng = np.random.default_rng(2)
    assert forms.bit_budget(100000, 8, 7) == 17 + 14 + 16
    forms.exact_block(rng, (4,), 1.0, 8, 7, nsum=1 << 22)                 # 22 + 14 + 16 = 52
    with pytest.raises(AssertionError, match="not exact in double"):
        forms.exact_block(rng, (4,), 1.0, 8, 7, nsum=(1 << 22) + 1)
    with pytest.raises(AssertionError, match="not exact in double"):
        forms.exact_block(rng, (4,), 1.0, 8, 5, nsum=(1 << 26) + 1)
    with pytest.raises(AssertionError, match="float32"):
        forms.exact_block(rng, (4,), 1.0, 12, 13)
    # every case of the tables is inside the budget (rescale_blocks asserts it when it builds the data); the longest runs are the ones
    # the tables name
    assert max(e - s for s, e in forms.rescale_intervals(*forms.RESCALE_BIG["fpt-slices-double"][2:4])) > 4096 * 4096
    assert max(e - s for s, e in forms.rescale_intervals(*forms.RESCALE_BIG["tfp-slices-double"][2:4])) > 64 * 4096
    # one apply launch per piece (the part of a run inside one block): the two cases that are there for a cap of the apply kernels
    # hold a piece beyond it -- rows of k_rescale_pscrunch_digitize (gridDim.y 8192), samples per row of k_rescale_apply_fpt (256 x 256)
    longest = lambda name: max(e - s for s, e in forms.rescale_pieces(*forms.RESCALE_BIG[name][2:4]))
    assert longest("fused-rows-cap") > 8192 and longest("apply-fpt-cap") > 256 * 256
    assert longest("tfp-slices-double") * 4 > 4096 * 256 and longest("fpt-slices-double") > 256 * 256       # k_rescale_apply, _fpt
    assert forms.DIGITIZE_BIG["ndat"] * forms.DIGITIZE_BIG["nchan"] > 8192 * 256


def test_rescale_intervals_follow_the_state_machine(oracle):
    """rescale_intervals against what oracle.Rescale does, observed from outside on samples that are all 1: its running total is the
    number of samples since it last zeroed its sums.  (a) Every case of the tables, block by block as the GPU test calls it: after
    each block, position - total is the end of the last closed run.  (b) Short streams (the tables' own where they are short, and
    analogues of the long ones): the first segment as one call -- it fixes nsample and takes the "right after the first call"
    estimate --, then ONE SAMPLE PER CALL; the total is zero exactly after the samples that end a run."""
    one = lambda n: np.ones((n, 1, 1), np.float32)
    for name in list(forms.RESCALE_CASES) + list(forms.RESCALE_BIG):
        blocks, interval, constant = forms.rescale_case(name)[2:5]
        runs = forms.rescale_intervals(blocks, interval)
        assert runs[0][0] == 0 and runs[-1][1] == sum(blocks) and all(a[1] == b[0] for a, b in zip(runs, runs[1:])), name
        ro, pos = oracle.Rescale(interval, constant), 0
        for ndat in blocks:
            ro.transform(one(ndat))
            pos += ndat
            zeroed_at = pos - int(ro.total[0, 0])                          # where the oracle last zeroed its sums
            ends = [e for _, e in runs if e <= pos]
            # the end of the last run that ends inside the stream so far -- or, after the last block, the start of a run left open
            assert zeroed_at == max(ends) or (pos == sum(blocks) and zeroed_at == runs[-1][0]), (name, pos, zeroed_at)
    small = {"by-100": ((777, 777, 500), 100), "longer-than-a-block": ((300, 300, 700), 1000), "first-block": ((513, 200, 513), 0),
             "one-segment": ((90, 82), 0), "small-then-one-interval": ((10, 269), 269), "interval-1": ((3, 2), 1),
             "ragged": ((7, 1, 13, 2), 5), "exact-multiple": ((20, 20), 10)}
    for name in list(forms.RESCALE_CASES) + list(forms.RESCALE_BIG):
        blocks, interval = forms.rescale_case(name)[2:4]
        if sum(blocks) <= 3000:
            small[name] = (blocks, interval)
    assert len(small) >= 12
    for name, (blocks, interval) in small.items():
        total = sum(blocks)
        first = min(blocks[0], interval or blocks[0])
        ro, ends = oracle.Rescale(interval, False), []
        ro.transform(one(first))
        assert ro.total[0, 0] == 0.0, name                                # the estimate right after the first call
        ends.append(first)
        for pos in range(first + 1, total + 1):
            ro.transform(one(1))
            if ro.total[0, 0] == 0.0:
                ends.append(pos)
        runs = forms.rescale_intervals(blocks, interval)
        want = [e for _, e in runs]
        if ro.total[0, 0] != 0.0:                                         # the last run is still open
            assert want[-1] == total and total - int(ro.total[0, 0]) == runs[-1][0], name
            want = want[:-1]
        assert ends == want, (name, ends[:8], want[:8])


@pytest.mark.parametrize("name", list(forms.RESCALE_CASES) + list(forms.RESCALE_BIG))
def test_the_reference_does_not_depend_on_the_order_of_its_sums(oracle, name):
    """oracle.Rescale on the case's stream and on the stream with the samples of every run reversed in time (block by block): identical
    offset and scale after every block, identical output (sample for sample, reversed back); and the totals it divides equal
    math.fsum's and those of the whole run added backwards."""
    nchan, npol, blocks, interval, constant, _, _, _, _ = forms.rescale_case(name)
    xs = forms.rescale_blocks(name)
    stream = np.concatenate(xs, axis=0)
    runs = forms.rescale_intervals(blocks, interval)
    # reversed inside every piece a run has in one block: a run that spans blocks leaves its first pieces with the estimate still in
    # force and its last piece with the new one (Rescale.C:298-352), so only samples of one piece may change places
    pieces = forms.rescale_pieces(blocks, interval)
    perm = np.concatenate([np.arange(s, e)[::-1] for s, e in pieces])
    assert np.array_equal(np.sort(perm), np.arange(len(stream)))
    rev = stream[perm]
    ra, rb, pos = oracle.Rescale(interval, constant), oracle.Rescale(interval, constant), 0
    out_a, out_b = [], []
    for ndat in blocks:
        out_a.append(ra.transform(stream[pos:pos + ndat]))
        out_b.append(rb.transform(rev[pos:pos + ndat]))
        assert np.array_equal(ra.offset.view(np.int32), rb.offset.view(np.int32)), name
        assert np.array_equal(ra.scale.view(np.int32), rb.scale.view(np.int32)), name
        pos += ndat
    assert np.array_equal(ra.total, rb.total) and np.array_equal(ra.totalsq, rb.totalsq), name      # (the run left open: whole in both)
    a, b = np.concatenate(out_a, axis=0), np.concatenate(out_b, axis=0)
    assert np.isfinite(a).all() and np.array_equal(a[perm].view(np.int32), b.view(np.int32)), name
    assert ra.scale[0, 0] == 1.0 or constant or len(runs) > 1                # the zero-variance column of the first block
    # the sums of every run, three ways, on a few columns (all of them where that is cheap)
    cols = [(c, p) for c in range(nchan) for p in range(npol)]
    if len(stream) * len(cols) > 2000000:
        cols = cols[:2]
    for s, e in runs:
        for c, p in cols:
            v = stream[s:e, c, p].astype(np.float64)
            q = (stream[s:e, c, p] * stream[s:e, c, p]).astype(np.float64)
            assert np.cumsum(v)[-1] == np.cumsum(v[::-1])[-1] == math.fsum(v), (name, s, e, c, p)
            assert np.cumsum(q)[-1] == np.cumsum(q[::-1])[-1] == math.fsum(q), (name, s, e, c, p)


def test_tscrunch_ref_restates_the_reference_loop(oracle):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 2, 61)).astype(np.float32)
    for sf in (1, 4, 7):
        assert np.array_equal(forms.tscrunch_ref(x, sf, 1), oracle.tscrunch_fpt(x, sf))
    for ndim in (2, 4):
        ndat, sf = 23, 5
        x = (rng.standard_normal((3, 2, ndat * ndim)) * 100).astype(np.float32)
        want = np.zeros((3, 2, (ndat // sf) * ndim), np.float32)
        for c in range(3):
            for p in range(2):
                for o in range(ndat // sf):
                    for d in range(ndim):
                        acc = x[c, p, o * sf * ndim + d]
                        for j in range(1, sf):
                            acc = np.float32(acc + x[c, p, (o * sf + j) * ndim + d])
                        want[c, p, o * ndim + d] = acc
        assert np.array_equal(forms.tscrunch_ref(x, sf, ndim).view(np.int32), want.view(np.int32))


def test_stream_reference_and_the_tscrunch_table():
    """the calls of every stream put together are the scrunch of the whole stream; the carry is the literal running sum; the table
    holds the calls the issue names"""
    rng = np.random.default_rng(4)
    seen = set()
    for name, nchan, npol, ndim, sf, blocks, place in forms.TSCRUNCH_CASES:
        x = (rng.standard_normal((nchan, npol, sum(blocks) * ndim)) * 100).astype(np.float32)
        calls = forms.stream_reference(x, blocks, sf, ndim)
        assert np.array_equal(np.concatenate([c["out"] for c in calls], axis=2), forms.tscrunch_ref(x, sf, ndim)), name
        pos = 0
        for n, c in zip(blocks, calls):
            assert c["nout"] == (pos + n) // sf - pos // sf and c["carry_count"] == (pos + n) % sf and c["c0"] == pos % sf, name
            assert (c["carry"] is None) == (c["carry_count"] == 0), name
            if c["carry"] is not None:
                open_ = x.reshape(nchan, npol, -1, ndim)[:, :, pos + n - c["carry_count"]:pos + n]
                acc = open_[:, :, 0]
                for i in range(1, open_.shape[2]):
                    acc = acc + open_[:, :, i]
                assert np.array_equal(c["carry"], acc), name
            if ndim in (1, 2, 4):
                seen.add((ndim, "nout0" if c["nout"] == 0 else "out"))
                seen.add((ndim, "rem0" if c["carry_count"] == 0 else "rem"))
                if c["c0"] and c["carry_count"] and c["nout"]:
                    seen.add((ndim, "begins and ends inside"))
                if c["c0"] and c["nout"] == 0:
                    seen.add((ndim, "nout0 behind a carry"))
                if c["nout"] * ndim > 256:
                    seen.add((ndim, "more than a workgroup"))
                if c["nout"] * ndim > 1024 * 256:
                    seen.add((ndim, "beyond the grid cap"))
            pos += n
    for ndim in (1, 2, 4):
        for what in ("nout0", "rem0", "begins and ends inside", "nout0 behind a carry", "more than a workgroup"):
            assert (ndim, what) in seen, (ndim, what)
    assert any(what == "beyond the grid cap" for _, what in seen)


def test_the_tables_hold_the_shapes_the_kernels_branch_on():
    assert {c[4] for c in forms.FSCRUNCH_CASES} >= {1, 2, 3, 6} and all(c[3] % 256 for c in forms.FSCRUNCH_CASES)
    assert any(forms.PLACEMENTS[c[5]][0][2] and c[4] > 1 for c in forms.FSCRUNCH_CASES)             # plane-major input, scrunched
    assert any(c[3] > 1024 * 256 for c in forms.FSCRUNCH_CASES)
    floats = {(c[3] * c[4], c[6]) for c in forms.SAMPLE_DELAY_CASES}
    assert {(2047, False), (2048, False), (2049, False), (2047, True), (2049, True)} <= floats
    assert {c[3] for c in forms.SAMPLE_DELAY_CASES} >= {1, 2, 4} and {c[5] for c in forms.SAMPLE_DELAY_CASES} == {False, True}
    for ndim in (1, 2, 4):
        assert {c[6] for c in forms.SAMPLE_DELAY_CASES if c[3] == ndim} == {False, True}
    rng = np.random.default_rng(5)
    for absolute in (False, True):
        d = forms.sample_delays(rng, 5, 2, absolute)
        assert d.min() == 0 and d.max() == forms.SAMPLE_DELAY_MAX and d.shape == (5, 2)
    for name, (nchan, npol, blocks, interval, constant, flip, swap, bits, why) in {**forms.RESCALE_CASES, **forms.RESCALE_BIG}.items():
        assert nchan % 8 == 0 or name in forms.RESCALE_BIG, name
    assert all(v[0] % 64 and (v[0] * v[1]) % 256 for v in forms.RESCALE_CASES.values())
    assert {v[1] for v in forms.RESCALE_CASES.values()} == {1, 2, 4}
    offs_in = {p[0][0] for p in forms.PLACEMENTS}
    offs_out = {p[1][0] for p in forms.PLACEMENTS}
    assert offs_in == offs_out == {0, 1, 2, 3}
    assert {p[0][1] for p in forms.PLACEMENTS} == {p[1][1] for p in forms.PLACEMENTS} == {0, 1, 3}
    assert any(p[0][2] for p in forms.PLACEMENTS) and any(p[1][2] for p in forms.PLACEMENTS)
    # every kernel of the three files is named with where it is reached
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dspsr_amd", "csrc")
    kernels = set()
    for f in ("scrunch.hip", "sample_delay.hip", "rescale.hip"):
        kernels |= set(re.findall(r"__global__[^\n]*?void (k_\w+)", open(os.path.join(csrc, f)).read()))
    assert kernels == set(forms.KERNELS), kernels ^ set(forms.KERNELS)


def test_the_sentinel_masks_cover_exactly_what_a_correct_writer_touches():
    """every output layout the GPU tests build (scrunch outputs, the carry, SampleDelay rows, FPT Rescale rows): the mask of
    device_buffers.written_mask equals the documented address arithmetic written out (place_parts)"""
    layouts = []
    for name, nchan, npol, ndim, sf, blocks, place in forms.TSCRUNCH_CASES:
        pos = 0
        for n in blocks:
            nout = (pos + n) // sf - pos // sf
            layouts.append((forms.layout(nchan, npol, (nout + 1) * ndim, forms.PLACEMENTS[place][1]), nout * ndim))
            pos += n
        layouts.append((forms.layout(nchan, npol, ndim, (1, 0, False)), ndim))                       # the carry: [row][ndim], dense
    for name, nchan, npol, nfloat, sf, place in forms.FSCRUNCH_CASES:
        layouts.append((forms.layout(nchan // sf, npol, nfloat + 2, forms.PLACEMENTS[place][1]), nfloat))
    for name, nchan, npol, ndim, nout, absolute, inplace, place in forms.SAMPLE_DELAY_CASES:
        row = (nout + (forms.SAMPLE_DELAY_MAX if inplace else 1)) * ndim
        layouts.append((forms.layout(nchan, npol, row, forms.PLACEMENTS[place][1]), nout * ndim))
    for name, v in forms.RESCALE_CASES.items():
        for ndat in v[2]:
            for place in forms.PLACEMENTS:
                layouts.append((forms.layout(v[0], v[1], ndat + 1, place[1]), ndat))
    assert len(layouts) >= 80
    for lay, n in layouts:
        m = written_mask(lay, 1 if n else 0, n, n)
        assert m.sum() == lay.nchan * lay.nplanes * n
        bits = np.full(lay.size, SENTINEL, np.int32)
        values = np.arange(1, 1 + lay.nchan * lay.nplanes * n, dtype=np.int32).reshape(lay.nchan, lay.nplanes, 1 if n else 0, n)
        place_parts(lay, bits, values, n)
        assert np.array_equal(bits != SENTINEL, m) and np.array_equal(np.sort(bits[m]), values.ravel())
