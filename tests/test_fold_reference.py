"""CPU checks of tests/fold_reference.py, the restatement of the stand-alone fold the GPU fold tests compare with: exact on sums
that every association gets right, equal where the two associations coincide, different where they do not (so a test can tell
them apart), and the host's kernel choice on a worked case at each of its boundaries."""
import numpy as np
import pytest

from fold_reference import (FOLD_CHUNK, fold_dispatch, fold_long_model, fold_time_order, long_segments, plan_span,
                            runs_of_plan)


def _random_runs(rng, nbin, ndat, lo, hi, idat_start=0, force=None):
    """runs of random lengths in [lo, hi] and random bins (never the bin of the run before), covering [idat_start, ndat)"""
    runs, off, b = [], idat_start, -1
    while off < ndat:
        n = int(force) if force is not None and not runs else int(rng.integers(lo, hi + 1))
        n = min(n, ndat - off)
        nb = int(rng.integers(0, nbin - 1))
        b = nb + (nb >= b) if b >= 0 else nb
        runs.append((off, b, n))
        off += n
    return np.array(runs, np.int64)


def _exact_sums(rows, runs, prof):
    out = prof.astype(np.float64)
    for off, b, n in runs:
        out[:, :, b, :] += rows[:, :, off:off + n, :].astype(np.float64).sum(axis=2)
    return out


def test_runs_of_plan_match_set_bin():
    plan = np.array([3, 3, 1, 1, 1, 3, 0, 0], np.uint32)
    assert runs_of_plan(plan, 10).tolist() == [[10, 3, 2], [12, 1, 3], [15, 3, 1], [16, 0, 2]]
    assert plan_span(runs_of_plan(plan, 10)) == (8, 18)


def test_time_order_equals_the_explicit_loop():
    """the vectorised step-by-step sums are the per-sample loop of Fold.C:844-852 in float32"""
    rng = np.random.default_rng(1)
    nchan, npol, ndat, ndim, nbin = 3, 2, 1500, 2, 17
    rows = (rng.standard_normal((nchan, npol, ndat, ndim)) * 3.0).astype(np.float32)
    prof = rng.standard_normal((nchan, npol, nbin, ndim)).astype(np.float32)
    runs = _random_runs(rng, nbin, ndat, 1, 90, idat_start=7)
    want = prof.copy()
    for off, b, n in runs:
        for t in range(off, off + n):
            want[:, :, b, :] += rows[:, :, t, :]
    before = prof.copy()
    got = fold_time_order(rows, runs, prof)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(prof, before)                                       # the input profile is left as it was


@pytest.mark.parametrize("ncu", [1, 4, 256])
def test_integer_data_every_association_is_exact(ncu):
    """integer-valued samples (every partial sum < 2^24): time order, the LONG model and the float64 sums agree exactly"""
    rng = np.random.default_rng(2)
    nchan, npol, ndim, nbin, ndat = 2, 2, 2, 5, 9000
    rows = rng.integers(-50, 50, (nchan, npol, ndat, ndim)).astype(np.float32)
    prof = rng.integers(-1000, 1000, (nchan, npol, nbin, ndim)).astype(np.float32)
    runs = _random_runs(rng, nbin, ndat, 20, 300, idat_start=5)
    want = _exact_sums(rows, runs, prof)
    assert np.array_equal(fold_time_order(rows, runs, prof).astype(np.float64), want)
    assert np.array_equal(fold_long_model(rows, runs, prof, nchan * npol, ncu).astype(np.float64), want)


def test_long_model_is_time_order_without_whole_micro_blocks():
    """one segment, no run holding a whole aligned 32-sample micro-block, an empty profile: the LONG association is the time
    order (into a profile that holds sums it is not: the segment is summed from zero and then added)"""
    rng = np.random.default_rng(3)
    nchan, npol, ndim, nbin, ndat = 4, 1, 4, 9, 5000
    rows = rng.standard_normal((nchan, npol, ndat, ndim)).astype(np.float32) ** 2
    prof = np.zeros((nchan, npol, nbin, ndim), np.float32)
    runs = _random_runs(rng, nbin, ndat, 1, 31, idat_start=2)
    first, last = plan_span(runs)
    assert runs[:, 2].max() < 32 and last - first > 2 * FOLD_CHUNK
    nrow = nchan * npol
    assert long_segments(-(-(last - first) // FOLD_CHUNK), nrow, 1)[0] == 1
    assert np.array_equal(fold_long_model(rows, runs, prof, nrow, 1), fold_time_order(rows, runs, prof))


@pytest.mark.parametrize("ncu", [1, 256])
def test_long_model_differs_from_time_order_on_float_data(ncu):
    """long runs of float samples: the two associations round differently (the GPU test can tell them apart), and equal to
    float rounding"""
    rng = np.random.default_rng(4)
    nchan, npol, ndim, nbin, ndat = 3, 1, 4, 8, 20000
    rows = rng.standard_normal((nchan, npol, ndat, ndim)).astype(np.float32) ** 2
    prof = np.zeros((nchan, npol, nbin, ndim), np.float32)
    runs = _random_runs(rng, nbin, ndat, 64, 700, idat_start=3)
    a, b = fold_long_model(rows, runs, prof, nchan * npol, ncu), fold_time_order(rows, runs, prof)
    want = _exact_sums(rows, runs, prof)
    assert not np.array_equal(a, b)
    assert np.abs(a - want).max() <= 2e-6 * np.abs(want).max() and np.abs(b - want).max() <= 2e-6 * np.abs(want).max()


def test_long_model_segment_order_matters():
    """three segments added to a profile that holds sums: adding them in another order changes bits (what k_fold_combine's
    order test rests on)"""
    rng = np.random.default_rng(5)
    nchan, npol, ndim, nbin, ndat = 1, 1, 4, 4, 3 * FOLD_CHUNK
    rows = rng.standard_normal((nchan, npol, ndat, ndim)).astype(np.float32) ** 2
    prof = rng.standard_normal((nchan, npol, nbin, ndim)).astype(np.float32) * 100
    runs = _random_runs(rng, nbin, ndat, 64, 200)
    assert long_segments(3, 1, 256) == (3, 1)
    a = fold_long_model(rows, runs, prof, 1, 256)
    one = fold_long_model(rows, runs, prof, 1024, 256)          # nrow >= 4 ncu: one segment
    assert not np.array_equal(a, one)


def _case(nbin, runs, nchan=1, npol=1, ndim=4, addr=0, cs=None, ps=None, ncu=256):
    ndat = int(runs[-1][0] + runs[-1][2])
    ps = ndat * ndim if ps is None else ps
    cs = npol * ps if cs is None else cs
    return fold_dispatch(addr, cs, ps, nchan, npol, ndim, nbin, np.array(runs, np.int64), ncu)


def _periodic(nbin, spb, ndat, start=0):
    """runs of spb samples sweeping the bins in order"""
    return [(o, (i % nbin), min(spb, ndat - o)) for i, o in enumerate(range(start, ndat, spb))]


def test_dispatch_worked_cases():
    # longest run 63 / 64 (fold_fold_impl `lng`)
    r63 = [(0, 0, 63), (63, 1, 10), (73, 0, 5000)]
    assert _case(64, [(0, 0, 63), (63, 1, 1)] * 1)["kernel"] != "long"
    assert _case(64, r63)["kernel"] == "long"
    short = [(o, (o // 63) % 40, 63) for o in range(0, 63 * 400, 63)]
    longr = short[:-1] + [(short[-1][0], short[-1][1], 64)]
    assert _case(40, short, nchan=64)["kernel"] in ("chunked", "dense")
    assert _case(40, longr, nchan=64)["kernel"] == "long"
    # nbin 4096 / 4097 (`chunked`)
    runs = _periodic(4097, 2, 40000)
    assert _case(4096, [(o, b % 4096, n) for o, b, n in runs], nchan=600)["kernel"] in ("chunked", "dense")
    assert _case(4097, runs, nchan=600)["kernel"] == "direct"
    # one run per (chunk, bin) or two (plan_scan): period 64 x 40 = 2560 > FOLD_CHUNK, and 64 x 20 = 1280 < FOLD_CHUNK
    assert _case(64, _periodic(64, 40, 30000), nchan=8)["kernel"] == "dense"
    assert _case(64, _periodic(64, 20, 30000), nchan=8)["kernel"] == "chunked"
    # dense table size (plan_scan): 4 * ntab <= data words -- 10 chunks x 512 bins against 20480 / 20479 samples of one row
    assert _case(512, _periodic(512, 20, 20480), nchan=1, ndim=1)["kernel"] == "dense"
    assert _case(512, _periodic(512, 20, 20479), nchan=1, ndim=1, ps=20480)["kernel"] == "chunked"
    # ... and ntab <= 2^24 (plan_scan): 4096 chunks x 4096 bins fit, one more chunk does not
    assert _case(4096, _periodic(4096, 63, 4096 * FOLD_CHUNK), nchan=4)["kernel"] == "dense"
    assert _case(4096, _periodic(4096, 63, 4096 * FOLD_CHUNK + 1), nchan=4)["kernel"] == "chunked"
    # alignment (`aligned`): address, channel stride, polarisation stride
    base = _periodic(64, 40, 30000)
    assert _case(64, base, nchan=8, addr=4)["kernel"] == "direct"
    assert _case(64, base, nchan=8, addr=16)["kernel"] == "dense"
    assert _case(64, base, nchan=8, cs=30000 * 4 + 2)["kernel"] == "direct"
    assert _case(64, base, nchan=8, npol=2, ndim=2, ps=30000 * 2 + 1)["kernel"] == "direct"
    # bin split and threads (`nsplit`, `threads`)
    assert _case(512, _periodic(512, 3, 8000), nchan=2)["nsplit"] == 8
    assert _case(512, _periodic(512, 3, 8000), nchan=2)["threads"] == 256
    c = _case(4096, _periodic(4096, 1, 8000), nchan=130, npol=2, ndim=2)
    assert (c["kernel"], c["nsplit"], c["threads"]) == ("dense", 2, 512)
    c = _case(4096, _periodic(4096, 1, 8000), nchan=600, npol=1, ndim=4)
    assert (c["nsplit"], c["threads"]) == (1, 1024)
    assert _case(100, _periodic(100, 3, 8000), nchan=2)["nsplit"] == 1          # 100 / 2 < 64
    # rows per workgroup (`nrw`): nchan * nsplit >= 2 ncu
    assert _case(200, _periodic(200, 3, 4000), nchan=512, npol=2, ndim=2)["nrow"] == 2
    assert _case(200, _periodic(200, 3, 4000), nchan=511, npol=2, ndim=2)["nrow"] == 1
    assert _case(200, _periodic(200, 3, 4000), nchan=520, npol=4, ndim=1)["nrow"] == 4
    assert _case(200, _periodic(200, 3, 4000), nchan=520, npol=4, ndim=1, ncu=304)["nrow"] == 1
    # LONG segments (`nseg`, `cps`): nseg from ncu and nchan * npol, rows per workgroup against nchan * nseg
    c = _case(16, _periodic(16, 100, 20000), nchan=3)
    assert (c["kernel"], c["nseg"], c["cps"]) == ("long", 10, 1)
    c = _case(16, _periodic(16, 100, 40000), nchan=200)
    assert (c["nseg"], c["cps"]) == (5, 4)
    c = _case(16, _periodic(16, 100, 12000), nchan=200, npol=2, ndim=2)
    assert (c["kernel"], c["nseg"], c["nrow"]) == ("long", 3, 2)
    c = _case(16, _periodic(16, 100, 5000), nchan=520, npol=4, ndim=1)
    assert (c["kernel"], c["nseg"], c["nrow"]) == ("long", 1, 4)
