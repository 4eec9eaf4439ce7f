"""The fold engine's plan builders (dspsr_amd/csrc/fold_plan.h: pure host C++, standard headers only) against the Python
restatements the GPU tests rely on.

tests/fold_plan_driver.cpp includes only that header; it is built with g++ and the address and undefined-behaviour sanitizers and
run as a stand-alone program (nothing is loaded into Python).  Its output buffers have exactly the sizes the builders' count
functions return, so a builder that writes past its table ends the driver with a sanitizer report and a non-zero exit code.

  plan_bucket            a stable sort by bin in numpy
  plan_scan              fold_reference.fold_dispatch: the dense decision and the longest run
  plan_dense_fill        a direct table built from the runs, s0 | n << 11 per (chunk, bin)
  part_plan_*            fused_fold_cases.part_plan, for every call of every case of fused_fold_cases
  segment_plan_*         the qualification the segsum cases name; run_off / blk_first from np.searchsorted
  fold_shape             fold_reference.fold_dispatch and long_segments: kernel family, <ND, NR>, grid, threads, LDS, segments
  fold_many_shape        fold_reference.fold_many_dispatch
  fold_moments_shape     moments_cases.geometry
"""
import os
import subprocess

import numpy as np
import pytest

import fused_fold_cases as fc
import moments_cases as mc
from fold_reference import FOLD_BPT, FOLD_CHUNK, FOLD_LONG_RUN, FOLD_MANY_THREADS, FOLD_MB, fold_dispatch, fold_many_dispatch, long_segments, plan_span

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fold_plan") / "fold_plan_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "dspsr_amd", "csrc"), os.path.join(ROOT, "tests", "fold_plan_driver.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr.strip() == "", p.stderr[-4000:]              # -Wall -Wextra clean

    def run(cases):
        """cases: dicts of the header fields and `runs`; returns one dict of name -> int64 array per case"""
        text = []
        for c in cases:
            if c["op"].endswith("_shape"):                           # the launch shapes: one line of plain numbers
                text.append("%s %d %d %d %d %d %d %d %d %d %d %d %d %d" % (
                    c["op"], c.get("aligned", 1), c["nchan"], c.get("npol", 1), c.get("ndim", 4), c.get("nbin", 0), c.get("first", 0),
                    c.get("last", 0), c.get("max_run", 0), c.get("dense", 0), c["ncu"], c.get("nslot", 0), mc.MOM_THREADS,
                    mc.MOM_BPT * mc.MOM_THREADS))
                continue
            runs = np.asarray(c["runs"], np.int64).reshape(-1, 3)
            text.append("%s %d %d %d %d %d %d %d %d %d %d %d" % (
                c["op"], c["nbin"], c.get("row_words", 4), c.get("try_dense", 1), c.get("first", 0), c.get("last", 0), c.get("nkeep", 1),
                c.get("npart", 0), c.get("ndat", 0), c.get("seg", 0), c.get("open_hits", 0), len(runs)))
            text.extend("%d %d %d" % (o, b, n) for o, b, n in runs.tolist())
        p = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-4000:])
        out, cur = [], None
        for line in p.stdout.splitlines():
            if line.startswith("begin"):
                cur = {}
            elif line == "end":
                out.append(cur)
            else:
                name, _, vals = line.partition(":")
                cur[name] = np.array(vals.split(), np.int64)
        assert len(out) == len(cases)
        return out
    return run


def _periodic(nbin, spb, ndat, start=0):
    """runs of spb samples sweeping the bins in order"""
    return [(o, i % nbin, min(spb, ndat - o)) for i, o in enumerate(range(start, ndat, spb))]


def _random_runs(seed, nbin, nrun, max_hits, start=0, zero_hits=False):
    """runs laid end to end, neighbouring bins different, some bins back again soon (several runs of a bin inside a chunk)"""
    rng = np.random.default_rng(seed)
    out, t, prev = [], start, -1
    for _ in range(nrun):
        b = int(rng.integers(0, nbin))
        if b == prev:
            b = (b + 1) % nbin
        n = int(rng.integers(0 if zero_hits else 1, max_hits + 1))
        out.append((t, b, n))
        t += n
        prev = b
    return out


# (nbin, runs, nchan, npol, ndim): plans of the stand-alone fold, the hand-made edges among them
C = FOLD_CHUNK
FOLD_PLANS = {
    "period-above-chunk": (64, _periodic(64, 40, 30000), 8, 1, 4),
    "period-below-chunk": (64, _periodic(64, 20, 30000), 8, 1, 4),
    "first-not-multiple-of-4": (64, _periodic(64, 40, 30000, start=1003), 8, 2, 2),
    "run-ends-at-a-chunk-end": (64, _periodic(64, 32, 3 * C + 7), 16, 1, 4),          # 64 runs of 32 samples fill a chunk
    "run-across-three-chunks": (8, [(0, 0, 30), (30, 1, 2 * C + 100), (2 * C + 130, 2, 50), (2 * C + 180, 0, 40)], 16, 1, 4),
    "two-runs-of-a-bin-in-a-chunk": (8, [(0, 0, 30), (30, 1, 30), (60, 0, 30), (90, 2, 3 * C)], 16, 1, 4),
    # bin 1 comes back in chunk 1, where its first run ENDS (the run crosses the chunk end): refused as well
    "second-run-in-the-chunk-a-run-ends-in": (8, [(0, 0, C - 10), (C - 10, 1, 30), (C + 20, 2, 30), (C + 50, 1, 30)], 16, 1, 4),
    "zero-hit-run": (8, [(0, 0, 30), (30, 1, 0), (30, 2, 30), (60, 1, 0), (60, 3, C)], 16, 1, 4),
    "runs-to-63": (40, [(o, (o // 63) % 40, 63) for o in range(0, 63 * 400, 63)], 64, 1, 4),
    "runs-to-64": (40, [(o, (o // 63) % 40, 63) for o in range(0, 63 * 399, 63)] + [(63 * 399, 39, 64)], 64, 1, 4),
    "with-a-gap": (16, [(8, 0, 50), (58, 1, 50), (500, 2, 50), (550, 0, 3000)], 4, 1, 4),
    # the table may take a quarter of the words it helps to fold: one chunk of 2048 one-float samples, 512 bins and 513
    "table-at-a-quarter-of-the-data": (512, _periodic(512, 4, C), 1, 1, 1),
    "table-one-word-past-a-quarter": (513, _periodic(513, 4, C), 1, 1, 1),
    "table-10-chunks-at-a-quarter": (512, _periodic(512, 20, 20480), 1, 1, 1),
    "table-10-chunks-past-a-quarter": (512, _periodic(512, 20, 20479), 1, 1, 1),
    "random-short": (37, _random_runs(1, 37, 900, 9, start=5), 3, 2, 2),
    "random-zero-hits": (5, _random_runs(2, 5, 700, 3, zero_hits=True), 3, 4, 1),
}
# the 2^24-entry limit of the table: 4096 chunks x 4096 bins fit, one more chunk does not (scan only: the table is 64 MiB)
BIG_PLANS = {
    "table-2^24-entries": (4096, _periodic(4096, 63, 4096 * C), 4, 1, 4),
    "table-2^24-entries-and-a-chunk": (4096, _periodic(4096, 63, 4096 * C + 1), 4, 1, 4),
}
EXPECT_KERNEL = {"period-above-chunk": "dense", "period-below-chunk": "chunked", "run-ends-at-a-chunk-end": "dense",
                 "run-across-three-chunks": "long", "two-runs-of-a-bin-in-a-chunk": "long", "second-run-in-the-chunk-a-run-ends-in": "long",
                 "runs-to-64": "long", "table-at-a-quarter-of-the-data": "dense",
                 "table-one-word-past-a-quarter": "chunked", "table-10-chunks-at-a-quarter": "dense", "table-10-chunks-past-a-quarter": "chunked",
                 "table-2^24-entries": "dense", "table-2^24-entries-and-a-chunk": "chunked", "zero-hit-run": "long"}


def _fold_case(op, plan, **kw):
    nbin, runs, nchan, npol, ndim = plan
    first, last = plan_span(runs)
    return dict(op=op, nbin=nbin, runs=runs, row_words=nchan * npol * ndim, first=first, last=last, **kw)


def test_bucket_is_a_stable_sort_by_bin(driver):
    names = list(FOLD_PLANS)
    plans = [FOLD_PLANS[n] for n in names]
    # ... and the plans of the fused cases, as the segment plan and the fourth moments bucket them
    for name in fc.of_group("runs") + fc.of_group("segsum"):
        c = fc.by_name(name)
        plans.append((c["nbin"], fc.call_runs(name, 0)[0], 1, 1, 4))
        names.append(name)
    got = driver([_fold_case("bucket", p) for p in plans])
    for name, (nbin, runs, *_), g in zip(names, plans, got):
        runs = np.asarray(runs, np.int64).reshape(-1, 3)
        order = np.argsort(runs[:, 1], kind="stable")
        want_iv = np.stack([runs[order, 0], runs[order, 2], np.zeros(len(runs), np.int64)], axis=1).ravel()
        want_start = np.concatenate(([0], np.cumsum(np.bincount(runs[:, 1], minlength=nbin))))
        assert np.array_equal(g["bin_start"], want_start), name
        assert np.array_equal(g["iv"], want_iv), name


def test_scan_agrees_with_fold_dispatch(driver):
    plans = dict(FOLD_PLANS, **BIG_PLANS)
    names = list(plans)
    got = driver([_fold_case("scan", plans[n], open_hits=7) for n in names]
                 + [_fold_case("scan", plans[n], try_dense=0, open_hits=100000) for n in names])
    for i, name in enumerate(names):
        nbin, runs, nchan, npol, ndim = plans[name]
        runs = np.asarray(runs, np.int64).reshape(-1, 3)
        first, last = plan_span(runs)
        disp = fold_dispatch(0, 0, 0, nchan, npol, ndim, nbin, runs, 256)          # (aligned rows: the chunk kernels)
        max_run, ntab, one, open_max = got[i]["scan"].tolist()
        assert max_run == int(runs[:, 2].max()), name
        assert open_max == max(max_run, 7), name                        # plan_max_run with the open run's hits
        assert ntab == -(-(last - first) // FOLD_CHUNK) * nbin, name
        assert (max_run >= FOLD_LONG_RUN) == (disp["kernel"] == "long"), name
        assert (bool(one) and max_run < FOLD_LONG_RUN) == (disp["kernel"] == "dense"), name
        if name in EXPECT_KERNEL:
            assert disp["kernel"] == EXPECT_KERNEL[name], name
        # no table wanted (k_fold_direct, the fourth moments): the longest run alone
        assert got[len(names) + i]["scan"].tolist() == [max_run, 0, 0, 100000], name
    # the refusals are the walk's, not only the LONG rule's: the same plans with their long runs shortened are still refused
    short = {n: (FOLD_PLANS[n][0], [(o, b, min(h, 40)) for o, b, h in FOLD_PLANS[n][1]]) + FOLD_PLANS[n][2:]
             for n in ("two-runs-of-a-bin-in-a-chunk", "second-run-in-the-chunk-a-run-ends-in", "run-across-three-chunks", "zero-hit-run")}
    got = driver([_fold_case("scan", short[n]) for n in short])
    assert [g["scan"][2] for g in got] == [0, 0, 1, 1]


def _dense_table(nbin, runs, first, last):
    nchunk = -(-(last - first) // FOLD_CHUNK)
    tab = np.zeros((nchunk, nbin), np.int64)
    for off, b, n in np.asarray(runs, np.int64).reshape(-1, 3).tolist():
        s, e = off - first, off - first + n
        while s < e:
            c = s // FOLD_CHUNK
            hi = min(e, (c + 1) * FOLD_CHUNK)
            assert tab[c, b] == 0, "two runs of a bin in a chunk"
            tab[c, b] = (s - c * FOLD_CHUNK) | ((hi - s) << 11)
            s = hi
    return tab.ravel()


def test_dense_table_holds_one_run_per_chunk_and_bin(driver):
    names = list(FOLD_PLANS)
    got = driver([_fold_case("dense", FOLD_PLANS[n]) for n in names])
    ndense = 0
    for name, g in zip(names, got):
        nbin, runs, *_ = FOLD_PLANS[name]
        first, last = plan_span(runs)
        if not g["scan"][2]:
            assert "tab" not in g
            continue
        ndense += 1
        assert np.array_equal(g["tab"], _dense_table(nbin, runs, first, last)), name
    assert ndense >= 7
    # (plan_scan accepts a plan whatever its longest run: the LONG rule is the caller's)
    assert got[names.index("run-across-three-chunks")]["scan"][2] == 1 and got[names.index("run-ends-at-a-chunk-end")]["scan"][2] == 1


def _part_plan_tables(pp, npart):
    """the device layout of fold_plan.h from fused_fold_cases.part_plan's lists: start[0 .. npart], zeros up to a multiple of four
    words, the entries {bin, first interval, count << 16 | hits0, offset0}; the intervals (offset in the part, hits, 0)"""
    start, ent, iv = [], [], []
    for part in pp:
        start.append(len(ent) // 4)
        for b, ivs in part:
            ent += [b, len(iv), (len(ivs) << 16) | ivs[0][1], ivs[0][0]]
            iv += [(w, m, 0) for w, m in ivs]
    start.append(len(ent) // 4)
    start += [0] * (-(npart + 1) % 4)
    return np.array(start + ent, np.int64), np.array(iv, np.int64).ravel()


def _check_part_plans(driver, plans):
    """plans: (label, runs, nkeep, npart, nbin)"""
    got = driver([dict(op="part", nbin=nbin, runs=runs, nkeep=nkeep, npart=npart) for _l, runs, nkeep, npart, nbin in plans])
    for (label, runs, nkeep, npart, nbin), g in zip(plans, got):
        start, iv = _part_plan_tables(fc.part_plan(runs, nkeep, npart, nbin), npart)
        assert "beyond" not in g, label
        assert g["size"].tolist() == [len(iv) // 3, (len(start) - ((npart + 4) & ~3)) // 4, len(start)], label
        assert np.array_equal(g["start"], start), label
        assert np.array_equal(g["iv"], iv), label
    return got


def test_part_plan_of_every_fused_case(driver):
    plans = []
    for c in fc.CASES:
        for k, (parts, _plan) in enumerate(c["calls"]):
            plans.append(("%s call %d" % (c["name"], k), fc.call_runs(c["name"], k)[0], c["M"] - sum(c["nfilt"]), parts, c["nbin"]))
    assert {c["group"] for c in fc.CASES} == {"psl", "seg", "cap", "runs", "placement", "grid", "segsum"}
    _check_part_plans(driver, plans)


def test_part_plan_edges(driver):
    cut = [(0, 3, 5), (5, 1, 20), (25, 3, 2), (27, 0, 13)]                  # nkeep 10: run 1 is cut at samples 10 and 20
    got = _check_part_plans(driver, [
        ("a run cut by two part boundaries", cut, 10, 4, 4),
        ("... with parts to spare", cut, 10, 7, 4),
        ("a zero-hit run", [(0, 0, 4), (4, 1, 0), (4, 2, 9), (13, 1, 0)], 5, 3, 3),
        ("a zero-hit run behind the parts", [(0, 0, 10), (10, 1, 0)], 5, 2, 2),
        ("a gap of a whole part", [(0, 0, 7), (20, 1, 9)], 10, 3, 2),
        ("nothing to fold", np.zeros((0, 3), np.int64), 10, 3, 2),
        ("one part, one bin", [(0, 0, 10)], 10, 1, 1),
        ("npart + 1 a multiple of four", _periodic(3, 2, 30), 10, 3, 3),
    ])
    assert got[0]["size"].tolist() == [7, 7, 8 + 4 * 7] and got[5]["size"].tolist() == [0, 0, 4]
    # a sample beyond npart is refused and named: the last sample of the first run that reaches out
    got = driver([dict(op="part", nbin=4, runs=cut, nkeep=10, npart=3), dict(op="part", nbin=4, runs=cut, nkeep=10, npart=2),
                  dict(op="part", nbin=4, runs=[(0, 0, 10), (10, 1, 1)], nkeep=10, npart=1)])
    assert [g["beyond"].tolist() for g in got] == [[39], [24], [10]] and all("start" not in g for g in got)


def _segment_tables(runs, ndat):
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    run_off = np.concatenate((runs[:, 0], [ndat]))
    blk = np.searchsorted(runs[:, 0], np.arange((ndat >> 10) + 1) << 10, side="right") - 1
    return run_off, np.minimum(blk, len(runs) - 1)


def _check_segment(g, runs, nbin, ndat, label):
    runs = np.asarray(runs, np.int64).reshape(-1, 3)
    run_off, blk = _segment_tables(runs, ndat)
    assert np.array_equal(g["run_off"], run_off), label
    assert np.array_equal(g["blk_first"], blk), label
    order = np.argsort(runs[:, 1], kind="stable")
    assert np.array_equal(g["bin_start"], np.concatenate(([0], np.cumsum(np.bincount(runs[:, 1], minlength=nbin))))), label
    assert np.array_equal(g["iv"], np.stack([runs[order, 0], runs[order, 2], np.zeros(len(runs), np.int64)], axis=1).ravel()), label


def test_segment_plan_of_the_segsum_cases(driver):
    names = fc.of_group("segsum")
    assert names == ["segsum-exact", "segsum-one-short-interval", "segsum-one-sample-short"]
    cases = []
    for name in names:
        c, rec = fc.by_name(name), fc.record(name)
        runs, _hits, ndat = fc.call_runs(name, 0)
        cases.append(dict(op="segment", nbin=c["nbin"], runs=runs, ndat=ndat, seg=rec["seg"]))
    got = driver(cases)
    assert [int(g["qualifies"][0]) for g in got] == [1, 0, 0]
    assert [fc.record(n)["calls"][0]["path"] == "segsum" for n in names] == [True, False, False]
    _check_segment(got[0], cases[0]["runs"], cases[0]["nbin"], cases[0]["ndat"], names[0])
    assert "run_off" not in got[1] and "run_off" not in got[2]


def test_segment_plan_edges(driver):
    seg = 32
    ok = [(0, 0, 5), (5, 1, 32), (37, 2, 1500), (1537, 3, 32), (1569, 0, 3)]          # short first and last intervals
    n = 1572
    shift = lambda runs, k, d: [(o + (d if i > k else 0), b, h + (d if i == k else 0)) for i, (o, b, h) in enumerate(runs)]
    open_last = ok[:-1] + [(1569, 0, 0)]                                     # set_bin's open run: its hits are still zero
    cases = [
        ("short first and last intervals", ok, n, 0, 1),
        ("an inner interval of seg - 1 samples", shift(ok, 1, -1), n - 1, 0, 0),
        ("the first inner interval of seg samples, the last of seg - 1", shift(ok, 3, -1), n - 1, 0, 0),
        ("a gap", ok[:2] + [(o + 1, b, h) for o, b, h in ok[2:]], n + 1, 0, 0),
        ("a start behind sample 0", [(o + 4, b, h) for o, b, h in ok], n + 4, 0, 0),
        ("samples missing at the end", ok, n + 1, 0, 0),
        ("more samples than ndat", ok, n - 1, 0, 0),
        ("an open last run", open_last, n, 3, 1),
        ("an open last run of other hits", open_last, n, 2, 0),
        ("a closed last run of no hits", open_last, n - 3, 0, 0),
        ("open hits replace the stored ones", ok, n + 4, 7, 1),
        ("one run", [(0, 5, 4096)], 4096, 0, 1),                               # ndat a multiple of 1024: blk_first[4] past the data
        ("two runs", [(0, 5, 1), (1, 6, 1)], 2, 0, 1),
        ("no run", np.zeros((0, 3), np.int64), 0, 0, 0),
        ("ndat of 2^32", [(0, 0, 5)], 1 << 32, 0, 0),
    ]
    got = driver([dict(op="segment", nbin=8, runs=runs, ndat=ndat, seg=seg, open_hits=oh) for _l, runs, ndat, oh, _q in cases])
    for (label, runs, ndat, oh, q), g in zip(cases, got):
        assert int(g["qualifies"][0]) == q, label
        if q:
            closed = [tuple(r) for r in np.asarray(runs, np.int64).tolist()]
            if oh:
                closed[-1] = (closed[-1][0], closed[-1][1], oh)
            _check_segment(g, closed, 8, ndat, label)


# ---- the launch shapes (fold_plan.h fold_shape, fold_many_shape, fold_moments_shape) -------------------------------------------
FAMILY = {"direct": 0, "chunked": 1, "long": 2, "dense": 3, "many": 4, "moments": 5, "moments-long": 6}      # enum FoldFamily
NCUS = (256, 8)                                   # the MI355X and a small device: no rule may hide a constant in the other


def _short_plan(nbin, nchunk=2, tail=77):
    """runs of 5 samples sweeping the bins over nchunk chunks and a ragged end: no LONG run; dense or not as plan_scan finds"""
    return _periodic(nbin, 5, nchunk * C + tail, start=6)


def _long_plan(nbin, nsamp):
    """two runs, the second a LONG one up to sample nsamp"""
    return [(0, 0, 40), (40, nbin - 1, nsamp - 40)]


def _want_fold_shape(disp, nchan, npol, ndim):
    """the FoldShape line fold_dispatch stands for"""
    lng, nr = disp["kernel"] == "long", disp["nrow"]
    if disp["kernel"] == "direct":
        grid, lds = [npol, nchan, disp["nsplit"]], 0
    else:
        grid = [npol // nr, nchan, disp["nseg"] if lng else disp["nsplit"]]
        lds = (FOLD_CHUNK + (FOLD_CHUNK // FOLD_MB if lng else 0)) * ndim * nr * 4
    return [FAMILY[disp["kernel"]], ndim, nr] + grid + [disp["threads"], lds, disp["nseg"], disp["cps"]]


def _fold_shape_cases():
    """(label, addr, nchan, npol, ndim, nbin, runs): the edges of every rule of fold_shape"""
    out = []
    for nbin in (127, 128, 129, 255, 256, 1023, 1024, 1025, 4096, 4097):        # bin split, threads, the chunk kernels' limit
        for nchan in (1, 4):
            out.append(("nbin %d" % nbin, 0, nchan, 1, 4, nbin, _short_plan(nbin)))
    out.append(("unaligned rows", 4, 4, 1, 4, 256, _short_plan(256)))
    out.append(("unaligned rows, nbin above 1024", 8, 4, 2, 2, 1500, _short_plan(1500)))
    # nrow * nsplit at 511 / 512: 73 x 7 rows = 511 and one split more would pass 512; 128 x 4 = 512 rows are not split at all
    for nchan, npol, ndim in ((73, 7, 1), (511, 1, 4), (512, 1, 4), (128, 4, 1), (255, 2, 2), (256, 2, 2), (127, 4, 1)):
        out.append(("rows %d x %d" % (nchan, npol), 0, nchan, npol, ndim, 1024, _short_plan(1024, nchunk=1)))
    # rows per workgroup, exact: nchan * nsplit either side of 2 * ncu (512 and 16), nsplit 1 (many rows) and above
    for npol, ndim in ((1, 4), (2, 2), (4, 1), (2, 1)):
        for nchan in (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 511, 512, 513):
            for nbin in (512, 256):          # a period of 2560 samples: the dense table; of 1280: two runs of a bin in a chunk, the walk
                out.append(("nrw exact %d x %d x %d, nbin %d" % (nchan, npol, ndim, nbin), 0, nchan, npol, ndim, nbin, _short_plan(nbin, nchunk=1)))
    # LONG: fewer chunks than wanted segments, exactly one chunk, many chunks; rows per workgroup with nchan * nseg at 2 * ncu
    for npol, ndim in ((1, 4), (2, 2), (4, 1), (2, 1)):
        for nchan in (1, 3, 4, 5, 16, 127, 128, 129, 300, 600):
            for nsamp in (100, C, C + 1, 3 * C, 40 * C + 5):
                out.append(("long %d x %d x %d, %d samples" % (nchan, npol, ndim, nsamp), 0, nchan, npol, ndim, 64, _long_plan(64, nsamp)))
    return out


def test_fold_shape_agrees_with_fold_dispatch(driver):
    cases, want = [], []
    for ncu in NCUS:
        for label, addr, nchan, npol, ndim, nbin, runs in _fold_shape_cases():
            runs = np.asarray(runs, np.int64).reshape(-1, 3)
            disp = fold_dispatch(addr, 0, 0, nchan, npol, ndim, nbin, runs, ncu)
            first, last = plan_span(runs)
            cases.append(dict(op="fold_shape", aligned=int(addr % 16 == 0), nchan=nchan, npol=npol, ndim=ndim, nbin=nbin, first=first,
                              last=last, max_run=int(runs[:, 2].max()), dense=int(disp["kernel"] == "dense"), ncu=ncu))
            want.append(("%s, ncu %d" % (label, ncu), _want_fold_shape(disp, nchan, npol, ndim), disp))
    got = driver(cases)
    seen = set()
    for g, (label, w, disp) in zip(got, want):
        assert g["shape"].tolist() == w, (label, disp)
        seen.add((disp["kernel"], disp["ndim"], disp["nrow"]))
    # every instantiation of every chunk kernel is chosen somewhere, and k_fold_direct
    for kernel in ("chunked", "dense", "long"):
        assert {(nd, nr) for k, nd, nr in seen if k == kernel} == {(4, 1), (2, 2), (2, 1), (1, 4), (1, 1)}, kernel
    assert {k for k, _, _ in seen} == {"direct", "chunked", "long", "dense"}


def test_fold_shape_long_segments_at_the_clamp(driver):
    """nseg is clamped to 65535 (grid.z) before the chunks are dealt: a span of 70000 chunks on a device large enough to want
    more segments than that; and one chunk short of / at / beyond a multiple of the segment length"""
    cases, want = [], []
    for ncu, nchan, nchunk in ((1 << 15, 1, 70000), (1 << 15, 1, 65535), (1 << 15, 1, 65536), (1 << 15, 2, 131071), (256, 1, 70000),
                               (256, 1, 1024), (256, 1, 1025), (8, 1, 33), (8, 3, 11)):
        last = nchunk * C - 3
        nseg, cps = long_segments(nchunk, nchan, ncu)
        cases.append(dict(op="fold_shape", nchan=nchan, npol=1, ndim=4, nbin=64, first=0, last=last, max_run=last - 40, dense=0, ncu=ncu))
        want.append([FAMILY["long"], 4, 1, 1, nchan, nseg, 256, (C + C // FOLD_MB) * 16, nseg, cps])
        assert nseg <= 65535 and nseg * cps >= nchunk > (nseg - 1) * cps
    got = driver(cases)
    assert [g["shape"].tolist() for g in got] == want
    assert want[0][5] == 35000 and want[1][5] == 65535 and want[2][5] == 32768          # 70000 chunks: two per segment


def test_many_shape_agrees_with_fold_many_dispatch(driver):
    cases, want = [], []
    full = FOLD_BPT * FOLD_MANY_THREADS                                   # slots of one workgroup
    for ncu in NCUS:
        for npol, ndim in ((1, 4), (2, 2), (4, 1), (2, 1)):
            for nchan in (1, 3, 7, 8, 9, 127, 128, 129, 255, 256, 257, 512, 520):
                for nslot in (8, 127, 128, 129, 255, 256, 1023, 1024, 1025, full, full + 1, 2 * full, 2 * full + 1, 4 * full,
                              4 * full + 1, 8 * full + 1):
                    d = fold_many_dispatch(nchan, npol, ndim, nslot, ncu)
                    cases.append(dict(op="many_shape", nchan=nchan, npol=npol, ndim=ndim, nslot=nslot, ncu=ncu))
                    want.append([FAMILY["many"], ndim, d["nrow"], d["nz"], npol // d["nrow"], nchan, d["threads"],
                                 FOLD_CHUNK * ndim * d["nrow"] * 4, 1, 0])
                    assert d["nz"] * full >= nslot and d["threads"] * FOLD_BPT * d["nz"] >= nslot        # every slot has an owner
    got = driver(cases)
    assert [g["shape"].tolist() for g in got] == want
    assert {(w[1], w[2]) for w in want} == {(4, 1), (2, 2), (2, 1), (1, 4), (1, 1)}
    # FOLD_BPT * 512 * nz slots fit nz workgroups, one more doubles them
    one = {(c["nslot"], w[3]) for c, w in zip(cases, want) if c["nchan"] == 520 and c["npol"] == 1}
    assert {(full, 1), (full + 1, 2), (2 * full, 2), (2 * full + 1, 4), (4 * full, 4), (4 * full + 1, 8), (8 * full + 1, 16)} <= one


def test_moments_shape_agrees_with_geometry(driver):
    cases, want = [], []
    for ncu in NCUS:
        for nchan in (1, 5, 63, 64, 65, 511, 512, 513):
            for nbin in (64, 127, 128, 129, 255, 256, 512, 513, 1024, 1025, 4097):
                plans = [_short_plan(nbin, nchunk=1), _long_plan(nbin, 100), _long_plan(nbin, C), _long_plan(nbin, C + 1),
                         _long_plan(nbin, 9 * C + 7), _long_plan(nbin, 300 * C)]
                for runs in plans:
                    g = mc.geometry(nchan, nbin, runs, ncu)
                    cases.append(dict(op="moments_shape", nchan=nchan, ndim=mc.MOM_NDIM, nbin=nbin, first=g["first"], last=g["last"],
                                      max_run=g["max_run"], ncu=ncu))
                    want.append([FAMILY["moments-long" if g["lng"] else "moments"], mc.MOM_NDIM, 1, g["ngroup"], nchan, g["nseg"],
                                 mc.MOM_THREADS, 0, g["nseg"], g["seg_samples"]])
    got = driver(cases)
    assert [g["shape"].tolist() for g in got] == want
    assert any(w[0] == FAMILY["moments-long"] and w[9] == C and w[5] == 1 for w in want)            # nunit 1
    assert {w[3] for w in want} >= {1, 2, 3, 4, 8, 9}                                                # bin groups: split and beyond 512 bins
