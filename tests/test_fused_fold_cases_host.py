"""The table of tests/fused_fold_cases.py and the model of tests/fold_reference.py (fused_fold_model), checked without a GPU:
every branch of the fused fold that tests/test_gpu_fused_fold.py is there for must be reached by a NAMED case, on the record
computed from the restated host code for a device of 256 compute units; and the model must be able to see the faults the GPU
tests are there to find.

Which records depend on wg3 (workgroups per compute unit of the three-pass inverse kernel, 1 or 2 by its LDS): none --
test_records_do_not_depend_on_wg3 computes every record with both values.  The segmented cases have 8 or 16 tiles, so that
wgs / tiles >= 16 already with one workgroup per compute unit, and the exact cases launch min(tiles, wgs) workgroups."""
import numpy as np
import pytest

import fused_fold_cases as fc
from fold_reference import clip_runs, fold_time_order, fused_fold_model, fused_launch_sums, fused_nseg, fused_runs_of_launch

NCU = 256


def _launches(name):
    return [l for call in fc.record(name, NCU)["calls"] for l in call["launches"]]


def test_constants_come_from_the_sources():
    assert (fc.FB_PSL_MAX, fc.FOLD_FUSED_MAX_RUN, fc.LOG_POINTS, fc.MAX_LOGF, fc.PTS) == (128, 640, 14, 13, 32)


def test_geometry_restates_known_shapes():
    # the shapes whose tiles the library's comments and tests name: cfg4 32 tiles of 16 channels, cfg2 128 tiles of 2
    g = fc.geometry(512, 512, (27, 27), False, force_four_pass=2)
    assert (g["passes"], g["tiles"], g["T3"]) == (3, 32, 16)
    g = fc.geometry(512, 512, (27, 27), False)
    assert (g["passes"], g["tiles"], g["T3"], g["blockdim"]) == (2, 32, 16, 512)
    g = fc.geometry(256, 4096, (953, 956), True)
    assert (g["passes"], g["tiles"], g["T3"]) == (3, 128, 2)
    assert fc.geometry(4, 16384, (301, 212), True)["passes"] == 4 and fc.geometry(4, 16384, (301, 212), True)["logTt"] == 5
    assert fc.fold_mode(fc.geometry(256, 4096, (953, 956), True), fc.FUSED_AUTO, NCU) == 2
    assert fc.fold_mode(fc.geometry(16, 256, (20, 21), True), fc.FUSED_AUTO, NCU) == 0
    assert [fc.grid_for(t, 256) for t in (1, 7, 8, 12, 16, 300)] == [1, 7, 8, 8, 16, 256]


@pytest.mark.parametrize("name", fc.NAMES)
def test_records_do_not_depend_on_wg3(name):
    strip = lambda r: {k: v for k, v in r.items() if k != "wgs"}          # (wgs itself is ncu * wg3)
    assert strip(fc.record(name, NCU, 1)) == strip(fc.record(name, NCU, 2)) == strip(fc.record(name, NCU))


@pytest.mark.parametrize("name", fc.of_group("psl"))
def test_psl_cases_reach_their_side_of_the_offset_table(name):
    rec = fc.record(name, NCU)
    if name.startswith("psl-2x129"):            # the second launch starts at part 129 of the call: pstart[part0 + lp] with part0 > 0
        assert [(l["ns"], l["use_psl"]) for l in _launches(name)] == [(129, [False]), (129, [False])] and rec["mode"] == 1
        assert rec["passes"] == (2 if name.endswith("2pass") else 3) and not any(x for l in _launches(name) for x in l["in_lds"])
        return
    (l,) = _launches(name)
    n = int(name.split("-")[1])
    assert rec["mode"] == 1 and l["ns"] == n and l["nseg"] == 1 and l["psl"] == [n + 1]
    assert l["use_psl"] == [n + 1 <= fc.FB_PSL_MAX] and (n + 1 <= fc.FB_PSL_MAX) == (n == 127)
    assert rec["passes"] == (2 if name.endswith("2pass") else 3)
    assert rec["tiles"] == (2 if n == 130 else 1) and min(l["items_per_thread"]) >= 2          # second work items in every part
    # the entries of every part would fit the LDS buffer: it is the offsets alone that decide where they come from
    assert 0 < min(l["nact"]) and max(l["nact"]) <= rec["plan_cap"]
    assert l["in_lds"] == l["use_psl"] * n
    # a second work item while the prefetched accumulator exists (w != tid with `pre`): every part of psl-127, no part of the others
    assert l["second_item_with_pre"] == (list(range(n)) if n == 127 else [])


def test_a_second_work_item_meets_a_prefetched_accumulator():
    """`pre && w != tid`: a part whose offsets and entries sit in LDS (use_psl, in_lds) and whose bins give a thread two items
    -- psl-127 (T3 = 32: some 38 bins x 32 channels on 512 threads; two passes: 276 bins x 16 channels, more items than the
    two prefetched ones of k_rows_inv).  The segmented cases keep their parts below one item per
    thread, and the cap cases reach w != tid only with entries from global memory (T3 = 1: 513 bins are more than plan_cap)"""
    reached = set()
    for name in fc.of_group("psl") + fc.of_group("seg"):
        rec = fc.record(name, NCU)
        for l in _launches(name):
            for p in l["second_item_with_pre"]:
                assert l["in_lds"][p] and l["items_per_thread"][p] >= 2 and l["nact"][p] <= rec["plan_cap"]
                reached.add(name)
    assert reached == {"psl-127-4", "psl-127-2x2", "psl-127-2pass"}
    assert min(fc.record("psl-127-2pass", NCU)["calls"][0]["launches"][0]["items_per_thread"]) >= 3
    assert not any(l["second_item_with_pre"] for name in fc.of_group("cap") for l in _launches(name))
    # (the fused placement cases fold the psl geometry two parts per launch: every part of theirs reaches it as well)
    for name in ("place-4-span4", "place-2x2-span4", "place-2x2-even"):
        assert all(l["second_item_with_pre"] == list(range(l["ns"])) for l in _launches(name))


def test_segmented_cases_reach_every_run_shape():
    sizes, shapes, empty, profs, paths, nchans = set(), set(), set(), set(), set(), set()
    for name in fc.of_group("seg"):
        c, rec = fc.by_name(name), fc.record(name, NCU)
        assert rec["mode"] == 2 and 8 <= rec["tiles"] <= 16 and rec["wgs"] // rec["tiles"] >= 16
        assert len(c["calls"]) >= 2, "run 0 must continue a profile that already holds sums"
        for l in _launches(name):
            assert l["nseg"] == min(l["ns"], 16) == fused_nseg(l["ns"], rec["tiles"], rec["wgs"]) and l["grid"] == rec["tiles"] * max(l["nseg"], 1)
            assert all(l["use_psl"]) and sum(l["run_parts"]) == l["ns"]
            sizes.add(l["ns"])
            shapes.add((l["ns"], tuple(l["empty_runs"]), l["run_parts"][l["nseg"] - len(l["empty_runs"]) - 1]))
            empty.update(l["empty_runs"])
        profs.add((rec["passes"], c["prof"]))
        paths.add((rec["passes"], c["real"]))
        nchans.add((rec["passes"], c["input_nchan"]))
    assert {1, 2, 11, 16, 17, 24, 37, 5} <= sizes
    assert (24, (12, 13, 14, 15), 2) in shapes and (37, (13, 14, 15), 1) in shapes          # 37: a last run of ONE part
    assert (17, tuple(range(9, 16)), 1) in shapes
    assert profs == {(3, "4"), (3, "2x2"), (2, "4"), (2, "2x2")}
    assert paths == {(3, True), (3, False), (2, False)} and {(2, 3), (3, 3), (2, 1), (3, 1)} <= nchans
    # an empty part as the first part of a run, and one inside a run
    (l,) = fc.record("seg-empty-part", NCU)["calls"][1]["launches"]
    assert l["empty_parts"] == [2, 7] and 2 in l["run_first_parts"] and 7 not in l["run_first_parts"]


def test_cap_cases_straddle_plan_cap_and_the_workgroup():
    for name in fc.of_group("cap"):
        rec = fc.record(name, NCU)
        cap, nt = rec["plan_cap"], rec["blockdim"]
        assert rec["mode"] == 1 and rec["T3"] == 1 and 16 <= cap < nt == 512
        nact = [a for l in _launches(name) for a in l["nact"]]
        in_lds = [a for l in _launches(name) for a in l["in_lds"]]
        assert nact == [cap - 1, cap, cap + 1, nt + 1, 3, cap]
        assert in_lds == [True, True, False, False, True, True]
        assert [i for l in _launches(name) for i in l["items_per_thread"]] == [1, 1, 1, 2, 1, 1]      # 513 items on 512 threads
        assert max(n for l in _launches(name) for n in l["nint"]) > 3


def test_runs_cases_reach_the_sample_loop_and_the_dispatcher():
    l = fc.record("runs-hits", NCU)["calls"][0]["launches"][0]
    assert {1, 7, 8, 9, 16, 17} <= set(l["first_hits"]) and {1, 2, 3} <= set(l["nint"])
    assert l["empty_parts"] == [2] and 0 < 2 < l["ns"] - 1 and l["nseg"] == 1
    a, b = fc.record("runs-639", NCU)["calls"][1], fc.record("runs-640", NCU)["calls"][1]
    assert (a["max_run"], a["path"]) == (fc.FOLD_FUSED_MAX_RUN - 1, "fused")
    assert (b["max_run"], b["path"], b["assoc"]) == (fc.FOLD_FUSED_MAX_RUN, "detect+fold", "long")
    assert 639 in a["launches"][0]["first_hits"]


def test_placement_cases_take_the_path_their_name_says():
    want = {"place-4-span4": "fused", "place-4-even": "detect+fold", "place-4-odd": "detect+fold", "place-4-off1": "detect+fold",
            "place-2x2-span4": "fused", "place-2x2-even": "fused", "place-2x2-odd": "detect+fold", "place-2x2-off1": "detect+fold"}
    assert set(want) == set(fc.of_group("placement"))
    for name, path in want.items():
        c = fc.by_name(name)
        span = c["nbin"] * (2 if c["prof"] == "2x2" else 4) + c["bound"][1]
        kind = name.split("-")[-1]
        assert {"span4": span % 4 == 0, "even": span % 4 == 2, "odd": span % 2 == 1, "off1": c["bound"][0] == 1}[kind]
        assert [call["path"] for call in fc.record(name, NCU)["calls"]] == [path, path], name
        assert all(call["assoc"] in (None, "time") for call in fc.record(name, NCU)["calls"])


def test_segment_sum_cases_qualify_as_named():
    recs = {n: fc.record(n, NCU) for n in fc.of_group("segsum")}
    assert all(r["mode"] == 3 and r["seg"] == 32 for r in recs.values())
    a, b, c = (recs["segsum-" + n]["calls"][0] for n in ("exact", "one-short-interval", "one-sample-short"))
    ndat = fc.call_runs("segsum-exact", 0)[2]
    assert (a["path"], a["inner"], a["end"]) == ("segsum", [32], ndat)
    assert (b["path"], b["inner"], b["end"]) == ("detect+fold", [31, 32], ndat)
    assert (c["path"], c["inner"], c["end"]) == ("detect+fold", [32], ndat - 1)
    assert min(x["max_run"] for x in (a, b, c)) >= 64


def test_grid_cases_and_the_tile_permutation():
    a, b = fc.record("grid-12-tiles", NCU), fc.record("grid-16-tiles", NCU)
    assert (a["mode"], a["tiles"], a["grid_exact"]) == (1, 12, 8)       # workgroups 0-3 walk tiles b and b + 8
    assert (b["mode"], b["tiles"], b["grid_exact"]) == (1, 16, 16)
    # fb_tile sets logT3 = logX3 for every three-pass geometry, and the kernel's own logT3 (LOGT - 1 of the full-size
    # instantiation, picked only where logT3 + 1 == LOGT = 14 - logM; g.logT3 otherwise) is the host's: lr = logX3 - logT3 is 0
    # and the permutation of fold_b is the identity on the device today -- no geometry can make it active; every record says so
    assert all(fc.record(n, NCU).get("lr", 0) == 0 for n in fc.NAMES)
    for logC in range(0, 13):
        for logM in range(5, fc.MAX_LOGF + 1):
            for real in (True, False):
                g = fc.geometry(1 << logC, 1 << logM, (1, 1), real)         # (any failure of the restatement fails here)
                if g["passes"] != 4:
                    assert g["kernel_logT3"] == g["logT3"] == g["logX3"], (logC, logM, real)
    # restated, it is a bijection of the tiles for every grid grid_for can produce and every lr, active or not
    for lr in range(4):
        for tiles in range(1, 513):
            grid = fc.grid_for(tiles, 2 * NCU)
            p = fc.fold_b_permutation(grid, lr)
            assert sorted(p.tolist()) == list(range(grid)), (grid, lr)
            if lr and grid % (8 << lr) == 0:
                assert not np.array_equal(p, np.arange(grid)) or grid == 0


@pytest.mark.parametrize("name", fc.NAMES)
def test_part_plan_covers_every_run_sample_once(name):
    c = fc.by_name(name)
    nkeep = c["M"] - sum(c["nfilt"])
    for k, (parts, _plan) in enumerate(c["calls"]):
        runs, hits, ndat = fc.call_runs(name, k)
        want = np.full(ndat, -1, np.int64)
        for off, b, n in runs:
            want[off:off + n] = b
        got = np.full(ndat, -1, np.int64)
        for p, bins in enumerate(fc.part_plan(runs, nkeep, parts, c["nbin"])):
            assert [b for b, _iv in bins] == sorted(b for b, _iv in bins)
            for b, iv in bins:
                assert iv == sorted(iv) and len(iv) < 1 << 16
                for off, n in iv:
                    assert 0 < n <= nkeep - off and (got[p * nkeep + off:p * nkeep + off + n] == -1).all()
                    got[p * nkeep + off:p * nkeep + off + n] = b
        assert np.array_equal(got, want) and np.array_equal(np.bincount(want[want >= 0], minlength=c["nbin"]), hits)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def _data(name, k, nchan=3):
    runs, _hits, ndat = fc.call_runs(name, k)
    rng = np.random.default_rng(5 + k)
    return runs, (rng.standard_normal((nchan, ndat, 4)) * 100).astype(np.float32)


def _wrong_library(det, runs, prof, nkeep, launches, nseg_of, fault):
    """What two WRONG libraries would leave in a [chan][1][nbin][4] profile after a segmented call: "reversed" -- the combine
    adds the run sums last run first; "onto" -- run 1 adds straight onto the profile instead of summing from zero"""
    rows, out, part0 = det[:, None], np.array(prof, np.float32), 0
    for ns in launches:
        nseg = nseg_of(ns)
        out, partial = fused_launch_sums(rows, runs, out, nkeep, part0, ns, nseg)
        if fault == "onto" and partial:
            p0, n = fused_runs_of_launch(ns, nseg)[1]
            out = fold_time_order(rows, clip_runs(runs, (part0 + p0) * nkeep, (part0 + p0 + n) * nkeep), out)
            partial = partial[1:]
        for p in (partial[::-1] if fault == "reversed" else partial):
            out = out + p
        part0 += ns
    return out


@pytest.mark.parametrize("name", ["seg-3pass-real-a", "seg-2pass-b", "seg-empty-part", "runs-hits"])
def test_model_orders(name):
    """mode 1 is fold_time_order; mode 2 with one run is mode 1; with the table's runs it differs from mode 1 in some bits, and a
    reversed run order, or run 1 added straight onto the profile, changes bits again: the GPU tests can see those faults"""
    c, rec = fc.by_name(name), fc.record(name, NCU)
    nkeep = c["M"] - sum(c["nfilt"])
    prof = np.zeros((3, 1, c["nbin"], 4), np.float32)
    exact, seg, rev, onto = prof, prof, prof, prof
    for k, call in enumerate(rec["calls"]):
        runs, det = _data(name, k)
        ls = [l["ns"] for l in call["launches"]]
        nseg = {l["ns"]: l["nseg"] for l in call["launches"]}
        e2 = fused_fold_model(det, runs, exact, nkeep, ls, 1)
        assert np.array_equal(e2, fold_time_order(det[:, None], runs, exact))
        assert np.array_equal(e2, fused_fold_model(det, runs, exact, nkeep, ls, 2, lambda ns: 1))
        exact = e2
        seg = fused_fold_model(det, runs, seg, nkeep, ls, 2, nseg.__getitem__)
        assert np.array_equal(_wrong_library(det, runs, seg, nkeep, ls, nseg.__getitem__, None),
                              fused_fold_model(det, runs, seg, nkeep, ls, 2, nseg.__getitem__))          # the wrapper, without a fault
        rev = _wrong_library(det, runs, rev, nkeep, ls, nseg.__getitem__, "reversed")
        onto = _wrong_library(det, runs, onto, nkeep, ls, nseg.__getitem__, "onto")
    if rec["mode"] == 2:
        assert not np.array_equal(seg, exact) and not np.array_equal(seg, rev) and not np.array_equal(seg, onto)
        assert np.abs(seg - exact).max() <= 1e-5 * np.abs(exact).max()
    else:
        assert np.array_equal(seg, exact)


def test_model_keeps_the_profile_shape():
    runs, det = _data("seg-2pass-b", 0)
    p4 = np.random.default_rng(1).standard_normal((3, 1, 32, 4)).astype(np.float32)
    p22 = p4.reshape(3, 32, 2, 2).transpose(0, 2, 1, 3)
    a = fused_fold_model(det, runs, p4, 48, [24], 2, lambda ns: 16)
    b = fused_fold_model(det, runs, p22, 48, [24], 2, lambda ns: 16)
    assert b.shape == (3, 2, 32, 2) and np.array_equal(b.transpose(0, 2, 1, 3).reshape(3, 1, 32, 4), a)
