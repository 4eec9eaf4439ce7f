"""The table of tests/fold_state_cases.py, checked without a GPU: every case of the square-law fold (dspsr -d 1, -d 2) reaches the
branch its name says on the record computed from the restated host code (256 compute units), where the Coherence case it is
derived from reaches the same kernel branch (tests/test_fused_fold_cases_host.py proves those), and the model sees the faults the
GPU test is there to find."""
import numpy as np
import pytest

import fold_state_cases as sc
import fused_fold_cases as fc
from fold_reference import fold_time_order, fused_fold_model

NCU = 256


def test_the_table_covers_the_groups_with_both_profiles():
    for group in sc.GROUPS:
        profs = {sc.by_name(n)["prof"] for n in sc.of_group(group)}
        assert profs == {"1", "2x1"}, group
    assert not [c for c in sc.CASES if c["group"] == "segsum"]
    # every three-pass base case of the groups is there with both shapes
    for c in fc.CASES:
        if c["group"] in ("psl", "seg", "cap", "runs", "grid") and fc.record(c["name"], NCU)["passes"] == 3:
            bases = {(s["C"], s["M"], repr(s["calls"]), s["max_parts"], s["input_nchan"], s["four"], s["prof"]) for s in sc.CASES}
            for prof in ("1", "2x1"):
                assert (c["C"], c["M"], repr(c["calls"]), c["max_parts"], c["input_nchan"], c["four"], prof) in bases, c["name"]


@pytest.mark.parametrize("name", sc.NAMES)
def test_records_do_not_depend_on_wg3(name):
    assert sc.record(name, NCU, 1) == sc.record(name, NCU, 2) == sc.record(name, NCU)


@pytest.mark.parametrize("name", sc.NAMES)
def test_fused_calls_launch_what_the_coherence_case_launches(name):
    """the launches of a fused call (parts, runs) do not depend on the state: where the base case fuses, the same ns and nseg; a
    three-pass call with a run below FOLD_FUSED_MAX_RUN always fuses here; a two-pass call never"""
    c, rec = sc.by_name(name), sc.record(name, NCU)
    base = fc.record(c["base"], NCU)
    assert rec["mode"] == (base["mode"] if base["mode"] in (1, 2) else 0) and rec["passes"] == base["passes"]
    for call, bcall in zip(rec["calls"], base["calls"]):
        if rec["passes"] == 2:
            assert call["path"] == "detect+fold" and bcall["path"] == "fused"
            continue
        assert (call["path"] == "fused") == (rec["mode"] in (1, 2) and call["max_run"] < fc.FOLD_FUSED_MAX_RUN)
        if call["path"] == "fused" and bcall["path"] == "fused" and c["group"] != "placement":
            assert [(l["ns"], l["nseg"]) for l in call["launches"]] == [(l["ns"], l["nseg"]) for l in bcall["launches"]]


def test_cases_reach_the_branch_their_name_says():
    r = lambda n: sc.record(n, NCU)
    # psl: one exact launch of 127 / 128 / 130 parts, and two of 129
    for prof in ("1", "2x1"):
        for n in (127, 128, 130):
            (call,) = r("psl-%d-%s" % (n, prof))["calls"]
            assert call["path"] == "fused" and call["launches"] == [dict(ns=n, nseg=1)]
        assert [l["ns"] for l in r("psl-2x129-%s" % prof)["calls"][0]["launches"]] == [129, 129]
    # the two-pass twin is not built: Detection + Fold, time order (runs of two samples), although the object reports mode 1
    for name in [n for n in sc.NAMES if n.endswith("2pass-1") or n.endswith("2pass-2x1")]:
        assert r(name)["mode"] == 1 and all(c["path"] == "detect+fold" and c["assoc"] == "time" for c in r(name)["calls"])
    assert {sc.by_name(n)["prof"] for n in sc.NAMES if "2pass" in n} == {"1", "2x1"}
    # seg: mode 2, up to 16 runs, ragged, fewer parts than runs
    sizes = set()
    for name in sc.of_group("seg"):
        rec = r(name)
        assert rec["mode"] == 2
        for call in rec["calls"]:
            for l in call["launches"]:
                assert l["nseg"] == min(l["ns"], 16)
                sizes.add(l["ns"])
    assert {1, 2, 5, 11, 16, 17, 24, 37} <= sizes
    assert {(r(n)["passes"], sc.by_name(n)["prof"]) for n in sc.of_group("seg")} >= {(3, "1"), (3, "2x1"), (2, "1"), (2, "2x1")}
    assert {sc.by_name(n)["input_nchan"] for n in sc.of_group("seg") if r(n)["passes"] == 3} == {1, 3}
    # runs: the longest fused run and the first that is not
    for prof in ("1", "2x1"):
        a, b = r("runs-639-%s" % prof)["calls"][1], r("runs-640-%s" % prof)["calls"][1]
        assert (a["max_run"], a["path"]) == (fc.FOLD_FUSED_MAX_RUN - 1, "fused")
        assert (b["max_run"], b["path"], b["assoc"]) == (fc.FOLD_FUSED_MAX_RUN, "detect+fold", "long")
    # cap and grid: exact launches, as their Coherence twins
    assert all(r(n)["mode"] == 1 and r(n)["calls"][0]["path"] == "fused" for n in sc.of_group("cap") + sc.of_group("grid"))
    assert {r(n)["tiles"] for n in sc.of_group("grid")} == {12, 16}


def test_every_placement_fuses():
    """scalar accumulators: no float4 condition -- rows at a multiple of 4 floats, even, odd, one and three floats off"""
    kinds = set()
    for name in sc.of_group("placement"):
        c = sc.by_name(name)
        off, pad = c["bound"]
        span = c["nbin"] + pad
        kinds.add((off % 4, span % 4))
        assert [call["path"] for call in sc.record(name, NCU)["calls"]] == ["fused", "fused"], name
    assert {(0, 0), (0, 2), (0, 1), (1, 0), (3, 3)} == kinds


def test_model_is_the_coherence_model_row_by_row():
    """fused_fold_model_sq on rows (a, b) gives, per row, what fused_fold_model gives for the float4 (a, b, ., .): the same order"""
    name = "seg-3pass-real-a-2x1"
    c, rec = sc.by_name(name), sc.record(name, NCU)
    nkeep = c["M"] - sum(c["nfilt"])
    prof2 = np.zeros((3, 2, c["nbin"], 1), np.float32)
    prof4 = np.zeros((3, 1, c["nbin"], 4), np.float32)
    exact = prof2
    for k, call in enumerate(rec["calls"]):
        runs, _h, ndat = sc.call_runs(name, k)
        det4 = (np.random.default_rng(5 + k).standard_normal((3, ndat, 4)) * 100).astype(np.float32)
        det2 = np.ascontiguousarray(det4[:, :, :2].transpose(0, 2, 1))
        ls = [l["ns"] for l in call["launches"]]
        nseg = {l["ns"]: l["nseg"] for l in call["launches"]}
        prof2 = sc.fused_fold_model_sq(det2, runs, prof2, nkeep, ls, 2, nseg.__getitem__)
        prof4 = fused_fold_model(det4, runs, prof4, nkeep, ls, 2, nseg.__getitem__)
        exact = sc.fused_fold_model_sq(det2, runs, exact, nkeep, ls, 1)
        assert np.array_equal(exact[:, :, :, 0], fold_time_order(det2[..., None], runs, np.zeros((3, 2, c["nbin"], 1), np.float32))[..., 0]) or k
    assert np.array_equal(prof2[:, 0, :, 0], prof4[:, 0, :, 0]) and np.array_equal(prof2[:, 1, :, 0], prof4[:, 0, :, 1])
    assert not np.array_equal(prof2, exact) and np.abs(prof2 - exact).max() <= 1e-5 * np.abs(exact).max()
