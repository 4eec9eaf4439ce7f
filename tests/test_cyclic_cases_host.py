"""The host model of cyclic folding's launch arithmetic (tests/cyclic_cases.py) and the case table tests/test_gpu_cyclic.py
builds from it: every edge of the partition into tiles, time segments and partial arrays must be reached by a NAMED case, and
every case must be exact (any order of summation gives the same float32 bits).  Runs without a GPU."""
import numpy as np
import pytest

import cyclic_cases as cc
import cyclic_reference as cr


def _parts(name):
    c = cc.by_name(name)
    return [cc.partition(c["nchan"], c["npol_out"], c["nlag"], c["nbin"], call[0]) for call in c["calls"]]


def _set_by(name):
    c = cc.by_name(name)
    return cc.nparts_set_by(c["nchan"], c["npol_out"], c["nlag"], c["nbin"])


def test_constants_come_from_the_source():
    text = open(cc.SOURCE).read()
    assert "constexpr int CY_T = %d;" % cc.CY_T in text and "constexpr int CY_HL = %d;" % cc.CY_HL in text
    assert cc.CY_PART_BYTES == 2 << 30 and cc.CY_MAX_NLAG == 1 << 16          # the suffixed forms (2ull << 30, 1u << 16) parse
    assert "nchan > %d" % cc.MAX_NCHAN in text


def test_model_restates_known_launches():
    # the probe's production shape, -F 64:D -cyclic 256 on 2^18 samples: 8 parts, 512 tiles, 64 per segment
    assert cc.partition(64, 4, 129, 256, 1 << 18) == (8, 512, 8, 64, 0)
    # the cases of tests/cyclic_reference.py always have more parts than tiles: never a segment with a second tile
    for c in cr.EXACT_CASES:
        for call in c["calls"]:
            p = cc.partition(c["nchan"], c["npol_out"], c["nlag"], c["nbin"], call[0])
            assert p.nparts >= 31 > p.ntile and p.ntile <= 5 and p.tps <= 1 and p.nseg == p.ntile and p.empty_segments == 0
    # a short block launches nothing
    assert cc.partition(2, 2, 33, 8, 33)[1:] == (0, 0, 0, 0)
    assert cc.partition(2, 2, 33, 8, 34)[1:] == (1, 1, 1, 0)


def test_every_edge_has_its_case():
    first, second = _parts("multi-tile")
    assert first == (4, 3, 3, 1, 0) and second == (4, 10, 4, 3, 0) and cc.segment_tiles(second) == [3, 3, 3, 1]
    assert _set_by("multi-tile") == "owners"
    c = cc.by_name("multi-tile")
    assert 1.0 / (c["calls"][1][3] * c["nbin"]) > 2 * cc.CY_T, "runs longer than two tiles: open across tile AND segment boundaries"
    assert second.tps >= 3 and second.nseg >= 3

    (p,) = _parts("empty-segment")
    assert p == (4, 5, 4, 2, 1) and cc.segment_tiles(p) == [2, 2, 1, 0]

    (p,) = _parts("three-parts")
    assert p == (3, 7, 3, 3, 0) and _set_by("three-parts") == "owners" and 1 < p.nparts < cc.CY_MAX_PARTS
    assert cc.by_name("three-parts")["nlag"] == 2 * cc.CY_HL + 2              # lags 128 and 129: one lane of each wave

    first, second = _parts("one-part")
    assert first == (1, 4, 1, 4, 0) and second == (1, 2, 1, 2, 0)
    c = cc.by_name("one-part")
    assert c["calls"][0][3] * c["nbin"] > 2, "several bins per sample: every run is one step long"
    p0, p1, _ = cc.call_plans(c, 0)
    assert (np.diff(p0) != 0).all() and (np.diff(p1) != 0).all() and (p0 != p1).any()

    for name, nlag in (("nlag128", 2 * cc.CY_HL), ("nlag256", 4 * cc.CY_HL)):
        (p,) = _parts(name)
        assert cc.by_name(name)["nlag"] == nlag and _set_by(name) == "max"
        assert p.nparts == cc.CY_MAX_PARTS > p.ntile == 4 and p.tps == 1     # tps is 1 by construction: these are about the lanes

    (p,) = _parts("max-nlag")
    assert cc.by_name("max-nlag")["nlag"] == cc.CY_MAX_NLAG and p == (2, 67, 2, 34, 0) and p.ntile > p.nparts
    (p,) = _parts("max-nchan")
    assert cc.by_name("max-nchan")["nchan"] == cc.MAX_NCHAN and p == (1, 2, 1, 2, 0)

    (p,) = _parts("part-cap")
    c = cc.by_name("part-cap")
    wanted, allowed = cc.nparts_limits(c["nchan"], c["npol_out"], c["nlag"], c["nbin"])
    assert _set_by("part-cap") == "bytes" and wanted > cc.CY_MAX_PARTS > allowed == p.nparts == 31
    assert p == (31, 41, 31, 2, 10) and cc.segment_tiles(p) == [2] * 20 + [1] + [0] * 10
    assert (p.nparts + 1) * cc.lag_array_bytes(c["nchan"], c["npol_out"], c["nlag"], c["nbin"]) > cc.CY_PART_BYTES

    assert all(p == (4, 10, 4, 3, 0) for p in _parts("placed-four-parts")) and _set_by("placed-four-parts") == "owners"
    assert all(p == (1, 10, 1, 10, 0) for p in _parts("placed-one-part"))

    # and as the classes the table is there for
    every = [p for name in cc.NAMES for p in _parts(name)]
    assert any(p.tps >= 3 and p.nseg >= 3 for p in every)
    assert any(p.empty_segments and cc.segment_tiles(p)[-1] == 0 for p in every)
    assert any(p.nparts == 1 and p.tps > 1 for p in every)
    assert {c["nlag"] for c in cc.CASES} >= {3, 33, 128, 130, 256, cc.CY_MAX_NLAG}
    assert {(c["npol_in"], c["npol_out"]) for c in cc.CASES} == {(1, 1), (2, 1), (2, 2), (2, 4)}


def _flips_in_one_tile(plan):
    """the longest stretch a, b, a, b, ... of one-step runs that lies within one tile"""
    ch = cc.change_points(plan)
    best = n = 0
    for u, v in zip(ch, ch[1:]):
        ok = v == u + 1 and u // cc.CY_T == v // cc.CY_T and u >= 2 and plan[v] == plan[u - 1]
        n = n + 1 if ok else 0
        best = max(best, n)
    return best


def test_placed_plans_hit_every_boundary_on_both_parities():
    nu, ndat, T = cc.PLACED_NU, cc.PLACED_NDAT, cc.CY_T
    assert nu == cc.steps(cc.PLACED_NLAG, ndat) and (cc.PLACED_SEG1, cc.PLACED_SEG2) == (1536, 3072)
    calls = cc.placed_plans()
    for name in ("placed-four-parts", "placed-one-part"):
        c = cc.by_name(name)
        assert (c["nlag"], c["nbin"]) == (cc.PLACED_NLAG, cc.PLACED_NBIN) and all(call[0] == ndat for call in c["calls"])
        assert len(c["placed"]) == len(calls)
        assert all(np.array_equal(a, b) for pair, mine in zip(c["placed"], calls) for a, b in zip(pair, mine))
    for par in (0, 1):
        plans = [pair[par] for pair in calls]
        assert all(len(pl) == ndat and 0 <= pl.min() and pl.max() < cc.PLACED_NBIN for pl in plans)
        assert any(not cc.change_points(pl) for pl in plans), "one single run over the whole block"
        edged = [pl for pl in plans if cc.change_points(pl)]
        for pl in edged:
            ch = set(cc.change_points(pl))
            assert {T - 1, T, T + 1} <= ch                                       # around the first tile boundary
            assert {3 * T - 1, 3 * T, 3 * T + 1} <= ch                           # the first step of segment 1 and either side
            assert 6 * T in ch and not any(3 * T + 1 < u < 6 * T for u in ch)    # one run that ends exactly with segment 1
            assert 9 * T in ch                                                   # a run begins with the last segment
            assert nu - 1 in ch                                                  # the last step that holds a product
            assert len([u for u in ch if nu <= u < ndat]) >= 3 and ndat - 1 in ch
            assert _flips_in_one_tile(pl) >= 300
            # a bin seen in one segment comes back in another, other bins between
            seg = lambda u: u // (3 * T)
            runs = [0] + sorted(ch)
            seen = {}
            for u in (u for u in runs if u < nu):
                seen.setdefault(int(pl[u]), set()).add(seg(u))
            assert sum(len(s) > 1 for s in seen.values()) >= 3
            assert (np.diff(pl[sorted(ch)]) < 0).any() and (np.diff(pl[sorted(ch)]) > 0).any()
    # set_bin(ibin = b, bins_per_sample = 2 k) must be able to state every pair: plan1 = (b + k) % nbin
    for p0, p1 in calls:
        k = (p1 - p0) % cc.PLACED_NBIN
        assert np.array_equal((p0.astype(np.float64) + 0.5 * (2.0 * k)).astype(np.uint32) % cc.PLACED_NBIN, p1)


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_is_exact_whatever_the_order(name):
    """check_exact bounds the sums; the float32 strict-order restatement and the float64 one then agree in every bit after
    every call, so the reference does not depend on the order where the device's order differs (tiles, segments, combine)"""
    case = cc.by_name(name)
    cr.check_exact(case)
    f32, f64 = cc.reference(name), cc.reference(name, np.float64)
    assert len(f32) == len(f64) == len(case["calls"])
    for k, ((hits, a), (_, b)) in enumerate(zip(f32, f64)):
        assert a.dtype == np.complex64 and b.dtype == np.complex128
        assert np.array_equal(a.view(np.uint32), b.astype(np.complex64).view(np.uint32)), "call %d" % k
        assert a.any() and hits.sum() == case["calls"][k][0]
    if len(f32) > 1:
        assert not np.array_equal(f32[0][1], f32[-1][1])


SMALL = [dict(npol_in=2, npol_out=4, nlag=6, nbin=5, nchan=3, ndat=300, pps=2.3 / 5),
         dict(npol_in=2, npol_out=1, nlag=33, nbin=8, nchan=2, ndat=700, pps=1.0 / 8 / 40.0),
         dict(npol_in=1, npol_out=1, nlag=130, nbin=4, nchan=1, ndat=400, pps=1.0 / 4 / 7.0),
         dict(npol_in=2, npol_out=2, nlag=2, nbin=3, nchan=4, ndat=50, pps=0.01)]


@pytest.mark.parametrize("c", SMALL, ids=["nlag%d" % c["nlag"] for c in SMALL])
def test_fold_keeps_the_association_of_the_sample_loop(c):
    """cr.fold walks u = idat + ilag / 2 on slices; cr.fold_by_sample is the CPU engine's loop as written.  On noise, where every
    other association of the float32 sums shows, and added to earlier sums: the same bits in both precisions."""
    rows = cr.noise_rows(11 + c["nlag"], c["nchan"], c["npol_in"], c["ndat"], 30.0)
    p0, p1, _ = cr.plans(0.37, c["pps"], c["nbin"], c["ndat"])
    for dtype, bits in ((np.float32, np.uint32), (np.float64, np.uint64)):
        a = b = None
        for piece in range(2):
            a = cr.fold(rows, p0, p1, c["nlag"], c["npol_out"], c["nbin"], a, dtype)
            b = cr.fold_by_sample(rows, p0, p1, c["nlag"], c["npol_out"], c["nbin"], b, dtype)
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(bits), b.view(bits)), (dtype, piece)
