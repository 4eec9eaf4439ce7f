"""The spectral-kurtosis case tables (tests/sk_cases.py) on the restatement alone (tests/sk_reference.py): every case is exact in
float32 in any order of addition, and reaches the edges it names.  No device."""
import numpy as np
import pytest

import sk_reference as ref
from sk_cases import (EDGES, IDS, NOISE, WANT_M, WANT_NCHAN, WANT_NPART, case, chain_length, detector, exact_bound, exact_rows,
                      limits_of, staged)


def _run(name, **over):
    c = case(name)
    c.update(over)
    rows = exact_rows(c)
    est, est_tscr = ref.compute(rows, c["M"], c["flags"][1])
    limits, limits_tscr = limits_of(c)
    det, masks = staged(c, est, est_tscr, limits, limits_tscr)
    return c, rows, est, est_tscr, limits, limits_tscr, det, masks


def test_the_tables_cover_what_the_issue_lists():
    cs = [case(n) for n in IDS]
    assert {c["M"] for c in cs} == WANT_M and {c["nchan"] for c in cs} == WANT_NCHAN and {c["npart"] for c in cs} == WANT_NPART
    assert {c["npol"] for c in cs} == {1, 2} and {c["offset"] for c in cs} == {0, 2} and any(c["pad"] for c in cs)
    assert {0, 1} <= {c["rem"] for c in cs} and any(c["rem"] == c["M"] - 1 for c in cs)
    assert set().union(*(c["expect"] for c in cs)) == EDGES
    assert {c["flags"] for c in cs} >= {(False, False, False), (True, False, False), (False, True, False), (False, False, True)}
    assert {m for m, *_ in NOISE} >= {32, 33, 128, 1000, 1024, 65536}
    # L(M) of the kernel's header comment
    assert [chain_length(m) for m in (32, 128, 1024, 65536)] == [7, 7, 11, 263]


@pytest.mark.parametrize("name", IDS)
def test_case_is_exact_and_reaches_its_edges(name):
    c, rows, est, est_tscr, limits, limits_tscr, det, masks = _run(name)
    M, nchan, npart = c["M"], c["nchan"], c["npart"]
    assert rows.shape == (nchan, c["npol"], 2 * c["ndat"]) and exact_bound(c, rows)
    # exact: the float64 sums are the same numbers
    s1, s2 = ref.sums(rows, M)
    d1, d2 = ref.sums(rows, M, np.float64)
    assert np.array_equal(s1, d1) and np.array_equal(s2, d2) and d2.sum(axis=0).max() <= 2 ** 24
    # the one-call form is the staged form
    one = detector(c)
    assert np.array_equal(one.detect(est, est_tscr, limits, limits_tscr), masks["fscr"]) and ref.same_statistics(one.statistics(), det.statistics())
    cs, ce = det.chan_start, det.chan_end
    lo, hi = limits
    bad = ((est > hi) | (est < lo)).any(axis=2)                # what skfb zaps
    stats = det.statistics()
    assert stats["npart_total"] == npart * nchan and stats["unfiltered_hits"] == npart
    assert stats["zap_counts"][ref.ZAP_ALL] == masks["fscr"][:, cs:ce].sum()
    assert np.array_equal(stats["filtered_hits"][cs:ce], npart - masks["fscr"][:, cs:ce].sum(axis=0))
    for edge in c["expect"]:
        if edge == "tscr":
            for chan in c["tscr"]:
                clean = [p for p in range(npart) if p not in c["fscr"]]
                assert masks["tscr"][:, chan].all() and not bad[clean, chan].any(), "the channel fails as a whole, not part by part"
            assert stats["zap_counts"][ref.ZAP_TSCR] == masks["tscr"].sum() >= npart * len(c["tscr"])
        elif edge in ("skfb_first", "skfb_last"):
            chan = 0 if edge == "skfb_first" else nchan - 1
            hit = [(p, ch) for p, ch in c["const"] + c["zero"] if ch == chan]
            assert hit and all(bad[p, ch] and masks["skfb"][p, ch] == 1 for p, ch in hit)
        elif edge == "skfb_borders":
            assert cs > 0 and ce < nchan
            for chan in (cs, cs + 1, ce - 1, ce):
                assert bad[:, chan].any()
            inside = np.zeros(nchan, bool)
            inside[cs + 1:ce] = True                           # strictly between the borders
            assert stats["zap_counts"][ref.ZAP_SKFB] == bad[:, inside].sum() < bad.sum() - bad[:, cs].sum()
        elif edge == "fscr_after_zaps":
            parts = [p for p in range(npart) if masks["fscr"][p].all() and not masks["skfb"][p].all() and masks["skfb"][p, cs:ce].any()]
            assert parts, "no part fails fscr with fewer channels in its mean than the range holds"
        elif edge == "fscr_only":
            for p in c["fscr"]:
                assert masks["fscr"][p].all() and not masks["skfb"][p].all()
            assert stats["zap_counts"][ref.ZAP_FSCR] >= nchan * len(c["fscr"])
        elif edge == "s1_zero":
            for p, ch in c["zero"]:
                assert not s1[p, ch].any() and not est[p, ch].any() and masks["skfb"][p, ch] == 1
        elif edge == "no_fscr":
            assert stats["zap_counts"][ref.ZAP_FSCR] == 0 and np.array_equal(masks["fscr"], masks["skfb"])
            with_it = _run(name, flags=(False, False, False))[-1]
            assert all(with_it["fscr"][p].all() for p in c["fscr"]) and c["fscr"]
        elif edge == "no_tscr":
            assert est_tscr is None and stats["zap_counts"][ref.ZAP_TSCR] == 0 and not masks["tscr"].any()
            with_it = _run(name, flags=(False, False, False))[-1]
            assert all(with_it["tscr"][:, ch].all() for ch in c["tscr"]) and c["tscr"]
        elif edge == "no_ft":
            assert stats["zap_counts"][ref.ZAP_SKFB] == 0 and np.array_equal(masks["skfb"], masks["tscr"]) and bad.any()
        else:
            raise AssertionError(edge)


def test_an_estimate_equal_to_a_limit_is_not_zapped():
    """V > upper || V < lower: with lower = 0 (the estimate of a constant part and of an empty one) and upper = the largest estimate
    nothing is zapped; one unit in the last place inside, both are."""
    c, rows, est, est_tscr, _, _, _, _ = _run("m128_c64_p2_n64")
    lo, hi = np.float32(0), est.max()
    assert (est == lo).any() and (est == hi).sum() == 1 and est.min() == 0
    det = detector(c)
    det.reset_mask(c["npart"])
    det.detect_skfb(est, lo, hi)
    assert not det.mask.any() and det.zap_counts[ref.ZAP_SKFB] == 0
    det.detect_skfb(est, np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0)))
    assert det.mask.sum() == len({(p, ch) for p, ch, _ in zip(*np.nonzero((est == lo) | (est == hi)))})


def test_mask_rows_zeroes_whole_parts_of_both_polarisations():
    c, rows, est, est_tscr, limits, limits_tscr, det, masks = _run("m128_c64_p2_n7_range")
    out = ref.mask_rows(rows, masks["fscr"], c["M"])
    assert out.shape[2] == 2 * c["npart"] * c["M"] < rows.shape[2]
    view = out.reshape(c["nchan"], c["npol"], c["npart"], 2 * c["M"])
    src = rows[:, :, :out.shape[2]].reshape(view.shape)
    for p in range(c["npart"]):
        for ch in range(c["nchan"]):
            assert np.array_equal(view[ch, :, p], 0 * src[ch, :, p] if masks["fscr"][p, ch] else src[ch, :, p])
    assert masks["fscr"].any() and not masks["fscr"].all()
