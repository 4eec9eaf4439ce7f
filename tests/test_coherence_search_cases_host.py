"""The cases of tests/test_gpu_coherence_search.py, checked without a GPU from the restated arithmetic of
tests/coherence_search_cases.py: every case reaches the edge it is there for -- the fit of the staged tile as the case states it,
the carries a thread holds, a part that reads AND replaces a carry, a call that begins inside a scrunch group, a call cut into
launch groups.  And the restatement itself against the source it restates."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coherence_search_cases as cc                                                  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dspsr_amd", "csrc")


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_the_case_reaches_its_edge(case):
    assert len(case.sfs) == len(case.fused)
    for sf, fused in zip(case.sfs, case.fused):
        assert cc.fits(case.C, case.M, case.nkeep, sf) == fused, (case.name, sf)
        # the condition the issue and the header give for tiles within the carry limit: tscrunch * G <= freq_res
        if case.rpt <= 4:
            assert (sf * cc.groups(case.nkeep, sf) <= case.M) == fused, (case.name, sf)
    assert cc.rows_per_thread(case.C, case.M) == case.rpt
    assert (case.rpt <= cc.carries_per_thread(case.M)) == (case.rpt <= 4)
    if case.nfilt is not None:
        assert case.nkeep == case.M - sum(case.nfilt)
    tsp = cc.parts_of(case.nkeep, case.sfs[0], case.parts)
    reads_and_replaces = any(phi and ng >= 2 and rlast < case.sfs[0] for (_c, _p0, phi, ng, rlast) in tsp)
    begins_inside = any(p0 for (_c, p0, _phi, _ng, _rl) in tsp)
    assert (reads_and_replaces and begins_inside) == case.carry
    assert (max(case.parts) > case.maxp) == case.split


def test_the_cases_the_carry_order_rests_on():
    """a, b, c, e and g each hold a part that reads and replaces a carry; a, b, c and g cut a call into launch groups"""
    for name in "abceg":
        assert cc.BY_NAME[name].carry and cc.BY_NAME[name].fused[0], name
    for name in "abcg":
        assert cc.BY_NAME[name].split, name
    assert [cc.BY_NAME[n].rpt for n in "abcd"] == [1, 2, 4, 8]
    assert cc.BY_NAME["h"].sfs == (1,) and not cc.BY_NAME["d"].fused[0]
    # i: four rows do not fit where two do
    i = cc.BY_NAME["i"]
    assert not cc.fits(i.C, i.M, i.nkeep, 16) and cc.fits(i.C, i.M, i.nkeep, 16, npo=2)
    # f: a tile smaller than 2^14 points; e and l: full-size ones
    assert cc.tile(4, 256)[1] * cc.PTS < 2 ** 14 and cc.tile(16, 2048)[1] * cc.PTS == 2 ** 14 and cc.tile(64, 256)[1] * cc.PTS == 2 ** 14
    assert cc.tile(16, 2048)[0] == 2                                                 # T3 = 4
    # m: more full-size tiles than compute units (one workgroup per unit: some walk two tiles); every other case has fewer
    m = cc.BY_NAME["m"]
    assert m.C >> cc.tile(m.C, m.M)[0] > cc.NCU and cc.tile(m.C, m.M)[1] * cc.PTS == 2 ** 14
    assert all(c.C >> cc.tile(c.C, c.M)[0] <= cc.NCU for c in cc.CASES if c.name != "m")


def test_the_restatement_follows_the_source():
    """the limits restated in coherence_search_cases are the ones the source holds"""
    fb = open(os.path.join(CSRC, "filterbank.hip")).read()
    body = fb[fb.index("static bool fb_search_fits("):]
    body = body[:body.index("\n}\n")]
    assert "((uint64_t)g.nkeep + 2ull * sf - 2) / sf" in body and "(uint32_t)ngmax | 1u" in body
    assert "floats > 2ull * fb->p3s.threads * PTS" in body and "4ull * fb->p3s.threads" in body
    m = re.search(r"npre = g\.logM <= 4 \? 4 : g\.logM == 5 \? 2 : 1;", body)
    assert m, "carries per thread of the Coherence form"
    assert [cc.carries_per_thread(1 << k) for k in (3, 4, 5, 6, 13)] == [4, 4, 2, 1, 1]
    wg = open(os.path.join(CSRC, "wgfft.h")).read()
    assert re.search(r"constexpr int PTS = %d;" % cc.PTS, wg)
    inv = open(os.path.join(CSRC, "fb_inv_chan.h")).read()
    assert "constexpr int FB_EPI_COHERENCE = 16;" in inv
    assert "constexpr int TS_NPRE = FftPlan<LOGF>::NS >= 2 ? (TS_MID2 ? 2 : 1) : 4;" in inv
