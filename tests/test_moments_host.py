"""Fourth-order moments (`dspsr -4`), the parts that need no GPU: the restatement of dsp::FourthMoment, the Archiver's
raw_to_central, the hand-off file, the Config's branch order and refusals, and the case table of tests/test_gpu_fourth_moment.py
against the launch arithmetic restated in tests/moments_cases.py."""
import numpy as np
import pytest

import moments_cases as mc
from fold_reference import runs_of_plan


def test_products_follow_the_reference_loop():
    # FourthMoment.C:67-72: i outer, j from i; the issue's list 00 01 02 03 11 12 13 22 23 33
    assert mc.PAIRS == ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
    from dspsr_amd import pipeline
    assert pipeline.MOMENT_PAIRS == mc.PAIRS
    s = np.array([[3.0, -5.0, 7.0, 11.0]], np.float32)                  # distinct primes: every product names its pair
    out = mc.fourth_moment(s)
    assert out.dtype == np.float32 and out.shape == (1, 14)
    assert out[0].tolist() == [3, -5, 7, 11, 9, -15, 21, 33, 25, -35, -55, 49, 77, 121]
    # one float32 multiply each: not the float64 product rounded twice or left unrounded
    rng = np.random.default_rng(0)
    x = rng.standard_normal((50, 4)).astype(np.float32)
    got = mc.fourth_moment(x)
    assert np.array_equal(got[:, :4].view(np.uint32), x.view(np.uint32))
    for k, (i, j) in enumerate(mc.PAIRS):
        assert np.array_equal(got[:, 4 + k], (x[:, i].astype(np.float64) * x[:, j].astype(np.float64)).astype(np.float32))


def test_kernel_constants_come_from_the_source():
    text = open(mc.SOURCE).read()
    for name in ("MOM_NDIM", "MOM_THREADS", "MOM_MB", "MOM_SEG_UNIT", "MOM_CHUNK_STOKES", "MOM_CHUNK_STREAM", "MOM_FM_SAMPLES"):
        assert "constexpr uint32_t %s = %d;" % (name, getattr(mc, name)) in text, name
    assert "constexpr int MOM_BPT = %d;" % mc.MOM_BPT in text
    assert mc.MOM_MB == mc.FOLD_MB and mc.MOM_SEG_UNIT == mc.FOLD_CHUNK          # what lets fold_long_model state the LONG sums
    assert mc.MOM_SEG_UNIT % mc.MOM_CHUNK_STOKES == 0 and mc.MOM_SEG_UNIT % mc.MOM_CHUNK_STREAM == 0
    assert mc.MOM_CHUNK_STREAM % mc.MOM_MB == 0 and mc.MOM_CHUNK_STOKES % mc.MOM_MB == 0


def test_moments_to_central_against_double():
    from dspsr_amd import pipeline
    rng = np.random.default_rng(5)
    nchan, nbin, scale = 3, 16, 4096.0 * 512.0
    hits = rng.integers(1, 400, nbin).astype(np.uint32)
    hits[3] = 0
    # sums as a fold would leave them: hits samples of Stokes-like values times the scale
    prof = np.zeros((nchan, 1, nbin, 14), np.float64)
    for b in range(nbin):
        s = rng.standard_normal((nchan, int(hits[b]), 4)) * scale * np.array([1.0, 0.3, 0.2, 0.1]) + scale * np.array([2.0, 0.1, 0, 0])
        prof[:, 0, b, :4] = s.sum(axis=1)
        for k, (i, j) in enumerate(mc.PAIRS):
            prof[:, 0, b, 4 + k] = (s[:, :, i] * s[:, :, j]).sum(axis=1)
    prof = prof.astype(np.float32)
    means, central = pipeline.moments_to_central(prof, hits, scale)
    assert means.shape == (nchan, 4, nbin) and central.shape == (nchan, 10, nbin) and means.dtype == central.dtype == np.float32
    ok = hits > 0
    p64 = prof.astype(np.float64)
    h = hits[ok].astype(np.float64)
    m = p64[:, 0, ok, :4] / (scale * h)[None, :, None]                              # Archiver.C:842 with scale
    assert np.abs(means[:, :, ok] - m.transpose(0, 2, 1)).max() <= 2.0 ** -24 * np.abs(m).max()
    for k, (i, j) in enumerate(mc.PAIRS):
        raw = p64[:, 0, ok, 4 + k] / (scale * scale * h)                             # :684 scale squared
        want = (raw - m[:, :, i] * m[:, :, j]) / h                                   # :763
        # float32 amps: one rounding of the moment, one of each mean; one of the result
        tol = 3 * 2.0 ** -24 * (np.abs(raw) + np.abs(m[:, :, i] * m[:, :, j])) / h + 2.0 ** -24 * np.abs(want)
        assert (np.abs(central[:, k, ok] - want) <= tol).all(), k
    assert (central[:, :, ~ok] == 0).all()
    # the variances of the mean are positive and of the size of var / hits
    assert (central[:, 0, ok] > 0).all()
    with pytest.raises(pipeline.DspsrAmdError, match="14"):
        pipeline.moments_to_central(np.zeros((2, 1, 8, 4), np.float32), np.ones(8), 1.0)


def test_hand_off_file_round_trips_a_moments_profile(tmp_path):
    from dspsr_amd import pipeline
    rng = np.random.default_rng(9)
    prof = rng.standard_normal((3, 1, 37, 14)).astype(np.float32)
    hits = rng.integers(0, 99, 37).astype(np.uint32)
    sub = {"hits": hits, "integration_length": 0.125, "ndat_total": int(hits.sum()), "profile": prof}
    cfg = pipeline.Config(nchan=3, nbin=37, folding_period=0.004, fourth_moment=True)
    info = pipeline.InputInfo()
    path = str(tmp_path / "m.ps")
    pipeline.write_phase_series(path, sub, info, cfg, npol=1, scale=7.0, folding_period=0.004)
    hdr, h, p = pipeline.read_phase_series(path)
    assert (hdr["STATE"], int(hdr["NPOL"]), int(hdr["NDIM"]), int(hdr["NCHAN"]), int(hdr["NBIN"])) == ("FourthMoment", 1, 14, 3, 37)
    assert p.shape == (3, 1, 37, 14) and np.array_equal(p.view(np.uint32), prof.view(np.uint32)) and np.array_equal(h, hits)
    # without -4 the same call writes what it always wrote
    cfg4 = pipeline.Config(nchan=3, nbin=37, folding_period=0.004)
    sub4 = dict(sub, profile=prof[..., :4].copy())
    pipeline.write_phase_series(path, sub4, info, cfg4, npol=1)
    hdr, _, p = pipeline.read_phase_series(path)
    assert (hdr["STATE"], int(hdr["NPOL"]), int(hdr["NDIM"])) == ("Coherence", 1, 4) and p.shape == (3, 1, 37, 4)
    # the C++ reader sizes by the header and knows the state
    import os
    text = open(os.path.join(os.path.dirname(mc.SOURCE), "..", "host", "dspsr_amd_phase_series_io.h")).read()
    assert 'state == "FourthMoment" ? Signal::FourthMoment' in text and "f.nchan) * f.npol * f.nbin * f.ndim" in text


def test_branch_order_and_forced_detection():
    from dspsr_amd import pipeline
    base = dict(nchan=16, nbin=64, folding_period=0.004, ndim=2, fused_fold=True)
    on = pipeline.Config(fourth_moment=True, **base)
    assert pipeline.fourth_moment_active(on)
    built = pipeline.fourth_moment_check(on)
    assert (built.stokes, built.ndim, built.fused_fold, built.force_fused) == (True, 4, False, False)      # LoadToFold1.C:1119-1123
    for npol in (1, 3):                                                     # :552: the first branch wins, -4 is not looked at
        c = pipeline.Config(fourth_moment=True, npol=npol, **base)
        assert not pipeline.fourth_moment_active(c)
        assert pipeline.fourth_moment_check(c, ntargets=3, subband=1) is c  # the ordinary chain: nothing forced, nothing refused
    for npol in (2, 4):
        assert pipeline.fourth_moment_active(pipeline.Config(fourth_moment=True, npol=npol, **base))
    off = pipeline.Config(**base)
    assert not pipeline.fourth_moment_active(off) and pipeline.fourth_moment_check(off) is off


def test_refused_combinations_name_the_option():
    from dspsr_amd import pipeline, DspsrAmdError
    info = pipeline.InputInfo(npol=2)
    cfg = pipeline.Config(nchan=16, nbin=64, folding_period=0.004, fourth_moment=True)
    targets = [pipeline.FoldTarget("a", folding_period=0.004, nbin=64), pipeline.FoldTarget("b", folding_period=0.005, nbin=64)]
    with pytest.raises(DspsrAmdError, match=r"fourth_moment \(-4\).*one pulsar"):
        pipeline.LoadToFold(cfg, info, targets=targets)
    with pytest.raises(DspsrAmdError, match=r"fourth_moment \(-4\).*multi-GPU"):
        pipeline.LoadToFold(cfg, info, subband=0)
    import dataclasses
    with pytest.raises(DspsrAmdError, match=r"fourth_moment \(-4\).*cyclic"):
        pipeline.LoadToFold(dataclasses.replace(cfg, cyclic_nchan=32), info)


def _case_runs(case, k, oracle):
    plan, _, _ = mc.case_call_plan(case, k, oracle.fold_binplan)
    return runs_of_plan(plan, case["calls"][k][0])


@pytest.mark.parametrize("case", mc.CASES, ids=[c["name"] for c in mc.CASES])
def test_every_case_reaches_its_edge(oracle, case):
    """geometry() -- fold_moments_run's arithmetic on an MI355X (256 compute units) -- says of every call of the case what its
    `edge` claims; the values are exact in any order; no bin takes more than 2^17 samples."""
    x = mc.case_stokes(case)
    assert x.min() >= -8 and x.max() <= 8 and np.array_equal(x, np.round(x))
    total = np.zeros(case["nbin"], np.int64)
    for k, (i0, n) in enumerate(case["calls"]):
        assert i0 + n <= case["ndat"]
        runs = _case_runs(case, k, oracle)
        assert runs[:, 2].sum() == n and runs[0, 0] == i0
        np.add.at(total, runs[:, 1], runs[:, 2])
        g = mc.geometry(case["nchan"], case["nbin"], runs)
        for key, want in case["edge"].items():
            if key == "nseg_min":
                assert g["nseg"] >= want, (key, g)
            elif key == "first_mod4":
                assert i0 % 4 == want and g["first"] == i0 - want, (key, g)
            else:
                assert g[key] == want, (key, g)
        if g["lng"]:
            assert g["seg_samples"] % mc.MOM_SEG_UNIT == 0 and g["nseg"] * g["seg_samples"] >= g["last"] - g["first"]
            assert (g["nseg"] - 1) * g["seg_samples"] < g["last"] - g["first"], "no empty segment"
        assert g["ngroup"] * mc.MOM_BPT * mc.MOM_THREADS >= case["nbin"]
    assert total.max() <= 1 << 17 and 64 * total.max() < 1 << 24


def test_the_table_covers_what_the_issue_lists(oracle):
    names = {c["name"]: c for c in mc.CASES}
    assert {c["nbin"] for c in mc.CASES} >= {1, 2, 37, 1024, 4097}
    assert {c["nchan"] for c in mc.CASES} >= {1, 300} and 300 > mc.NCU_MI355X
    assert {c["calls"][0][0] % 4 for c in mc.CASES} == {0, 1, 2, 3}
    assert len(names["three-calls"]["calls"]) == 3
    # both variants, and a LONG case whose runs cross the ends of several time segments
    lng = [mc.geometry(c["nchan"], c["nbin"], _case_runs(c, 0, oracle))["lng"] for c in mc.CASES]
    assert any(lng) and not all(lng)
    c = names["nbin1024-long-segments"]
    runs = _case_runs(c, 0, oracle)
    g = mc.geometry(c["nchan"], c["nbin"], runs)
    ends = g["first"] + g["seg_samples"] * np.arange(1, g["nseg"])
    crossed = [(runs[:, 0] < e) & (runs[:, 0] + runs[:, 2] > e) for e in ends]
    assert sum(m.any() for m in crossed) >= 4
    # the straddle: 63 keeps the exact kernel, 64 takes LONG, same shape otherwise
    a, b = names["runs-to-63"], names["runs-to-64"]
    assert (a["nchan"], a["nbin"], a["ndat"]) == (b["nchan"], b["nbin"], b["ndat"])
    # the weighted plan of the GPU test: zero-weight blocks at the start, in the middle and at the end end runs
    plan = oracle.fold_binplan(0.2, 1.0 / (3.1 * 37), 37, 3000)
    w = np.ones(30, np.uint32)
    w[[0, 13, 14, 29]] = 0
    runs, keep = mc.weighted_runs(plan, 0, w, 100)
    assert not keep[:100].any() and not keep[1300:1500].any() and not keep[2900:].any() and keep.sum() == 2600
    assert runs[:, 2].sum() == 2600 and runs[0, 0] == 100 and runs[-1, 0] + runs[-1, 2] == 2900
