"""Two-bit voltages, the host side (no device): dspsr_amd.twobit's limits and level table, its three weight operations against
brute-force statements of what they do, the refusals of dspsr_amd_twobit_check one by one, the NBIT 2 header cases of DadaFile, the
plan-time refusals of the drivers, and the proof that every case of tests/twobit_cases.py reaches the edges it is there for."""
import dataclasses
import math

import numpy as np
import pytest

import twobit_cases as tc


# ---- limits and levels ---------------------------------------------------------------------------------------------------------
def test_limits_values_cutoff_zero_and_error():
    from dspsr_amd import twobit, DspsrAmdError
    assert twobit.limits(512) == (234, 447)
    assert twobit.limits(64) == (4, 63)
    assert twobit.limits(8) == (1, 7)
    assert twobit.limits(512, cutoff_sigma=0) == (0, 512) and twobit.limits(8, cutoff_sigma=0.0) == (0, 8)
    for nsample in tc.NSAMPLES:
        assert twobit.limits(nsample) == tc.limits_restated(nsample)
    # a threshold so high that every sample is expected low: float(nsample * erf(t / sqrt 2)) == nsample
    with pytest.raises(DspsrAmdError, match="sampling threshold error: mean nlow=512.000000 == sample size=512.000000"):
        twobit.limits(512, threshold=8.0)


@pytest.mark.parametrize("nsample,threshold", [(512, 0.9674), (64, 0.9674), (8, 0.9674), (4, 0.9674), (512, 1.2)])
def test_levels_against_the_float64_restatement(nsample, threshold):
    from dspsr_amd import twobit
    for cutoff in (10.0, 0.0):                              # cutoff 0: nlo = 0 and nlo = nsample, the two clamps
        nlow_min, nlow_max = twobit.limits(nsample, threshold, cutoff)
        got = twobit.levels(nsample, nlow_min, nlow_max, threshold)
        want = tc.levels_restated(nsample, nlow_min, nlow_max, threshold)
        assert got.dtype == np.float32 and got.shape == (nlow_max - nlow_min + 1, 2)
        # the two double computations agree to ~1e-14: they can only straddle a float32 rounding boundary
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, "levels differ by %d float32 ulps" % ulps.max()
        assert np.isfinite(got).all() and (got[:, 0] > 0).all() and (got[:, 1] > got[:, 0]).all()
    if nsample > 4:
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[-1], got[-2])      # nlo 0 uses 1, nlo nsample uses nsample - 1


def test_levels_conserve_power():
    """Phi lo^2 + (1 - Phi) hi^2 = sigma^2: the digitised power equals the undigitised (JA98 eq. 41's purpose), in double"""
    from dspsr_amd import twobit
    for nsample in (8, 64, 512):
        for nlo in range(1, nsample):
            phi = float(np.float32(nlo) / np.float32(nsample))
            lo, hi = twobit.ja98_levels(phi)
            sigma = twobit.THRESHOLD / (math.sqrt(2.0) * twobit.erf_inverse(phi))
            assert abs(phi * lo * lo + (1.0 - phi) * hi * hi - sigma * sigma) <= 1e-12 * sigma * sigma
            assert abs(math.erf(twobit.erf_inverse(phi)) - phi) <= 4e-16


def test_levels_refuses_bad_limits():
    from dspsr_amd import twobit, DspsrAmdError
    for args in ((512, 300, 300), (512, 10, 513), (512, -1, 5)):
        with pytest.raises(DspsrAmdError, match="nlow_min"):
            twobit.levels(*args)


# ---- the weight operations -----------------------------------------------------------------------------------------------------
def test_mask_weights_against_brute_force():
    from dspsr_amd import twobit
    rng = np.random.default_rng(5)
    for nparts in (1, 2, 3):
        w = (rng.random((nparts, 23)) > 0.2).astype(np.uint32)
        got = twobit.mask_weights(w)
        assert np.array_equal(got, tc.mask_restated(w)) and got.dtype == np.uint32
        assert np.array_equal(w, (w != 0).astype(np.uint32))                 # the argument is not written


def _convolve_brute(w, ndat, npw, widat, nfft, nkeep):
    """What convolve_weights does, said another way: transform t tests the weights as the transforms up to t - 2 left them (the
    reference flags the previous transform only after it has tested the next); every bad transform's range ends up zero."""
    w = np.array(w, dtype=np.uint32)
    if npw >= nfft or ndat + nkeep < nfft:
        return w
    ntrans = (ndat + nkeep - nfft) // nkeep
    ranges, bad = [], []
    for t in range(ntrans):
        seen = w.copy()
        for u in range(t - 1):
            if bad[u]:
                seen[ranges[u][0]:ranges[u][1]] = 0
        start = int((t * nkeep + widat) * (1.0 / npw))
        end = int(math.ceil((t * nkeep + widat + nfft) * (1.0 / npw)))
        bad.append(bool((seen[start:end] == 0).any()))
        ranges.append((start, int(math.ceil((t * nkeep + nkeep) * (1.0 / npw)))))
    for t in range(ntrans):
        if bad[t]:
            w[ranges[t][0]:ranges[t][1]] = 0
    return w


@pytest.mark.parametrize("npw,nfft,nkeep", [(64, 32, 24), (32, 32, 24), (8, 32, 24), (4, 64, 40), (12, 100, 70), (16, 16, 16), (4, 16, 16)])
@pytest.mark.parametrize("widat", [0, 3])
def test_convolve_weights_against_brute_force(npw, nfft, nkeep, widat):
    """ndat_per_weight above, equal to and below nfft; weight_idat zero and not; a bad weight in the first, a middle and the last
    transform, one at a time and all together; a block too short for one transform"""
    from dspsr_amd import twobit
    widat = min(widat, npw - 1)
    ntrans = 6
    ndat = (ntrans - 1) * nkeep + nfft + 5
    nweights = twobit.get_nweights(ndat + widat, npw)
    mid = lambda t: min(nweights - 1, (t * nkeep + widat + nfft // 2) // npw)
    spots = [[mid(0)], [mid(ntrans // 2)], [mid(ntrans - 1)], [0], [nweights - 1], [mid(0), mid(ntrans // 2), mid(ntrans - 1)], []]
    for bad in spots:
        w = np.ones(nweights, dtype=np.uint32)
        w[bad] = 0
        got, npw2, widat2 = twobit.convolve_weights(w, ndat, npw, widat, nfft, nkeep)
        assert (npw2, widat2) == (npw, widat)
        want = _convolve_brute(w, ndat, npw, widat, nfft, nkeep)
        assert np.array_equal(got, want), "bad %s: %s, want %s" % (bad, got.tolist(), want.tolist())
        if npw < nfft and bad:
            assert (got == 0).sum() >= (w == 0).sum()
        if npw >= nfft:
            assert np.array_equal(got, w)                                    # the fft happens within one weight
    short = np.array([1, 0, 1], dtype=np.uint32)
    assert np.array_equal(twobit.convolve_weights(short, nfft - nkeep - 1, 1, 0, nfft, nkeep)[0], short)


@pytest.mark.parametrize("npw,widat,nscrunch", [(64, 0, 16), (64, 5, 16), (64, 32, 16), (16, 3, 16), (8, 0, 16), (8, 3, 16), (4, 1, 16), (4, 0, 6)])
def test_scrunch_weights_against_brute_force(npw, widat, nscrunch):
    from dspsr_amd import twobit
    rng = np.random.default_rng(npw + widat)
    for nweights in (1, 7, 16, 33):
        w = (rng.random(nweights) > 0.25).astype(np.uint32)
        got, npw2, widat2 = twobit.scrunch_weights(w, npw, widat, nscrunch)
        if npw >= nscrunch:
            assert np.array_equal(got, w) and npw2 == npw // nscrunch
            assert widat2 == -(-widat // npw2)                               # rounded up (WeightedTimeSeries.C:727-730)
        else:
            groups = [w[k:k + nscrunch] for k in range(0, nweights, nscrunch)]
            want = [0 if (g == 0).any() else int(g.sum()) // len(g) for g in groups]
            assert got.tolist() == want and (npw2, widat2) == (1, widat)
    # ndat: only the weights that cover ndat samples count
    w = np.array([1, 1, 1, 1, 0, 1, 1, 1], dtype=np.uint32)
    got, _, _ = twobit.scrunch_weights(w, 4, 0, 8, ndat=16)
    assert got.tolist() == [1]


# ---- the device-free check -----------------------------------------------------------------------------------------------------
def test_twobit_check_refusals_one_by_one():
    import dspsr_amd
    from dspsr_amd import DspsrAmdError
    ok = dict(raw_addr=4096, table_type=dspsr_amd.TWOBIT_OFFSET_BINARY, npol=2, nsample=512, first_sample=0, ndat=2048, nlow_min=234,
              nlow_max=447, out_addr=8192, out_pol_stride=2048)
    dspsr_amd.twobit_check(**ok)
    for t in (dspsr_amd.TWOBIT_SIGN_MAGNITUDE, dspsr_amd.TWOBIT_TWOS_COMPLEMENT):
        dspsr_amd.twobit_check(**dict(ok, table_type=t))
    dspsr_amd.twobit_check(**dict(ok, nsample=4, nlow_min=1, nlow_max=3, first_sample=3, ndat=1))
    dspsr_amd.twobit_check(**dict(ok, nsample=65536, nlow_min=0, nlow_max=65536, first_sample=65535))
    dspsr_amd.twobit_check(**dict(ok, npol=1, out_pol_stride=0, out_addr=8196))
    for change, words in ((dict(nsample=510), "multiple of 4"), (dict(nsample=0), "multiple of 4"), (dict(nsample=65540), "65536"),
                          (dict(nlow_max=234), "nlow_min"), (dict(nlow_max=200), "nlow_min"), (dict(nlow_max=513), "nsample"),
                          (dict(first_sample=512), "first_sample"), (dict(npol=0), "npol"), (dict(npol=4), "npol"),
                          (dict(raw_addr=4098), "4 bytes"), (dict(raw_addr=4097), "4 bytes"), (dict(out_pol_stride=2047), "overlap"),
                          (dict(table_type=3), "table_type"), (dict(table_type=-1), "table_type"), (dict(out_addr=8194), "4-byte"),
                          (dict(ndat=1 << 32), "too large")):
        with pytest.raises(DspsrAmdError, match=words):
            dspsr_amd.twobit_check(**dict(ok, **change))


def test_header_declares_the_entry_points():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dspsr_amd.h")).read()
    for k, name in enumerate(("OFFSET_BINARY", "SIGN_MAGNITUDE", "TWOS_COMPLEMENT")):
        assert re.search(r"#define DSPSR_AMD_TWOBIT_%s %d\b" % (name, k), text)
    assert "dspsr_amd_twobit_unpack(" in text and "dspsr_amd_twobit_check(" in text


# ---- DADA headers and the drivers' plans --------------------------------------------------------------------------------------
def _write(path, data, **kw):
    from dspsr_amd import synth
    args = dict(freq=1400.0, bw=16.0, nchan=1, npol=2, ndim=1, tsamp_us=1.0 / 32.0, instrument="CPSR2")
    args.update(kw)
    hdr = synth.dada_header(args["freq"], args["bw"], args["nchan"], args["npol"], args["ndim"], args["tsamp_us"],
                            instrument=args["instrument"]).replace(b"NBIT 8", b"NBIT 2")
    path.write_bytes(hdr + np.asarray(data, dtype=np.uint8).tobytes())
    return str(path)


class _Geometry:
    """what DadaFile.blocks reads of a LoadToFold"""

    def __init__(self, nsample, step, overlap, ppb):
        from types import SimpleNamespace
        from dspsr_amd import inputs
        self.form = inputs.TwoBit(granule=nsample)
        self.nsamp_step, self.nsamp_overlap = step, overlap
        self.cfg = SimpleNamespace(parts_per_block=ppb)


def test_nbit2_header_cases(tmp_path):
    from dspsr_amd import dada, DspsrAmdError, _lib
    data = np.arange(4000, dtype=np.uint8)
    f = dada.DadaFile(_write(tmp_path / "a.dada", data))
    assert f.twobit and f.info.nbit == 2 and f.table_type == _lib.TWOBIT_OFFSET_BINARY and f.ndat == 8000
    assert dada.DadaFile(_write(tmp_path / "b.dada", data[:3999], npol=1)).ndat == 4 * 3999
    assert dada.DadaFile(_write(tmp_path / "c.dada", data[:3999])).ndat == 4 * 1999         # whole bytes of both digitisers
    for kw, words in ((dict(instrument="APSR"), "NBIT=2 with INSTRUMENT APSR"), (dict(instrument="DADA"), "NBIT=2"),
                      (dict(ndim=2), "NDIM=2"), (dict(nchan=2), "NCHAN=2"), (dict(npol=4), "NPOL=4")):
        with pytest.raises(DspsrAmdError, match=words):
            dada.DadaFile(_write(tmp_path / "x.dada", data, **kw))
    # blocks: whole windows from the one that holds the block's first sample; the samples behind the last whole window are dropped
    lt = _Geometry(nsample=64, step=100, overlap=30, ppb=3)
    f = dada.DadaFile(_write(tmp_path / "d.dada", data[:3990]))
    assert f.ndat == 7980
    assert f.usable(lt) == 7936 and f.nblocks(lt) == divmod((7936 - 30) // 100, 3)
    got = list(f.blocks(lt))
    assert len(got) == 27 and got[-1][1] == 1
    for b, (block, npart, first) in enumerate(got):
        s0, nsamp = b * 300, npart * 100 + 30
        assert first == s0 % 64
        w0, w1 = s0 // 64, -(-(s0 + nsamp) // 64)
        assert np.array_equal(np.asarray(block).view(np.uint8), data[w0 * 32:w1 * 32]) and w1 * 64 <= 7936
    with pytest.raises(DspsrAmdError, match="one channel"):
        next(f.blocks(lt, channel=0))
    # a file shorter than one window gives no blocks
    short = dada.DadaFile(_write(tmp_path / "s.dada", data[:30]))
    assert short.ndat == 60 and short.nblocks(_Geometry(64, 10, 4, 2)) == (0, 0) and list(short.blocks(_Geometry(64, 10, 4, 2))) == []


def test_plan_refusals_by_name():
    from dspsr_amd import pipeline, DspsrAmdError
    info = pipeline.InputInfo(centre_frequency=1400.0, bandwidth=16.0, nchan=1, npol=2, ndim=1, tsamp_us=1.0 / 32.0, machine="CPSR2", nbit=2)
    cfg = pipeline.Config(nchan=8, dispersion_measure=2.0, nbin=32, folding_period=0.004, freq_res=64, parts_per_block=4)
    plan = pipeline.twobit_check(cfg, info)
    assert (plan.nsample, plan.nlow_min, plan.nlow_max, plan.table_type) == (512, 234, 447, 0) and plan.levels.shape == (214, 2)
    plan = pipeline.twobit_check(dataclasses.replace(cfg, excision_nsample=64, excision_cutoff=0.0, excision_threshold=1.1), info)
    assert (plan.nsample, plan.nlow_min, plan.nlow_max, plan.threshold) == (64, 0, 64, 1.1)
    for change, words in ((dict(cyclic_nchan=16, ndim=1), "-cyclic"), (dict(plfb_nbin=16, ndim=1), "-G"), (dict(fourth_moment=True), "-4"),
                          (dict(interchan_dedispersion=True), "-K"), (dict(zap_rfi=True), "-R"), (dict(sk_zap=True), "-skz"),
                          (dict(calibrator=(np.zeros(2), np.zeros((2, 2, 2)))), "-pac"), (dict(convolve_when="after"), "-F N:D"),
                          (dict(convolve_when="before"), "-F N:D"), (dict(excision_nsample=510), "excision_nsample")):
        with pytest.raises(DspsrAmdError, match="two-bit input.*%s" % words):
            pipeline.LoadToFold(dataclasses.replace(cfg, **change), info)
    with pytest.raises(DspsrAmdError, match="two-bit input.*one pulsar"):
        pipeline.LoadToFold(cfg, info, targets=[pipeline.FoldTarget(folding_period=0.004), pipeline.FoldTarget(folding_period=0.005)])
    with pytest.raises(DspsrAmdError, match="two-bit input.*sub-band"):
        pipeline.LoadToFold(cfg, info, subband=0)
    with pytest.raises(DspsrAmdError, match="two-bit input.*INSTRUMENT"):
        pipeline.LoadToFold(cfg, dataclasses.replace(info, machine="APSR"))
    scfg = pipeline.SearchConfig(nchan=64, tscrunch=16, nbit=8, parts_per_block=16)
    for driver in (pipeline.LoadToFil, pipeline.LoadToFilCoherent, pipeline.LoadToFilDirect):
        with pytest.raises(DspsrAmdError, match="two-bit input"):
            driver(scfg, info)


def test_tool_options():
    import io
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import dspsr_amd_fold as tool
    a = tool.parse_args(["-F", "8:D", "-2", "c5.5", "-2n64", "-2", "t1.1", "-2", "zzz", "x.dada"])
    log = io.StringIO()
    assert tool.unpacker_options(a.unpack, log) == {"excision_cutoff": 5.5, "excision_nsample": 64, "excision_threshold": 1.1}
    assert log.getvalue().splitlines() == ["dspsr: Setting impulsive interference excision threshold to 5.5",
                                           "dspsr: Using 64 samples to estimate undigitized power",
                                           "dspsr: Setting two-bit sampling threshold to 1.1"]
    assert tool.unpacker_options(tool.parse_args(["-F", "8:D", "x.dada"]).unpack, log) == {}


# ---- the generator reaches its edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_generator_case_reaches_its_edges(case):
    from dspsr_amd import twobit
    table_type, npol, nsample = case
    block, nlow_min, nlow_max = tc.stream(*case)
    assert (nlow_min, nlow_max) == twobit.limits(nsample)
    levels = twobit.levels(nsample, nlow_min, nlow_max)
    rows, weights, n_low = tc.unpack_restated(block, table_type, npol, nsample, nlow_min, nlow_max, levels)
    nbyte = nsample // 4
    for idig in range(npol):
        zero = [not block[idig::npol][w * nbyte:(w + 1) * nbyte].any() for w in range(weights.shape[1])]
        few = [(not z) and n < nlow_min for z, n in zip(zero, n_low[idig])]
        many = [(not z) and n > nlow_max for z, n in zip(zero, n_low[idig])]
        assert any(zero) and any(few) and any(many), "an excision cause is missing"
        assert all(weights[idig][w] == 0 for w in range(len(zero)) if zero[w] or few[w] or many[w])
        kept = weights[idig] == 1
        assert (n_low[idig][kept] == nlow_min).any() and (n_low[idig][kept] == nlow_max).any(), "an edge of the limits is not reached"
        assert 2 * kept.sum() >= kept.size
        for w in range(kept.size):
            seg = rows[idig, w * nsample:(w + 1) * nsample]
            assert (seg != 0).all() if kept[w] else (seg == 0).all()
        assert len({tuple(np.unique(np.abs(rows[idig, w * nsample:(w + 1) * nsample]))) for w in np.nonzero(kept)[0]}) >= 2 or nsample == 4
    masked = tc.mask_restated(weights)
    assert 2 * (masked[0] == 1).sum() >= masked.shape[1]
    if npol == 2:
        assert ((weights[0] == 0) & (weights[1] == 1)).any() and ((weights[0] == 1) & (weights[1] == 0)).any()
