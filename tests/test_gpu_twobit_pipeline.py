"""Two-bit input through LoadToFold (`dspsr -F 8:D` on an NBIT 2 file of INSTRUMENT CPSR2): a dispersed pulse in noise, quantised to
two bits, with bursts of interference over a few excision windows and one window of zero bytes.  nsample is 64, so that the
16384 samples of a polarisation hold 256 windows; 29 overlap-save parts of 544 samples (34 windows to every 4 parts).

dada.fold_file against: the loop restatement of the unpacker (tests/twobit_cases.py) -> oracle.filterbank -> oracle.detect_* -> a fold
whose plan is oracle.fold_binplan_weighted with the masked, convolved and scrunched weights of every block.  Hits and
discarded_weights identical, the profile within 1e-5 of its maximum (the project's bound for a float32 path against float64,
tests/test_gpu_parity.py:7).

Block cuts.  WeightedTimeSeries carries weight_idat, the place of a block's first sample inside its first weight, and two of the
reference's steps are not neutral to it: convolve_weights ends a flagged range at ceil((start_idat + nkeep) / ndat_per_weight)
without it (:676), and scrunch_weights divides it by the NEW ndat_per_weight, not by the scrunch factor (:725-730).  Blocks that
start on a window (weight_idat 0) therefore drop the same samples however the file is cut, and those runs must agree bit for bit;
a cut whose blocks start inside a window is compared with the restatement made for that cut."""
import io
import os
import sys

import numpy as np
import pytest

import twobit_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FREQ, BW, TSAMP, DM, NCHAN, NBIN, FREQ_RES, NSAMPLE = 1382.0, -16.0, 1.0 / 32.0, 2.0, 8, 16, 64, 64
PERIOD = 6.4e-5                     # 2048 input samples, 128 output samples: eight turns in the file
NWINDOW = 256
NDAT = NWINDOW * NSAMPLE
BURSTS = ((0, 40, 43), (1, 120, 122), (0, 121, 122))          # (polarisation, first window, end): sigma x 200
ZERO = (1, 200)                                         # (polarisation, window) of zero bytes


def _pack(codes):
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, 4)
    return (c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]


def _file_bytes(rfi, seed=11):
    """the two-bit block of the whole file: byte k belongs to polarisation k % 2"""
    from dspsr_amd import synth
    x = synth.voltages(NDAT, FREQ, BW, TSAMP, DM, PERIOD, pulse_amp=1.0, seed=seed).astype(np.float64).reshape(NDAT, 2) / 24.0
    if rfi:
        for pol, w0, w1 in BURSTS:
            x[w0 * NSAMPLE:w1 * NSAMPLE, pol] *= 200.0          # (the limits of 64 samples are 4 ... 63: ten sigma is far out)
    block = np.zeros(NDAT // 4 * 2, dtype=np.uint8)
    code = np.array([[tc.code_of(tc.OFFSET_BINARY, n, h) for h in (False, True)] for n in (False, True)], dtype=np.uint8)
    for pol in range(2):
        block[pol::2] = _pack(code[(x[:, pol] < 0).astype(int), (np.abs(x[:, pol]) >= tc.THRESHOLD).astype(int)])
    if rfi:
        pol, w = ZERO
        block[pol::2][w * NSAMPLE // 4:(w + 1) * NSAMPLE // 4] = 0
    return block


def _write(path, block, tail=b""):
    from dspsr_amd import synth
    hdr = synth.dada_header(FREQ, BW, 1, 2, 1, TSAMP, instrument="CPSR2").replace(b"NBIT 8", b"NBIT 2")
    with open(path, "wb") as f:
        f.write(hdr + block.tobytes() + tail)
    return str(path)


def _config(**over):
    from dspsr_amd import pipeline
    return pipeline.Config(**{**dict(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, freq_res=FREQ_RES, ndim=4,
                                     parts_per_block=4, max_parts=2, force_fused=True, excision_nsample=NSAMPLE), **over})


def _run(path, **over):
    import torch
    from dspsr_amd import dada
    lt = dada.fold_file(path, _config(**over), stream=torch.cuda.current_stream().cuda_stream)
    assert len(lt.subints) == 1
    s = lt.subints[0]
    out = dict(hits=s["hits"].copy(), profile=s["profile_dev"].cpu().numpy(), ndat_total=s["ndat_total"],
               integration_length=s["integration_length"], discarded=lt.twobit.discarded_weights, fused=lt.twobit.blocks_fused,
               weighted=lt.twobit.blocks_weighted, nkeep=lt.nkeep, step=lt.nsamp_step, overlap=lt.nsamp_overlap, rate=lt.out_rate,
               fused_mode=lt.fused_mode, limits=(lt.twobit.nlow_min, lt.twobit.nlow_max), ndat_out=lt.ndat_out)
    lt.close()
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("twobit")
    rfi, clean = _file_bytes(True), _file_bytes(False)
    # 37 bytes behind the last whole window: dropped
    return dict(rfi=_write(d / "rfi.dada", rfi, tail=b"\x5a" * 37), clean=_write(d / "clean.dada", clean), rfi_block=rfi)


@pytest.fixture(scope="module")
def restated(oracle, files):
    """the float64 chain on the restated unpacking, once: detected samples, the masked weights of every window, the geometry"""
    import dspsr_amd
    from dspsr_amd import twobit
    o = oracle
    nlow_min, nlow_max = twobit.limits(NSAMPLE)
    rows, weights, _ = tc.unpack_restated(files["rfi_block"], tc.OFFSET_BINARY, 2, NSAMPLE, nlow_min, nlow_max,
                                          twobit.levels(NSAMPLE, nlow_min, nlow_max))
    obs = o.Observation(centre_frequency=FREQ, bandwidth=BW, tsamp_us=TSAMP, dispersion_measure=DM)
    resp = dspsr_amd.Dedispersion(FREQ, BW, DM)
    resp.set_frequency_resolution(FREQ_RES)
    resp.match(NCHAN)
    oresp = o.Dedispersion()
    oresp.set_frequency_resolution(FREQ_RES)
    oresp.match(obs, NCHAN)
    plan = o.filterbank_plan(obs, NCHAN, oresp)
    fb = o.filterbank(rows.reshape(1, 2, NDAT), plan, resp.kernel, dtype=np.float64)
    det = o.detect_layout(o.detect_products(fb, "Coherence"), 4)
    return dict(det=det, masked=tc.mask_restated(weights), weights=weights, plan=plan, fobs=o.filterbank_output_observation(obs, plan))


def _expected(oracle, r, ppb):
    """hits, profile (float64) and discarded_weights of the file cut into blocks of ppb parts"""
    from dspsr_amd import twobit
    o, plan, fobs, det = oracle, r["plan"], r["fobs"], r["det"]
    step, nfft, nkeep = plan.nsamp_step, plan.nsamp_fft, plan.nkeep
    overlap = nfft - step
    nparts = (NDAT - overlap) // step
    assert det.shape[2] == nparts * nkeep
    cfg = o.FoldConfig(nbin=NBIN, folding_period=PERIOD)
    hits = np.zeros(NBIN, np.uint32)
    prof = np.zeros((NCHAN, 1, NBIN + 1, 4), np.float64)
    discarded, firsts, dropped = 0, [], 0
    for p0 in range(0, nparts, ppb):
        npart = min(ppb, nparts - p0)
        s0, nsamp = p0 * step, npart * step + overlap
        first = s0 % NSAMPLE
        firsts.append(first)
        w = r["masked"][0][s0 // NSAMPLE:-(-(s0 + nsamp) // NSAMPLE)]
        discarded += int((w == 0).sum())
        row, npw, widat = twobit.convolve_weights(w, nsamp, NSAMPLE, first, nfft, step)
        row, npw, widat = twobit.scrunch_weights(row, npw, widat, nfft // FREQ_RES, ndat=nsamp)
        i0, n = p0 * nkeep, npart * nkeep
        phi, pfold = o.fold_phase(cfg, fobs, fobs.start_seconds + (i0 + 0.5) / fobs.rate)
        binplan = o.fold_binplan_weighted(phi, (1.0 / fobs.rate) / pfold, NBIN, 0, n, row, npw, widat)
        hits += np.bincount(binplan, minlength=NBIN + 1)[:NBIN].astype(np.uint32)
        dropped += int((binplan == NBIN).sum())
        np.add.at(prof, (slice(None), slice(None), binplan), det[:, :, i0:i0 + n, :])
    return dict(hits=hits, profile=prof[:, :, :NBIN, :], discarded=discarded, firsts=firsts, dropped=dropped, ndat=nparts * nkeep)


@pytest.fixture(scope="module")
def runs(files):
    """the file in one block, in blocks that start on windows (7 x 4 + 1 parts) and in blocks of which every other starts inside a
    window (9 x 3 + 2)"""
    return {ppb: _run(files["rfi"], parts_per_block=ppb) for ppb in (64, 4, 3)}


@pytest.mark.parametrize("ppb", [64, 4, 3])
def test_fold_file_against_the_restated_chain(oracle, restated, runs, ppb):
    got, want = runs[ppb], _expected(oracle, restated, ppb)
    plan = restated["plan"]
    assert (got["step"], got["overlap"], got["nkeep"]) == (plan.nsamp_step, plan.nsamp_fft - plan.nsamp_step, plan.nkeep)
    assert got["limits"] == (4, 63) and got["ndat_out"] == want["ndat"] == got["ndat_total"]
    # the case is what it says: bad windows in each polarisation alone, a zero window, dropped and folded samples, and for ppb 3
    # blocks that start inside a window
    w = restated["weights"]
    assert ((w[0] == 0) & (w[1] == 1)).any() and ((w[0] == 1) & (w[1] == 0)).any() and w[ZERO[0], ZERO[1]] == 0
    assert 0 < want["dropped"] < want["ndat"] // 2
    assert any(want["firsts"]) == (ppb == 3) and len(want["firsts"]) == {64: 1, 4: 8, 3: 10}[ppb]       # (29 parts: ragged last blocks)
    assert np.array_equal(got["hits"], want["hits"]), "hits differ"
    assert got["discarded"] == want["discarded"] > 0
    assert int(got["hits"].sum()) == want["ndat"] - want["dropped"]
    assert abs(got["integration_length"] - (want["ndat"] - want["dropped"]) / got["rate"]) <= 1e-12
    err = np.abs(got["profile"].reshape(want["profile"].shape) - want["profile"]).max() / np.abs(want["profile"]).max()
    print("ppb %d: profile error %.3g of the maximum, %d of %d samples dropped, %d weights discarded" % (
        ppb, err, want["dropped"], want["ndat"], want["discarded"]))
    assert err <= 1e-5


def test_block_cuts_on_window_starts_give_identical_bits(runs):
    one, several = runs[64], runs[4]
    assert several["weighted"] >= 1 and one["weighted"] == 1
    assert np.array_equal(one["hits"], several["hits"])
    assert np.array_equal(one["profile"].view(np.int32), several["profile"].view(np.int32))


def test_clean_file_equals_cutoff_zero_and_takes_the_fused_fold(files):
    a = _run(files["clean"], parts_per_block=3)
    b = _run(files["clean"], parts_per_block=3, excision_cutoff=0.0)
    assert a["limits"] == (4, 63) and b["limits"] == (0, 64)
    assert a["discarded"] == b["discarded"] == 0
    assert a["fused_mode"] != 0 and a["fused"] == b["fused"] == 10 and a["weighted"] == b["weighted"] == 0
    assert np.array_equal(a["hits"], b["hits"]) and int(a["hits"].sum()) == a["ndat_out"]
    assert np.array_equal(a["profile"].view(np.int32), b["profile"].view(np.int32))
    # and the fused fold gives what Detection + Fold gives
    c = _run(files["clean"], parts_per_block=3, fused_fold=False)
    assert c["fused"] == 0 and np.array_equal(c["hits"], a["hits"])
    if a["fused_mode"] == 1:                                 # exact time-order sums
        assert np.array_equal(c["profile"].view(np.int32), a["profile"].view(np.int32))
    else:
        assert np.abs(c["profile"] - a["profile"]).max() <= 1e-5 * np.abs(a["profile"]).max()


def test_engine_raw_form_returns_the_weights(files, restated):
    """FilterbankEngine's two-bit form: a RAW_TWOBIT block through perform_raw equals unpack_twobit + perform, and the per-digitiser
    weights come back with it"""
    import torch
    import dspsr_amd
    from dspsr_amd import _lib, twobit
    plan = restated["plan"]
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    resp = dspsr_amd.Dedispersion(FREQ, BW, DM)
    resp.set_frequency_resolution(FREQ_RES)
    resp.match(NCHAN)
    eng = dspsr_amd.FilterbankEngine(ctx).setup(plan.nchan_subband, plan.freq_res, plan.nfilt_pos, plan.nfilt_neg, 1, 2, True, resp.kernel,
                                                max_parts=2)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="set_twobit"):
        eng.unpack_twobit(torch.zeros(64, dtype=torch.uint8, device="cuda"), 0, 1)
    nlow_min, nlow_max = twobit.limits(NSAMPLE)
    eng.set_twobit(NSAMPLE, nlow_min, nlow_max, twobit.levels(NSAMPLE, nlow_min, nlow_max))
    npart, p0 = 3, 1
    s0, nsamp = p0 * eng.nsamp_step, npart * eng.nsamp_step + eng.nsamp_overlap
    first, w0, w1 = s0 % NSAMPLE, s0 // NSAMPLE, -(-(s0 + nsamp) // NSAMPLE)
    assert first != 0
    raw = torch.from_numpy(files["rfi_block"][w0 * 32:w1 * 32].copy()).cuda()
    out = torch.zeros((NCHAN, 2, 2 * npart * eng.nkeep), dtype=torch.float32, device="cuda")
    eng.perform_raw(raw, _lib.twobit_at(first), 1.0, out, npart)
    ctx.synchronize()
    assert np.array_equal(eng.twobit_weights.cpu().numpy().view(np.uint32), restated["weights"][:, w0:w1])
    rows, in_step, _ = eng.unpack_twobit(raw, first, npart)
    ref = torch.zeros_like(out)
    eng.perform(rows, ref, npart, in_step, 2 * eng.nkeep)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int32), ref.cpu().numpy().view(np.int32))
    eng.close()
    ctx.close()


def test_tool_options_reach_config(files, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dspsr_amd_fold as tool
    from dspsr_amd import dada
    seen = {}

    class Stop(Exception):
        pass

    def spy(path, cfg, **kw):
        seen["cfg"] = cfg
        raise Stop

    monkeypatch.setattr(dada, "fold_file", spy)
    monkeypatch.setattr(sys, "stderr", io.StringIO())
    with pytest.raises(Stop):
        tool.main(["-F", "8:D", "-D", "2", "-c", str(PERIOD), "-b", "16", "-x", "64", "-2", "c7.5", "-2n64", "-2", "t1.05", files["clean"]])
    cfg = seen["cfg"]
    assert (cfg.excision_cutoff, cfg.excision_nsample, cfg.excision_threshold) == (7.5, 64, 1.05)
    with pytest.raises(Stop):
        tool.main(["-F", "8:D", "-D", "2", "-c", str(PERIOD), files["clean"]])
    assert (seen["cfg"].excision_cutoff, seen["cfg"].excision_nsample, seen["cfg"].excision_threshold) == (-1.0, 0, -1.0)


def test_report_shows_the_discarded_weights(files):
    import torch
    from dspsr_amd import dada
    lt = dada.fold_file(files["rfi"], _config(parts_per_block=64, record_time=True), stream=torch.cuda.current_stream().cuda_stream)
    text = io.StringIO()
    lt.report(text)
    n = lt.twobit.discarded_weights
    lt.close()
    line = [l for l in text.getvalue().splitlines() if l.startswith("TwoBitCorrection")]
    assert n > 0 and len(line) == 1 and line[0].split()[-1] == str(n)
