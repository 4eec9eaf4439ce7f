"""`dspsr -skz` through LoadToFold (dspsr_amd/pipeline.py: KurtosisFold) on a 16-channel, 8-bit, dual-polarisation synthetic
observation: Gaussian noise, a weak pulse, and in one channel a tone that is on for one eighth of every 128 output samples.
The driver against the same steps made by hand through the public engines, bit for bit; the cleaned rows against the mask; the
restatement (tests/sk_reference.py) on the device's voltages for what is zapped; the files and the tool."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dspsr_amd
import sk_reference as ref
from dspsr_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FREQ, BW, TSAMP, DM, PERIOD, NCHAN, NBIN, M = 1382.0, -16.0, 1.0 / 32.0, 1.0, 0.004, 16, 64, 128
NBLOCK = 3
TONE_MHZ, TONE_AMP = 5.5, 30.0          # baseband frequency of the tone (the middle of one 1 MHz channel) and its amplitude;
                                        # the noise has sigma 24 over 16 MHz, 6 per channel: the tone is 12.5 times a channel's power
SEED, PULSE_AMP = 4, 0.25               # a seed for which the restatement alone meets the condition of the second test (one in
                                        # three seeds loses a whole block of some channel to tscr: 96 trials at 3 sigma)


def _config(pipeline, **over):
    return pipeline.Config(**{**dict(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, ndim=4, parts_per_block=1,
                                     max_parts=2, sk_zap=True, sk_m=M), **over})


def _info(pipeline):
    return pipeline.InputInfo(centre_frequency=FREQ, bandwidth=BW, tsamp_us=TSAMP, machine="DADA")     # the generic 8-bit order


@pytest.fixture(scope="module")
def obs():
    """The observation, the block geometry and one -skz run of the driver with -L (shared, never changed)."""
    import torch
    from dspsr_amd import pipeline, synth
    probe = pipeline.LoadToFold(_config(pipeline), _info(pipeline), stream=torch.cuda.current_stream().cuda_stream)
    nkeep, step, overlap, rate = probe.nkeep, probe.nsamp_step, probe.nsamp_overlap, probe.out_rate
    probe.close()
    ppb = -(-64 * M // nkeep)                                 # blocks of (a little more than) 64 parts of M samples
    assert (ppb * nkeep) % M, "the block must leave a carried tail"
    nsamp = NBLOCK * ppb * step + overlap
    raw = synth.voltages(nsamp, FREQ, BW, TSAMP, DM, PERIOD, pulse_amp=PULSE_AMP, seed=SEED).astype(np.float64).reshape(nsamp, 2)
    t = np.arange(nsamp)
    on = ((t // 32) % M) < M // 8                             # 32 input samples per output sample: 1/8 duty in every M samples
    raw += (TONE_AMP * np.cos(2 * np.pi * TONE_MHZ / 32.0 * t) * on)[:, None]
    raw = np.clip(np.rint(raw), -128, 127).astype(np.int8).reshape(-1)
    length = 1.5 * ppb * nkeep / rate                         # -L: the first boundary lies in the middle of block two
    return dict(raw=torch.from_numpy(raw).cuda(), ppb=ppb, nkeep=nkeep, step=step, overlap=overlap, rate=rate, L=length)


def _blocks(o):
    step = o["ppb"] * o["step"]
    for b in range(NBLOCK):
        yield o["raw"][2 * b * step: 2 * (b * step + step + o["overlap"])]


def _drive(o, **over):
    """LoadToFold over the three blocks -> (entries of subints as host copies, the driver's members of interest)"""
    import torch
    from dspsr_amd import pipeline
    cfg = _config(pipeline, parts_per_block=o["ppb"], **over)
    lt = pipeline.LoadToFold(cfg, _info(pipeline), stream=torch.cuda.current_stream().cuda_stream)
    cleaned = []
    if cfg.sk_zap:                                           # the rows SpectralKurtosis cleaned in each block, and its mask
        transform = lt.sk.transform

        def spy(inp, out, ndat):
            n = transform(inp, out, ndat)
            assert inp.data_ptr() == out.data_ptr()          # in place
            cleaned.append((out[:, :, :2 * n].cpu().numpy(), lt.sk.zapmask()))
            return n
        lt.sk.transform = spy
    for blk in _blocks(o):
        lt.process_block(blk)
    if lt.ndat_total:
        lt.finish_subint()
    lt.synchronize()
    subs = [dict(hits=s["hits"].copy(), integration_length=s["integration_length"], ndat_total=s["ndat_total"],
                 profile=s["profile_dev"].cpu().numpy()) for s in lt.subints]
    out = dict(subs=subs, cleaned=cleaned, ndat_out=lt.ndat_out, stats=lt.sk.get_statistics() if cfg.sk_zap else None,
               sk_statistics=lt.sk_statistics, scale=lt.scalefac, npol_out=lt.npol_out, out_start=lt.out_start, cfg=cfg)
    lt.close()
    return out


@pytest.fixture(scope="module")
def driven(obs):
    return _drive(obs, subint_seconds=obs["L"])


def _by_hand(o, length):
    """perform_raw -> SpectralKurtosisEngine.transform (in place) -> detect_polarimetry -> fold_zeroed, with the carry, the pieces of
    -L and the books kept here.  Also returns the voltages before cleaning, for the restatement."""
    import torch
    from dspsr_amd import pipeline
    cfg = _config(pipeline, parts_per_block=o["ppb"], subint_seconds=length)
    front = pipeline.LoadToFold(cfg, _info(pipeline), stream=torch.cuda.current_stream().cuda_stream)     # its filterbank and ephemeris
    ctx, nkeep, rate = front.ctx, o["nkeep"], o["rate"]
    sk = dspsr_amd.SpectralKurtosisEngine(ctx)
    sk.set_shape(NCHAN, 2, M)
    sk.set_options(3, 0, 0, False, False, False)
    fold = dspsr_amd.FoldEngine(ctx)
    fold.set_shape(NCHAN, 1, 4, NBIN)
    det_eng = dspsr_amd.DetectionEngine(ctx)
    ndat, head = o["ppb"] * nkeep, M - 1
    volt = torch.zeros((NCHAN, 2, 2 * (head + ndat)), dtype=torch.float32, device="cuda")
    det = torch.zeros((NCHAN, 1, 4 * (head + ndat)), dtype=torch.float32, device="cuda")
    hits_dev = torch.zeros((NCHAN, NBIN), dtype=torch.int32, device="cuda")
    tail, ndat_out, ndat_total, subs, before = 0, 0, 0, [], []

    def finish():
        nonlocal ndat_total
        hits = hits_dev.cpu().numpy().view(np.uint32)
        subs.append(dict(hits=hits, integration_length=float(int(hits.sum(dtype=np.uint64))) / (rate * NCHAN), ndat_total=ndat_total,
                         profile=fold.synch().reshape(-1)))
        fold.zero()
        hits_dev.zero_()
        ndat_total = 0
    for blk in _blocks(o):
        front.fb.perform_raw(blk, front.layout, front.scale8, volt[:, :, 2 * head:], o["ppb"])
        rows = volt[:, :, 2 * (head - tail):]
        nuse = (tail + ndat) // M * M
        before.append(rows[:, :, :2 * nuse].cpu().numpy())
        assert sk.transform(rows, rows, tail + ndat) == nuse
        det_eng.polarimetry(4, rows[:, :, :2 * nuse], det[:, :, :4 * nuse], _lib.COHERENCE)
        for idat_start, ndat_fold, _division, complete in pipeline.subint_pieces(ndat_out, nuse, length, rate):
            phi, pfold = front._phase(front.out_start + (ndat_out + idat_start + 0.5) / rate)
            fold.set_nbin(NBIN)
            fold.set_ndat(ndat_fold, idat_start)
            fold.set_bins(phi, (1.0 / rate) / pfold, ndat_fold, idat_start, None)
            fold.fold_zeroed(det[:, :, :4 * nuse], hits_dev)
            ndat_total += ndat_fold
            if complete:
                finish()
        keep = tail + ndat - nuse
        carried = rows[:, :, 2 * nuse:2 * (nuse + keep)].clone()
        volt[:, :, 2 * (head - keep):2 * head] = carried
        tail, ndat_out = keep, ndat_out + nuse
    if ndat_total:
        finish()
    stats = sk.get_statistics()
    for e in (sk, fold):
        e.close()
    front.close()
    return subs, stats, before, ndat_out


def test_driver_is_the_engines_by_hand_bit_for_bit(obs, driven):
    subs, stats, before, ndat_out = _by_hand(obs, obs["L"])
    assert len(driven["subs"]) == len(subs) >= 2 and driven["ndat_out"] == ndat_out
    assert 0 < NBLOCK * obs["ppb"] * obs["nkeep"] - ndat_out < M            # the last < M samples of the run are dropped
    for d, h in zip(driven["subs"], subs):
        assert d["hits"].shape == (NCHAN, NBIN) and d["hits"].dtype == np.uint32 and np.array_equal(d["hits"], h["hits"])
        assert d["integration_length"] == h["integration_length"] and d["ndat_total"] == h["ndat_total"]
        assert np.isfinite(d["profile"]).all() and np.array_equal(d["profile"].view(np.uint32), h["profile"].view(np.uint32))
    assert sum(d["ndat_total"] for d in driven["subs"]) == ndat_out
    assert ref.same_statistics(driven["stats"], stats) and ref.same_statistics(driven["sk_statistics"], stats)
    assert driven["stats"]["npart_total"] == ndat_out // M * NCHAN and driven["stats"]["unfiltered_hits"] == ndat_out // M
    # the cleaned rows: the voltages where the mask is 0, +0.0 where it is 1
    for (clean, mask), volt in zip(driven["cleaned"], before):
        npart = mask.shape[0]
        assert clean.shape == volt.shape == (NCHAN, 2, 2 * npart * M)
        want = ref.mask_rows(volt, mask, M)
        assert np.array_equal(clean.view(np.uint32), want.view(np.uint32))


def test_the_burst_channel_is_zapped_and_the_others_are_not(obs, driven):
    """A condition, not a measurement: on the restatement, run on the CPU from the device's voltages, the burst channel is zapped in
    >= 90 % of its parts and every other channel in <= 2 %.  The host half comes first: the restatement alone meets it for this seed."""
    _, _, before, _ = _by_hand(obs, obs["L"])
    zapped, nparts, masks = np.zeros(NCHAN), 0, []
    for volt in before:
        est, est_tscr = ref.compute(volt, M)
        npart = est.shape[0]
        det = ref.Detector(NCHAN, 2, M)
        m_t = int(np.float32(M * npart))
        masks.append(det.detect(est, est_tscr, dspsr_amd.sk_limits(M, 3), dspsr_amd.sk_limits(m_t, 3)).copy())
        zapped += masks[-1].sum(axis=0)
        nparts += npart
    frac = zapped / nparts
    burst = int(np.argmax(frac))
    print("zapped fraction per channel:", np.round(frac, 4))
    assert frac[burst] >= 0.90 and np.delete(frac, burst).max() <= 0.02
    # the device: the same channel, hence no hits from it, and the other channels keep theirs
    dev = np.concatenate([mask for _, mask in driven["cleaned"]])
    dfrac = dev.mean(axis=0)
    assert int(np.argmax(dfrac)) == burst and dfrac[burst] >= 0.90 and np.delete(dfrac, burst).max() <= 0.02
    hits = sum(d["hits"].astype(np.int64) for d in driven["subs"])
    for ch in range(NCHAN):
        assert hits[ch].sum() == (dev[:, ch] == 0).sum() * M, ch            # no detected sample of a kept part is exactly zero


def _snr(profile, hits, burst=None):
    """the pulse of the summed total-intensity profile over the scatter of its off-pulse bins; per-channel hits normalise"""
    prof = profile.reshape(NCHAN, 1, NBIN, 4)[:, 0, :, 0] + profile.reshape(NCHAN, 1, NBIN, 4)[:, 0, :, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = np.where(hits > 0, prof / hits, 0.0)
    chans = [c for c in range(NCHAN) if norm[c].any()]
    p = norm[chans].sum(axis=0)
    peak = int(np.argmax(np.convolve(np.r_[p, p], np.ones(5), "same")[:NBIN]))
    onp = [(peak + k) % NBIN for k in range(-3, 4)]
    off = np.delete(p, onp)
    return (p[onp].mean() - off.mean()) / off.std()


def test_the_pulse_is_not_weaker_with_skz_and_off_means_the_old_path(obs):
    import torch
    from dspsr_amd import pipeline
    with_sk = _drive(obs)
    without = _drive(obs, sk_zap=False)
    assert len(with_sk["subs"]) == len(without["subs"]) == 1
    s, w = with_sk["subs"][0], without["subs"][0]
    assert w["hits"].shape == (NBIN,) and s["hits"].shape == (NCHAN, NBIN)
    snr_sk = _snr(s["profile"].astype(np.float64), s["hits"].astype(np.float64))
    snr_no = _snr(w["profile"].astype(np.float64), np.broadcast_to(w["hits"].astype(np.float64), (NCHAN, NBIN)))
    print("pulse S/N with -skz %.2f, without %.2f" % (snr_sk, snr_no))
    assert snr_sk >= snr_no > 0
    # sk_zap=False is the path as it was: the same bits as a run whose Config never heard of the feature
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, ndim=4, parts_per_block=obs["ppb"],
                          max_parts=2)
    lt = pipeline.LoadToFold(cfg, _info(pipeline), stream=torch.cuda.current_stream().cuda_stream)
    assert lt.sk is None and lt.sk_statistics is None and lt.voltages is None
    for blk in _blocks(obs):
        lt.process_block(blk)
    lt.finish_subint()
    old = lt.subints[0]
    assert np.array_equal(old["hits"], w["hits"]) and old["integration_length"] == w["integration_length"]
    assert np.array_equal(old["profile_dev"].cpu().numpy().view(np.uint32), w["profile"].view(np.uint32))
    lt.close()


def test_refusals_at_plan_time_by_name():
    from dspsr_amd import pipeline
    info = _info(pipeline)
    for over, kwargs, text in (
            (dict(cyclic_nchan=16, cyclic_mover=2, cyclic_npol=2, nbin=32), {}, r"-skz\) is not built with cyclic_nchan \(-cyclic\)"),
            (dict(plfb_nbin=8, nchan=8, folding_period=0.0004, plfb_nchan=64), {}, r"-skz\) is not built with plfb_nbin \(-G\)"),
            (dict(fourth_moment=True), {}, r"-skz\) is not built with fourth_moment \(-4\)"),
            (dict(interchan_dedispersion=True), {}, r"-skz\) is not built with interchan_dedispersion \(-K\)"),
            (dict(folding_period=0.0), dict(targets=[pipeline.FoldTarget("a", folding_period=0.004), pipeline.FoldTarget("b", folding_period=0.003)]),
             r"-skz\) folds one pulsar; 2 targets given"),
            (dict(convolve_when="after"), {}, r"-skz\) is built for -F N:D"),
            ({}, dict(dump_before=("Fold",)), r"-skz\) is not built with the dump taps"),
            (dict(sk_m=31), {}, r"sk_m=31 outside \[32, 65536\]"), (dict(sk_m=65537), {}, r"sk_m=65537 outside \[32, 65536\]"),
            (dict(sk_std_devs=0), {}, "sk_std_devs == 0"),
            (dict(sk_chan_start=9, sk_chan_end=9), {}, "sk_chan_start=9 >= sk_chan_end=9")):
        with pytest.raises(dspsr_amd.DspsrAmdError, match=text):
            pipeline.LoadToFold(_config(pipeline, **over), info, **kwargs)
    with pytest.raises(dspsr_amd.DspsrAmdError, match=r"-skz\) is not built for sub-band sharded runs"):
        pipeline.LoadToFold(_config(pipeline, nchan=32), pipeline.InputInfo(centre_frequency=FREQ, bandwidth=BW, tsamp_us=2 * TSAMP, nchan=2,
                                                                            ndim=2, machine="DADA"), subband=1)
    # a refusal the run had without -skz still wins
    with pytest.raises(dspsr_amd.DspsrAmdError, match="convolve_when='x' is not one of"):
        pipeline.LoadToFold(_config(pipeline, convolve_when="x"), info)


def test_the_tool_writes_files_with_per_channel_hits(obs, tmp_path):
    """tools/dspsr_amd_fold.py -skz: HITS_NCHAN files that read_phase_series and the C++ reader give back; the reference's Zapped line;
    the options the reference has and this path does not are refused by argparse."""
    from dspsr_amd import pipeline, synth
    path = tmp_path / "synthetic.dada"
    path.write_bytes(synth.dada_header(FREQ, BW, 1, 2, 1, TSAMP) + obs["raw"].cpu().numpy().tobytes())
    tool = [sys.executable, os.path.join(ROOT, "tools", "dspsr_amd_fold.py"), "-F", "16:D", "-D", str(DM), "-b", str(NBIN), "-c", str(PERIOD)]
    p = subprocess.run(tool + ["-skz", "-skzm", str(M), "-L", repr(obs["L"]), "-O", str(tmp_path / "sk"), str(path)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stderr.splitlines() if ln.startswith("Zapped:")]
    assert len(line) == 1 and all(k in line[0] for k in (" total=", "% skfb=", "% tscr=", "% fscr="))
    files = sorted(f for f in os.listdir(tmp_path) if f.startswith("sk_") and f.endswith(".ps"))
    assert len(files) >= 2
    src = tmp_path / "reader.cpp"
    src.write_text('#include "dspsr_amd_phase_series_io.h"\n#include <stdio.h>\nint main (int argc, char** argv) {\n'
                   '  HIP::PhaseSeriesFile f = HIP::read_phase_series_file (argv[1]);\n  unsigned long long sum = 0;\n'
                   '  for (size_t i = 0; i < f.hits.size (); i++) sum += f.hits[i];\n'
                   '  printf ("%u %u %zu %llu %u %.9g\\n", f.hits_nchan, f.nbin, f.hits.size (), sum, f.hits[f.hits.size () - 1], (double) f.sums[f.sums.size () - 1]);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "reader"
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "dspsr_amd", "host"), str(src), "-o", str(exe)], check=True)
    for f in files:
        hdr, hits, prof = pipeline.read_phase_series(str(tmp_path / f))
        assert hdr["HITS_NCHAN"] == str(NCHAN) and hits.shape == (NCHAN, NBIN) and prof.shape == (NCHAN, 1, NBIN, 4)
        assert float(hdr["INTEGRATION_LENGTH"]) == float(int(hits.sum(dtype=np.uint64))) / (obs["rate"] * NCHAN)
        got = subprocess.run([str(exe), str(tmp_path / f)], capture_output=True, text=True, check=True).stdout.split()
        assert [int(v) for v in got[:5]] == [NCHAN, NBIN, NCHAN * NBIN, int(hits.sum()), int(hits[-1, -1])]
        assert np.float32(float(got[5])) == prof.reshape(-1)[-1]
    # one-dimensional hits: header and body are what they always were
    sub = dict(hits=np.arange(NBIN, dtype=np.uint32), integration_length=1.0, ndat_total=5, profile=np.zeros((NCHAN, 1, NBIN, 4), np.float32))
    pipeline.write_phase_series(str(tmp_path / "plain.ps"), sub, _info(pipeline), _config(pipeline), npol=1)
    blob = (tmp_path / "plain.ps").read_bytes()
    assert b"HITS_NCHAN" not in blob and len(blob) == 4096 + 4 * NBIN + 4 * NCHAN * NBIN * 4
    hdr, hits, _ = pipeline.read_phase_series(str(tmp_path / "plain.ps"))
    assert "HITS_NCHAN" not in hdr and np.array_equal(hits, sub["hits"])
    for opt in (["-noskz_too"], ["-sk_fold"], ["-skzn", "2"]):
        p = subprocess.run(tool + ["-skz"] + opt + [str(path)], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and ("unrecognized arguments" in p.stderr or "ignored explicit argument" in p.stderr
                                      or "expected" in p.stderr), p.stderr[-500:]
