"""LoadToFold with cyclic_nchan on a synthetic dispersed pulsar, against oracle filterbank -> float64 restatement -> Synch."""
import math

import numpy as np
import pytest

import cyclic_reference as cr
import dspsr_amd
from dspsr_amd import pipeline, synth

pytestmark = pytest.mark.gpu

FREQ, BW, TSAMP, DM, PERIOD, NCHAN, NBIN = 1382.0, -16.0, 1.0 / 32.0, 30.0, 0.004, 16, 32


def _run(oracle, npol, mover, npol_out, subint_seconds, max_parts=32, parts=6):
    import torch
    o = oracle
    obs = o.Observation(centre_frequency=FREQ, bandwidth=BW, tsamp_us=TSAMP, dispersion_measure=DM, npol=npol)
    resp = o.Dedispersion().match(obs, NCHAN)
    plan = o.filterbank_plan(obs, NCHAN, resp)
    raw = synth.voltages(parts * plan.nsamp_step + plan.nsamp_overlap, FREQ, BW, TSAMP, DM, PERIOD, npol=npol)
    info = pipeline.InputInfo(centre_frequency=FREQ, bandwidth=BW, npol=npol, ndim=1, tsamp_us=TSAMP, machine="DADA", mjd_sec=0.0)
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, parts_per_block=parts,
                          max_parts=max_parts, subint_seconds=subint_seconds, cyclic_nchan=16, cyclic_mover=mover, cyclic_npol=npol_out)
    lt = pipeline.LoadToFold(cfg, info, stream=torch.cuda.current_stream().cuda_stream)
    lt.process_block(torch.from_numpy(raw).cuda())
    lt.finish_subint()
    subs = lt.subints
    geo = (lt.nkeep, lt.out_rate, lt.out_start)
    lt.close()
    fb = o.filterbank(o.unpack_8bit(raw, obs), plan, dspsr_amd.Dedispersion(FREQ, BW, DM).match(NCHAN).kernel, dtype=np.float64)
    return cfg, subs, fb, geo, plan


@pytest.mark.parametrize("npol,mover,npol_out,subint", [(2, 1, 4, 0.0), (2, 4, 2, 0.0), (1, 1, 1, 0.0), (2, 1, 1, 0.00045)],
                         ids=["pol4", "mover4-pol2", "onepol", "subint-boundary"])
def test_cyclic_pipeline_against_the_oracle(oracle, npol, mover, npol_out, subint):
    cfg, subs, fb, (nkeep, rate, start), plan = _run(oracle, npol, mover, npol_out, subint)
    g = pipeline.cyclic_geometry(cfg, pipeline.InputInfo(npol=npol))
    ndat = fb.shape[2]
    pieces = pipeline.subint_pieces(0, ndat, subint, rate) if subint > 0 else [(0, ndat, 0, False)]
    if subint > 0:
        assert len(pieces) > 1 and len(subs) >= 2, "the block must hold a sub-integration boundary"
    # the float64 chain, piece by piece, a new lag array after every completed sub-integration
    want, lags, hits = [], None, np.zeros(NBIN, np.uint32)
    for i0, n, _div, complete in pieces:
        t0 = start + (i0 + 0.5) / rate
        phi = math.fmod(t0, PERIOD) / PERIOD
        p0, p1, h = cr.plans(phi, (1.0 / rate) / PERIOD, NBIN, n)
        lags = cr.fold(fb[:, :, i0:i0 + n], p0, p1, g["nlag"], g["npol"], NBIN, lags)
        hits += h
        if complete:
            want.append((cr.synch(lags, mover), hits.copy()))
            lags, hits = None, np.zeros(NBIN, np.uint32)
    if lags is not None:
        want.append((cr.synch(lags, mover), hits.copy()))
    assert len(subs) == len(want)
    # Tolerance, composed.  Filterbank (tests/test_gpu_parity.py): max error of a voltage 8 * 2e-6 * sqrt(log2 N) of rms(out).  A lag
    # product has two voltage factors: 2 * that, relative to rms^2, which the zero lag -- the largest value of an auto lag function --
    # sums coherently; the fold adds the bound of tests/test_gpu_cyclic.py (floor 4 * 2^-24, the strict-order float32 error of sums
    # this short is below it) and Synch (log2(n) + 1) * 2^-23 (tests/test_cyclic_host.py).  All three are relative to the largest
    # value, and the transform is linear, so they add.  Cross products are bounded by sqrt(PP QQ) (Cauchy-Schwarz): their scale
    # is the geometric mean of the two auto maxima of the channel.
    n = g["nchan_spec"]
    tol = 2 * 8 * 2e-6 * math.sqrt(math.log2(2 * plan.nchan_subband * plan.freq_res)) + 4 * 2.0 ** -24 + (math.log2(n) + 1) * 2.0 ** -23
    per = g["nchan_per_channel"]
    for sub, (ref, rhits) in zip(subs, want):
        assert np.array_equal(sub["hits"], rhits), "hits differ"
        got = sub["profile"][..., 0].astype(np.float64).reshape(NCHAN, per, g["npol"], NBIN)
        ref = ref.reshape(NCHAN, per, g["npol"], NBIN)
        peak = np.abs(ref).max(axis=(1, 3))                               # [chan][pol]
        scale = peak.copy()
        if g["npol"] == 4:
            scale[:, 2:] = np.sqrt(peak[:, 0] * peak[:, 1])[:, None]
        err = np.abs(got - ref).max(axis=(1, 3)) / scale
        assert err.max() <= tol, "error %.3g > %.3g" % (err.max(), tol)
        assert peak.min() > 0


def test_block_cut_gives_the_same_bits(oracle):
    """the same pieces through a different max_parts (another cut of the filterbank's launch groups): identical spectra"""
    a = _run(oracle, 2, 1, 4, 0.0, max_parts=32)[1]
    b = _run(oracle, 2, 1, 4, 0.0, max_parts=2)[1]
    assert np.array_equal(a[0]["profile"].view(np.uint32), b[0]["profile"].view(np.uint32)) and np.array_equal(a[0]["hits"], b[0]["hits"])


def test_tool_writes_a_readable_file(oracle, tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool_gpu_cyclic", os.path.join(root, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    o = oracle
    obs = o.Observation(centre_frequency=FREQ, bandwidth=BW, tsamp_us=TSAMP, dispersion_measure=DM)
    plan = o.filterbank_plan(obs, NCHAN, o.Dedispersion().match(obs, NCHAN))
    raw = synth.voltages(4 * plan.nsamp_step + plan.nsamp_overlap, FREQ, BW, TSAMP, DM, PERIOD)
    path = tmp_path / "in.dada"
    path.write_bytes(synth.dada_header(FREQ, BW, 1, 2, 1, TSAMP, extra={"DM": DM}) + raw.tobytes())
    prefix = str(tmp_path / "out")
    tool.main(["-F", "%d:D" % NCHAN, "-cyclic", "16", "-cyclicoversample", "2", "-d", "2", "-b", str(NBIN), "-c", str(PERIOD), "-O", prefix,
               str(path)])
    hdr, hits, prof = pipeline.read_phase_series(prefix + "_0000.ps")
    assert (int(hdr["NCHAN"]), int(hdr["NPOL"]), int(hdr["NDIM"]), hdr["STATE"]) == (NCHAN * 16, 2, 1, "PPQQ")
    assert not os.path.exists(prefix + "_0001.ps")
    # the same Config on the same bytes through the pipeline: the file holds exactly that sub-integration
    import torch
    from dspsr_amd import dada
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, ndim=1, cyclic_nchan=16,
                          cyclic_mover=2, cyclic_npol=2)
    lt = dada.fold_file(str(path), cfg, stream=torch.cuda.current_stream().cuda_stream)
    assert len(lt.subints) == 1
    sub = lt.subints[0]
    assert hits.sum() == sub["ndat_total"] > 0
    assert np.array_equal(hits, sub["hits"])
    assert prof.shape == sub["profile"].shape == (NCHAN * 16, 2, NBIN, 1) and prof.any()
    assert np.array_equal(prof.view(np.uint32), np.ascontiguousarray(sub["profile"]).view(np.uint32))
    assert float(hdr["INTEGRATION_LENGTH"]) == sub["integration_length"] and float(hdr["SCALE"]) == lt.scalefac
    # a second finish with nothing folded emits nothing; a communicator is refused on a cyclic run
    lt.finish_subint()
    assert len(lt.subints) == 1
    with pytest.raises(dspsr_amd.DspsrAmdError, match="multi-GPU"):
        lt.set_communicator(None, 0, 2)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="multi-GPU"):
        lt.set_rccl_communicator(object())
    lt.close()
