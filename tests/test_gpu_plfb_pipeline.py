"""LoadToFold with plfb_nbin (dspsr -G) on a synthetic DADA stream: -F 8:D, -G 8, a period that gives 64 channels per window,
several blocks.  hits / ndat_total / integration_length against the sample-walking restatement of the divider, the profile
against the oracle filterbank's rows pushed through the float64 loop (tests/plfb_reference.py), block sizes against each
other, and the tool's file against the pipeline's sub-integration."""
import importlib.util
import os

import numpy as np
import pytest

import plfb_reference as pr
import dspsr_amd
from dspsr_amd import dada, pipeline, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQ, BW, TSAMP, DM, PERIOD, NCHAN, NBIN, PARTS = 1382.0, -16.0, 1.0 / 32.0, 3.0, 0.0004, 8, 8, 12
NFFT = 64


def _info():
    return pipeline.InputInfo(centre_frequency=FREQ, bandwidth=BW, npol=2, ndim=1, tsamp_us=TSAMP, machine="DADA", mjd_sec=0.0)


def _cfg(parts_per_block, **kw):
    return pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=64, folding_period=PERIOD, parts_per_block=parts_per_block,
                           plfb_nbin=NBIN, **kw)


@pytest.fixture(scope="module")
def stream(oracle):
    """raw bytes, the oracle's float64 rows [chan][pol][2 ndat], the float32 oracle's rows, the plan"""
    o = oracle
    obs = o.Observation(centre_frequency=FREQ, bandwidth=BW, tsamp_us=TSAMP, dispersion_measure=DM)
    plan = o.filterbank_plan(obs, NCHAN, o.Dedispersion().match(obs, NCHAN))
    raw = synth.voltages(PARTS * plan.nsamp_step + plan.nsamp_overlap, FREQ, BW, TSAMP, DM, PERIOD)
    kernel = dspsr_amd.Dedispersion(FREQ, BW, DM).match(NCHAN).kernel
    unpacked = o.unpack_8bit(raw, obs)

    def rows(dtype):
        fb = o.filterbank(unpacked, plan, kernel, dtype=dtype)
        return np.ascontiguousarray(np.stack([fb.real, fb.imag], axis=-1)).reshape(fb.shape[0], fb.shape[1], -1)
    return raw, rows(np.float64), rows(np.float32), plan


def _feed(lt, raw, plan, parts_per_block):
    import torch
    dev = torch.from_numpy(raw.reshape(-1)).cuda()
    unit = 2                                                # bytes per time sample: 2 polarisations, real
    for first in range(0, PARTS, parts_per_block):
        n = min(parts_per_block, PARTS - first)
        lo = first * plan.nsamp_step * unit
        lt.process_block(dev[lo:lo + (n * plan.nsamp_step + plan.nsamp_overlap) * unit], n)
    lt.finish_subint()
    lt.synchronize()


def _run(raw, plan, parts_per_block, inject=None, **kw):
    import torch
    lt = pipeline.LoadToFold(_cfg(parts_per_block, **kw), _info(), stream=torch.cuda.current_stream().cuda_stream)
    if inject is not None:                                  # exact rows in place of the filterbank's
        rows = torch.from_numpy(inject).cuda()

        def perform_raw(_raw, _layout, _scale, out, npart):
            n = npart * lt.nkeep
            out[:, :, :2 * n].copy_(rows[:, :, 2 * lt.ndat_out:2 * (lt.ndat_out + n)])
        lt.fb.perform_raw = perform_raw
    _feed(lt, raw, plan, parts_per_block)
    subs, geo = lt.subints, (lt.nkeep, lt.out_rate, lt.out_start, lt.scalefac, dict(lt.plfb_geometry))
    lt.close()
    return subs, geo


def _windows(rate, start, ndat):
    phase = lambda t: (int(np.floor(t / PERIOD)), t / PERIOD - np.floor(t / PERIOD))
    iphase = lambda ph, guess: (ph[0] + ph[1]) * PERIOD
    return pr.divider_windows(phase, iphase, start, rate, NBIN, 0.0, ndat, NFFT)


def _error(got, ref):
    return np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()


def test_route_against_the_restatement_and_the_oracle(stream):
    raw, rows64, rows32, plan = stream
    subs, (nkeep, rate, start, scalefac, g) = _run(raw, plan, 4)
    assert len(subs) == 1 and PARTS // 4 >= 3
    sub = subs[0]
    assert g["nchan_fft"] == NFFT == pipeline.plfb_choose_nchan(PERIOD, rate, NBIN)            # plfb_nchan = 0: the reference's choice
    ndat = PARTS * nkeep
    assert rows64.shape == (NCHAN, 2, 2 * ndat)
    wins = _windows(rate, start, ndat)
    hits, total, length = pr.window_totals(wins, NBIN, NFFT, rate)
    assert total >= 3 * NBIN
    assert np.array_equal(sub["hits"], hits) and sub["ndat_total"] == total and sub["integration_length"] == length
    assert (sub["state"], sub["rate"], sub["nsub_swap"], sub["scale"]) == ("Coherence", rate / NFFT, NCHAN, scalefac * NFFT)
    assert sub["profile"].shape == (NCHAN * NFFT, 4, NBIN, 1)
    starts, bins = [w[0] for w in wins], [w[1] for w in wins]
    ref = pr.plfb_loop(rows64, 2, NFFT, 4, NBIN, starts, bins, np.float64)
    f32 = pr.plfb_loop(rows32, 2, NFFT, 4, NBIN, starts, bins, np.float32)
    e_gpu, e_f32 = _error(sub["profile"][..., 0], ref), _error(f32, ref)
    print("plfb route e_gpu=%.3e e_f32=%.3e ratio=%.2f" % (e_gpu, e_f32, e_gpu / e_f32))
    assert e_gpu <= 4 * e_f32, "e_gpu %.3e > 4 x e_f32 %.3e" % (e_gpu, e_f32)
    # another block size: the same windows, the sums to the same bound
    subs1, _ = _run(raw, plan, 1)
    one = subs1[0]
    assert np.array_equal(one["hits"], hits) and one["ndat_total"] == total and one["integration_length"] == length
    e_one = _error(one["profile"][..., 0], ref)
    print("plfb route parts_per_block=1 e_gpu=%.3e" % e_one)
    assert e_one <= 4 * e_f32
    # output polarisations from Config.npol
    subs2, (_, _, _, _, g2) = _run(raw, plan, 4, npol=1)
    assert g2["state"] == "Intensity" and subs2[0]["profile"].shape == (NCHAN * NFFT, 1, NBIN, 1)
    ref1 = pr.plfb_loop(rows64, 2, NFFT, 1, NBIN, starts, bins, np.float64)
    f32_1 = pr.plfb_loop(rows32, 2, NFFT, 1, NBIN, starts, bins, np.float32)
    e_gpu1, e_f32_1 = _error(subs2[0]["profile"][..., 0], ref1), _error(f32_1, ref1)
    print("plfb route npol=1 e_gpu=%.3e e_f32=%.3e" % (e_gpu1, e_f32_1))
    assert e_gpu1 <= 4 * e_f32_1


def test_block_size_gives_the_same_bits_on_exact_rows(stream):
    """exact rows injected in place of the filterbank's: windows that span two blocks, blocks shorter than a window's carry"""
    raw, rows64, _rows32, plan = stream
    rng = np.random.default_rng(11)
    ndat = rows64.shape[2] // 2
    amp = rng.integers(1, 4, (NCHAN, 2, 1, 2)).astype(np.float32)
    tone = np.where(np.arange(ndat) % 2 == 0, 1.0, -1.0).astype(np.float32)
    exact = np.ascontiguousarray((amp * tone[None, None, :, None]).reshape(NCHAN, 2, 2 * ndat))
    got = {}
    for ppb in (1, 4):
        subs, (nkeep, rate, start, _, _) = _run(raw, plan, ppb, inject=exact)
        got[ppb] = subs[0]
    wins = _windows(rate, start, ndat)
    assert any(s // (nkeep) != (s + NFFT - 1) // nkeep for s, _ in wins)                       # a window spans two blocks
    ref = pr.plfb_loop(exact, 2, NFFT, 4, NBIN, [w[0] for w in wins], [w[1] for w in wins], np.float64)
    units = ref / float(NFFT * NFFT)
    assert np.array_equal(units, np.round(units)) and np.abs(units).max() < 2 ** 24
    for ppb in (1, 4):
        assert np.array_equal(got[ppb]["profile"][..., 0].view(np.uint32), ref.astype(np.float32).view(np.uint32)), ppb
        assert np.array_equal(got[ppb]["hits"], got[1]["hits"])


def test_tool_writes_the_pipelines_subint(stream, tmp_path):
    import torch
    raw, _rows64, _rows32, _plan = stream
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool_gpu_plfb", os.path.join(ROOT, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = tmp_path / "in.dada"
    path.write_bytes(synth.dada_header(FREQ, BW, 1, 2, 1, TSAMP, extra={"DM": DM}) + raw.tobytes())
    prefix = str(tmp_path / "out")
    tool.main(["-F", "%d:D" % NCHAN, "-G", str(NBIN), "-d", "2", "-c", str(PERIOD), "-O", prefix, str(path)])
    hdr, hits, prof = pipeline.read_phase_series(prefix + "_0000.ps")
    assert not os.path.exists(prefix + "_0001.ps")
    assert (int(hdr["NCHAN"]), int(hdr["NPOL"]), int(hdr["NDIM"]), int(hdr["NBIN"]), hdr["STATE"]) == (NCHAN * NFFT, 2, 1, NBIN, "PPQQ")
    lt = dada.fold_file(str(path), pipeline.Config(nchan=NCHAN, dispersion_measure=DM, folding_period=PERIOD, ndim=1, plfb_nbin=NBIN,
                                                   npol=2), stream=torch.cuda.current_stream().cuda_stream)
    assert len(lt.subints) == 1
    sub = lt.subints[0]
    assert np.array_equal(hits, sub["hits"]) and hits.sum() == sub["ndat_total"] == int(hdr["NDAT_TOTAL"]) > 0
    assert np.array_equal(prof.view(np.uint32), np.ascontiguousarray(sub["profile"]).view(np.uint32)) and prof.any()
    assert float(hdr["INTEGRATION_LENGTH"]) == sub["integration_length"] and float(hdr["SCALE"]) == sub["scale"] == lt.scalefac * NFFT
    assert float(hdr["RATE"]) == sub["rate"] == lt.out_rate / NFFT and int(hdr["NSUB_SWAP"]) == NCHAN
    lt.finish_subint()                                      # nothing accumulated since: nothing emitted
    assert len(lt.subints) == 1
    with pytest.raises(dspsr_amd.DspsrAmdError, match="multi-GPU"):
        lt.set_communicator(None, 0, 2)
    lt.close()
