"""MeerKAT beamformer files (INSTRUMENT MKBF / MKBFRo) through the fold pipeline: a synthetic dispersed pulse in 4 channels, reordered
to heaps and written as a DADA file, folded with dada.fold_file -- the one-pass convolution reading the heaps itself, against the
same run with the engine unpacking first (bit for bit) and against the float64 oracle chain (unpack, convolution, detect, fold);
with -x 16384, where the engine always unpacks and the three-pass convolution runs; and as a sub-band run on one channel's runs."""
import numpy as np
import pytest

import heap_cases as hc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FREQ, BW, NCHAN, TSAMP, DM, PERIOD, NBIN = 1382.0, -16.0, 4, 0.25, 10.0, 0.004, 64
NBLOCKS = 3


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    return dspsr_amd


def _response(o, M):
    obs = o.Observation(centre_frequency=FREQ, bandwidth=BW, nchan=NCHAN, npol=2, ndim=2, tsamp_us=TSAMP, dispersion_measure=DM)
    r = o.Dedispersion()
    r.set_frequency_resolution(M)
    r.match(obs, NCHAN)
    return obs, r


_made = {}


def _observation(o, tmp_path_factory, M, ppb):
    """(paths per machine, TFP bytes, oracle fold) of the M-point case, made once"""
    if M in _made:
        return _made[M]
    from dspsr_amd import dada, synth
    obs, r = _response(o, M)
    step, ovl = M - r.impulse_pos - r.impulse_neg, r.impulse_pos + r.impulse_neg
    ndat = NBLOCKS * ppb * step + ovl
    ndat += (-ndat) % hc.HEAP                                    # whole heaps
    tfp = synth.voltages(ndat, FREQ, BW, TSAMP, DM, PERIOD, npol=2, ndim=2, nchan=NCHAN).reshape(ndat, NCHAN, 2, 2)
    d = tmp_path_factory.mktemp("mkbf%d" % M)
    paths = {}
    for machine, swap in hc.MACHINES.items():
        block = hc.heaps_from_stream(np.ascontiguousarray(tfp.transpose(1, 2, 0, 3)), swap) if M == 1024 else dada.heaps_from_tfp(tfp, swap)
        paths[machine] = hc.write_dada(d / ("%s.dada" % machine), block, machine=machine, nchan=NCHAN, npol=2, freq=FREQ, bw=BW, tsamp_us=TSAMP)
    # the oracle chain in float64: unpack, convolution of every channel, detection, fold block by block
    plan = o.filterbank_plan(obs, NCHAN, r)
    assert (plan.nchan_subband, plan.nsamp_step, plan.nsamp_overlap) == (1, step, ovl)
    x = o.unpack_8bit(tfp.reshape(-1), obs)
    npart = NBLOCKS * ppb
    cv = o.convolution(x, r.ndat, r.impulse_pos, r.impulse_neg, r.buffer, False, npart=npart, dtype=np.float64)
    fobs = o.filterbank_output_observation(obs, plan)
    det = o.detect_layout(o.detect_products(cv, "Coherence"), 4)
    ps = o.PhaseSeries(NCHAN, 1, 4, NBIN, data=np.zeros((NCHAN, 1, NBIN, 4), np.float64))
    fcfg = o.FoldConfig(nbin=NBIN, folding_period=PERIOD)
    per_block = ppb * plan.nkeep
    for b in range(NBLOCKS):
        o.fold(det, fobs, fcfg, ps, idat_start=b * per_block, ndat_fold=per_block)
    _made[M] = (paths, r, step, ovl, ps, fobs)
    return _made[M]


def _fold(gpu, path, M, ppb, **kw):
    from dspsr_amd import dada, pipeline
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, freq_res=M, ndim=4, parts_per_block=ppb,
                          max_parts=2, **kw)
    return dada.fold_file(path, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("machine", sorted(hc.MACHINES))
def test_fold_file_of_heaps(oracle, gpu, tmp_path_factory, machine):
    from dspsr_amd import dada
    M, ppb = 1024, 3
    paths, r, step, ovl, ps, fobs = _observation(oracle, tmp_path_factory, M, ppb)
    assert (ppb * step) % 256 != 0 and (2 * ppb * step) % 256 != 0          # the second and third blocks start inside a heap
    lt = _fold(gpu, paths[machine], M, ppb)
    assert lt.info.machine == machine and lt.fb.takes_heaps() and lt.fb.fuse_heaps
    assert np.abs(r.buffer - lt.response.kernel).max() <= 1.2e-7 and (r.impulse_pos, r.impulse_neg) == (lt.response.impulse_pos, lt.response.impulse_neg)
    assert (lt.nsamp_step, lt.nsamp_overlap) == (step, ovl)
    firsts = [first for _v, _n, first in dada.DadaFile(paths[machine]).blocks(lt)]
    assert len(firsts) == NBLOCKS and firsts[0] == 0 and firsts[1] and firsts[2]
    sub = lt.subints[0]
    hits, prof = sub["hits"].copy(), sub["profile_dev"].cpu().numpy().copy()
    assert abs(lt.out_rate - fobs.rate) <= 1e-9 * fobs.rate and abs(lt.out_start - fobs.start_seconds) <= 1e-12
    lt.close()
    # the engine unpacks, the float kernel runs: the same bits
    ref = _fold(gpu, paths[machine], M, ppb, fuse_heaps=False)
    assert ref.fb.takes_heaps() and not ref.fb.fuse_heaps
    assert np.array_equal(ref.subints[0]["hits"], hits)
    assert np.array_equal(ref.subints[0]["profile_dev"].cpu().numpy().view(np.int32), prof.view(np.int32))
    ref.close()
    # the oracle chain
    assert np.array_equal(hits, ps.hits)
    got = prof.reshape(NCHAN, 1, NBIN, 4)
    err = np.abs(got - ps.data).max() / np.abs(ps.data).max()
    print(machine, "largest error of the folded sums / largest sum", err)
    assert err <= 1e-5


def test_fold_file_of_heaps_long_response(oracle, gpu, tmp_path_factory):
    """-x 16384: no heap loader for this length (takes_heaps() == 0) -- the engine unpacks and the three-pass convolution runs"""
    M, ppb = 16384, 2
    paths, r, step, ovl, ps, fobs = _observation(oracle, tmp_path_factory, M, ppb)
    assert (ppb * step) % 256 != 0
    lt = _fold(gpu, paths["MKBF"], M, ppb)
    assert not lt.fb.takes_heaps() and lt.fb.npass(False) == 3
    assert np.abs(r.buffer - lt.response.kernel).max() <= 1.2e-7 and (r.impulse_pos, r.impulse_neg) == (lt.response.impulse_pos, lt.response.impulse_neg)
    sub = lt.subints[0]
    assert np.array_equal(sub["hits"], ps.hits)
    got = sub["profile_dev"].cpu().numpy().reshape(NCHAN, 1, NBIN, 4)
    err = np.abs(got - ps.data).max() / np.abs(ps.data).max()
    print("largest error of the folded sums / largest sum", err)
    assert err <= 1e-5
    lt.close()


def test_search_mode_reads_heaps_through_the_engine(oracle, gpu, tmp_path_factory):
    """`digifil -F 4:D -x 1024 -t 4` (LoadToFilCoherent) on blocks of heaps, the second and third starting inside a heap: both machines
    give the same scrunched rows bit for bit, and those are the rows of the same samples in generic DADA order -- another kernel path:
    each path is held to 1e-5 of the largest value against the float64 oracle by the suite, so the two differ by at most twice that"""
    from dspsr_amd import dada, pipeline
    M, ppb = 1024, 3
    paths, r, step, ovl, ps, fobs = _observation(oracle, tmp_path_factory, M, ppb)
    cfg = pipeline.SearchConfig(nchan=NCHAN, tscrunch=4, nbit=8, rescale_seconds=0.0, parts_per_block=ppb, dispersion_measure=DM, freq_res=M,
                                npol=2, max_parts=2)
    rows = {}
    for machine in ("MKBF", "MKBFRo", "DADA"):
        f = dada.DadaFile(paths[machine if machine != "DADA" else "MKBF"])
        info = f.info
        if machine == "DADA":
            info = pipeline.InputInfo(**{**f.info.__dict__, "machine": "DADA"})
        lt = pipeline.LoadToFilCoherent(cfg, info, device=0, stream=torch.cuda.current_stream().cuda_stream)
        assert (lt.nsamp_step, lt.nsamp_overlap) == (step, ovl)
        got = []
        for view, npart, first in f.blocks(lt):
            if machine == "DADA":                                  # the block's samples in TFP order
                nsamp = npart * step + ovl
                view = dada.tfp_from_heaps(view, NCHAN, 2, False)[first:first + nsamp].reshape(-1)
                out = lt.detect_scrunch(torch.from_numpy(np.array(view)).cuda(), npart)
            else:
                assert lt.fb.takes_heaps()
                out = lt.detect_scrunch(torch.from_numpy(np.array(view)).cuda(), npart, first)
            lt.synchronize()
            got.append(out.cpu().numpy().copy())
        lt.close()
        rows[machine] = np.concatenate(got, axis=2)
    assert rows["MKBF"].shape[2] == (NBLOCKS * ppb * step) // 4 and np.abs(rows["MKBF"]).max() > 0
    assert np.array_equal(rows["MKBF"].view(np.int32), rows["MKBFRo"].view(np.int32))
    assert np.abs(rows["MKBF"] - rows["DADA"]).max() <= 2e-5 * np.abs(rows["DADA"]).max()


def test_subband_run_on_one_channels_runs(oracle, gpu, tmp_path_factory):
    from dspsr_amd import dada, pipeline
    M, ppb, g = 1024, 3, 1
    paths, r, step, ovl, ps, fobs = _observation(oracle, tmp_path_factory, M, ppb)
    whole = _fold(gpu, paths["MKBFRo"], M, ppb)
    want = whole.subints[0]["profile_dev"].cpu().numpy().reshape(NCHAN, NBIN, 4)[g].copy()
    want_hits = whole.subints[0]["hits"].copy()
    whole.close()
    f = dada.DadaFile(paths["MKBFRo"])
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, freq_res=M, ndim=4, parts_per_block=ppb, max_parts=2)
    lt = pipeline.LoadToFold(cfg, f.info, device=0, stream=torch.cuda.current_stream().cuda_stream, subband=g)
    assert lt.fb.takes_heaps() and lt.in_nchan == 1
    assert lt.process_host_blocks(f.blocks(lt, channel=g)) == NBLOCKS
    lt.finish_subint()
    lt.synchronize()
    got = lt.subints[0]["profile_dev"].cpu().numpy().reshape(1, NBIN, 4)[0]
    assert np.array_equal(lt.subints[0]["hits"], want_hits)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    lt.close()


def test_fold_tool_takes_the_format_from_the_header(oracle, gpu, tmp_path_factory, tmp_path):
    """tools/dspsr_amd_fold.py -F 4:D on an MKBFRo file, no new option: the PhaseSeries file of the pipeline call it makes, and the
    profile of the same samples folded with the engine unpacking first"""
    import importlib.util
    import os
    from dspsr_amd import dada, pipeline
    M, ppb = 1024, 3
    paths, r, step, ovl, ps, fobs = _observation(oracle, tmp_path_factory, M, ppb)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool_gpu_heaps", os.path.join(root, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    prefix = str(tmp_path / "tool")
    tool.main(["-F", "%d:D" % NCHAN, "-D", str(DM), "-x", str(M), "-b", str(NBIN), "-c", str(PERIOD), "-O", prefix, paths["MKBFRo"]])
    h, hits, prof = pipeline.read_phase_series(prefix + "_0000.ps")
    assert hits.sum() == int(h["NDAT_TOTAL"]) == NBLOCKS * ppb * step and np.abs(prof).max() > 0
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, freq_res=M, fuse_heaps=False)
    lt = dada.fold_file(paths["MKBFRo"], cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)
    mine = str(tmp_path / "mine_0000.ps")
    pipeline.write_phase_series(mine, lt.subints[0], lt.info, cfg, npol=lt.npol_out, scale=lt.subints[0].get("scale", lt.scalefac), division=0,
                                start_seconds=lt.out_start, folding_period=PERIOD)
    lt.close()
    assert open(prefix + "_0000.ps", "rb").read() == open(mine, "rb").read()
