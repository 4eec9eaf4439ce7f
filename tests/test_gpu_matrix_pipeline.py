"""`dspsr -pac` through the pipeline: pipeline.Config.calibrator builds chirp x Jones per bin (dspsr_amd/polcal.py) and hands it to the
filterbank as a matrix response; the tool spells it -pac.

Reference: tests/matrix_cases.py filterbank_matrix in float64 -> oracle.detect_products -> oracle.fold; hits equal, profiles within
1e-5 of the maximum (the bound of every pipeline parity test here).  The input is the small synthetic pulsar of dspsr_amd.synth:
64 channels of 256 bins, two blocks of three parts."""
import importlib.util
import os

import numpy as np
import pytest

import matrix_cases as mc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P = dict(freq=1382.0, bw=-16.0, tsamp_us=1.0 / 32.0, dm=30.0, period=0.004, nchan=64, nbin=64, freq_res=256)
PARTS, NBLOCK = 3, 2


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    return dspsr_amd


def calibrator(n=16, seed=21):
    """n calibrator channels across the band (scrambled order), well-conditioned Jones matrices"""
    rng = np.random.default_rng(seed)
    freq = P["freq"] + (np.arange(n) + 0.5) / n * abs(P["bw"]) - 0.5 * abs(P["bw"])
    order = rng.permutation(n)
    return freq[order], mc.jones_matrices(n, seed)[order]


def config(pipeline, **extra):
    return pipeline.Config(nchan=P["nchan"], dispersion_measure=P["dm"], nbin=P["nbin"], folding_period=P["period"],
                           freq_res=P["freq_res"], parts_per_block=PARTS, max_parts=2, **extra)


def info_of(pipeline):
    return pipeline.InputInfo(centre_frequency=P["freq"], bandwidth=P["bw"], tsamp_us=P["tsamp_us"], machine="DADA")


def run(pipeline, synth, cfg):
    """(first sub-integration, LoadToFold attributes the reference needs, raw int8 stream)"""
    lt = pipeline.LoadToFold(cfg, info_of(pipeline), stream=torch.cuda.current_stream().cuda_stream)
    step, ovl = PARTS * lt.nsamp_step, lt.nsamp_overlap
    raw = synth.voltages(NBLOCK * step + ovl, P["freq"], P["bw"], P["tsamp_us"], P["dm"], P["period"])
    dev = torch.from_numpy(raw.reshape(-1)).cuda()
    for b in range(NBLOCK):
        lt.process_block(dev[2 * b * step:2 * ((b + 1) * step + ovl)])
    lt.finish_subint()
    sub = lt.subints[0]
    prof = pipeline.subint_profile(sub).reshape(P["nchan"], 1, P["nbin"], 4).copy()
    keep = dict(hits=sub["hits"].copy(), kernel=lt.response.kernel.copy(), ndat=lt.response.ndat, pos=lt.response.impulse_pos,
                neg=lt.response.impulse_neg, fused=lt.fused_fold, ndim=lt.fb.response_ndim())
    lt.close()
    return prof, keep, raw


def test_load_to_fold_with_a_calibrator(oracle, gpu):
    from dspsr_amd import pipeline, polcal, synth
    o = oracle
    freq, jones = calibrator()
    prof, k, raw = run(pipeline, synth, config(pipeline, calibrator=(freq, jones)))
    assert k["ndim"] == 8 and not k["fused"] and k["ndat"] == P["freq_res"]
    obs = o.Observation(centre_frequency=P["freq"], bandwidth=P["bw"], tsamp_us=P["tsamp_us"], dispersion_measure=P["dm"])
    plan = mc.make_plan(o, P["nchan"], P["freq_res"], (k["pos"], k["neg"]), True)
    matrix = polcal.response_product(polcal.jones_response(freq, jones, obs, P["nchan"], P["freq_res"]), k["kernel"])
    npart = PARTS * NBLOCK
    fb = mc.filterbank_matrix(o.unpack_8bit(raw, obs), plan, matrix, npart, dtype=np.float64)
    det = o.detect_layout(o.detect_products(fb, "Coherence"), 4)
    fobs = o.filterbank_output_observation(obs, plan)
    ps = o.PhaseSeries(P["nchan"], 1, 4, P["nbin"], data=np.zeros((P["nchan"], 1, P["nbin"], 4), np.float64))
    o.fold(det, fobs, o.FoldConfig(nbin=P["nbin"], folding_period=P["period"]), ps)
    assert np.array_equal(k["hits"], ps.hits) and ps.hits.sum() == npart * plan.nkeep
    err = np.abs(prof - ps.data).max() / np.abs(ps.data).max()
    print("calibrated profile: max error %.3g of the maximum" % err)
    assert err <= 1e-5
    # the calibrator does something: the uncalibrated run differs
    plain, _, _ = run(pipeline, synth, config(pipeline, fused_fold=False))
    assert np.abs(plain - prof).max() > 1e-2 * np.abs(prof).max()


def test_identity_calibrator_changes_nothing(gpu):
    from dspsr_amd import pipeline, polcal, synth
    a, ka, _ = run(pipeline, synth, config(pipeline, calibrator=polcal.identity_calibrator(P["freq"])))
    b, kb, _ = run(pipeline, synth, config(pipeline, fused_fold=False))
    assert (ka["ndim"], kb["ndim"]) == (8, 2) and np.abs(a).max() > 0
    assert np.array_equal(ka["hits"], kb["hits"]) and np.array_equal(a, b)


def test_refusals_come_before_any_device_work(gpu, monkeypatch):
    from dspsr_amd import pipeline
    cal = calibrator()

    def no_device(*a, **kw):
        raise AssertionError("a device context was opened before the refusal")
    monkeypatch.setattr(pipeline, "Context", no_device)
    info = info_of(pipeline)
    for extra, inf, word in [(dict(convolve_when="after"), info, "convolve_when"),
                             (dict(), pipeline.InputInfo(centre_frequency=P["freq"], bandwidth=16.0, nchan=2, ndim=2, tsamp_us=0.125,
                                                         machine="DADA"), "one input channel"),
                             (dict(), pipeline.InputInfo(centre_frequency=P["freq"], bandwidth=P["bw"], npol=1, tsamp_us=P["tsamp_us"],
                                                         machine="DADA"), "two polarisations"),
                             (dict(nchan=96), info, "powers of"),
                             (dict(cyclic_nchan=16), info, "-cyclic"),
                             (dict(plfb_nbin=16), info, "-G")]:
        kw = dict(nchan=P["nchan"], dispersion_measure=P["dm"], nbin=P["nbin"], folding_period=P["period"], freq_res=P["freq_res"],
                  parts_per_block=PARTS, max_parts=2, calibrator=cal)
        kw.update(extra)
        with pytest.raises(gpu.DspsrAmdError, match=word):
            pipeline.LoadToFold(pipeline.Config(**kw), inf)


def test_tool_pac_writes_the_pipeline_file(gpu, tmp_path):
    from dspsr_amd import dada, pipeline, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool_gpu_pac", os.path.join(root, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    freq, jones = calibrator()
    cal = tmp_path / "cal.npz"
    np.savez(cal, freq=freq, jones=jones)
    probe = pipeline.LoadToFold(config(pipeline), info_of(pipeline), stream=torch.cuda.current_stream().cuda_stream)
    step, ovl = probe.nsamp_step, probe.nsamp_overlap
    probe.close()
    raw = synth.voltages(6 * step + ovl, P["freq"], P["bw"], P["tsamp_us"], P["dm"], P["period"])
    path = tmp_path / "in.dada"
    path.write_bytes(synth.dada_header(P["freq"], P["bw"], 1, 2, 1, P["tsamp_us"], extra={"DM": P["dm"]}) + raw.tobytes())
    prefix = str(tmp_path / "tool")
    tool.main(["-F", "%d:D" % P["nchan"], "-pac", str(cal), "-x", str(P["freq_res"]), "-b", str(P["nbin"]), "-c", str(P["period"]),
               "-O", prefix, str(path)])
    # the same through the pipeline call the tool makes
    hdr, _ = dada.read_header(str(path))
    info, _ = dada.observation(hdr)
    cfg = pipeline.Config(nchan=P["nchan"], dispersion_measure=P["dm"], nbin=P["nbin"], folding_period=P["period"],
                          freq_res=P["freq_res"], calibrator=(freq, jones))
    lt = dada.fold_file(str(path), cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)
    assert lt.fb.response_ndim() == 8 and len(lt.subints) == 1
    mine = str(tmp_path / "mine_0000.ps")
    pipeline.write_phase_series(mine, lt.subints[0], info, cfg, npol=lt.npol_out, scale=lt.subints[0].get("scale", lt.scalefac),
                                division=0, start_seconds=lt.out_start, folding_period=P["period"])
    lt.close()
    h, hits, prof = pipeline.read_phase_series(prefix + "_0000.ps")
    assert hits.sum() == int(h["NDAT_TOTAL"]) > 0 and np.abs(prof).max() > 0
    assert open(prefix + "_0000.ps", "rb").read() == open(mine, "rb").read()
