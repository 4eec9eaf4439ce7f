"""`dspsr -R` through the pipeline on the stream of tests/rfi_pipeline_case.py: -F 16:D with 256-point responses (the mask of 1024
channels is stretched four times), three blocks of three parts.  The GPU filter's mask against the restatement's; the folded profiles
bit for bit against a run handed the restatement's product through set_kernel, against the oracle within the bound of the
phase-locked filterbank's route (four times the float32 oracle's own error), and -- with the reference's literal loop, whose mask is
all ones -- bit for bit against a run without -R."""
import numpy as np
import pytest

import rfi_pipeline_case as pc
import rfi_reference as rr
import dspsr_amd
from dspsr_amd import pipeline, rfi

pytestmark = pytest.mark.gpu


def _info():
    return pipeline.InputInfo(centre_frequency=pc.FREQ, bandwidth=pc.BW, npol=2, ndim=1, tsamp_us=pc.TSAMP, machine="CASPSR", mjd_sec=0.0)


def _cfg(**kw):
    return pipeline.Config(nchan=pc.NCHAN, dispersion_measure=pc.DM, nbin=pc.NBIN, folding_period=pc.PERIOD, freq_res=pc.FREQ_RES,
                           parts_per_block=pc.PARTS, max_parts=2, **kw)


@pytest.fixture(scope="module")
def case(oracle):
    plan = pc.plan(oracle)
    raw = pc.stream(plan.nsamp_step, plan.nsamp_overlap)
    _band, want = pc.restatement(raw, np.float32)
    return plan, raw, want


def _run(raw, cfg, keep_zapped=None, product_of=None):
    """keep_zapped: build an RfiFilter on the pipeline's context and give it to set_rfi_filter; product_of: a mask whose product
    (the numpy restatement's) goes to the response engine's set_kernel directly.  Returns (profile, hits, filter results)."""
    import torch
    lt = pipeline.LoadToFold(cfg, _info(), stream=torch.cuda.current_stream().cuda_stream)
    dev = torch.from_numpy(raw).cuda()
    ndat = raw.size // 2
    assert ndat == pc.NBLOCK * pc.PARTS * lt.nsamp_step + lt.nsamp_overlap
    found = None
    if keep_zapped is not None:
        filt = rfi.RfiFilter(lt.ctx, _info(), interval=pc.INTERVAL, keep_zapped=keep_zapped)
        used = filt.integrate_raw(dev, ndat)
        assert used == pc.blocks_used() * pc.BLOCK and filt.complete and filt.integrate_raw(dev, ndat) == 0      # excess input is not used
        lt.set_rfi_filter(filt)
        assert filt.bandpass.integration_samples == used
        found = dict(filt.result, passband=filt.passband.copy())
        filt.close()
    if product_of is not None:
        k = lt.response.kernel
        lt.fb.set_kernel(rr.response_multiply(k, rr.rfi_expand(product_of, k.size)))      # -F N:D: the convolving filterbank itself
    step, ovl = pc.PARTS * lt.nsamp_step, lt.nsamp_overlap
    for b in range(pc.NBLOCK):
        lt.process_block(dev[2 * b * step:2 * ((b + 1) * step + ovl)])
    lt.finish_subint()
    sub = lt.subints[0]
    prof = pipeline.subint_profile(sub).reshape(pc.NCHAN, 1, pc.NBIN, 4).copy()
    hits = sub["hits"].copy()
    kernel = lt.response.kernel.copy()
    lt.close()
    return prof, hits, found, kernel


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_mask_product_and_profiles(case, oracle):
    o = oracle
    plan, raw, want = case
    prof, hits, found, kernel = _run(raw, _cfg(zap_rfi=True), keep_zapped=True)
    # (a) the mask is the restatement's, and the tones' channels are in it
    assert np.array_equal(found["mask"], want["mask"]) and found["rounds"] == want["rounds"] and found["total_zapped"] == want["total_zapped"]
    assert all(found["mask"][k] == 0 for k, *_ in pc.TONES) and found["mask"].sum() < 1024
    band64, _ = pc.restatement(raw, np.float64)
    e_band = np.abs(found["passband"][:, 0].astype(np.float64) - band64[:, 0]).max() / band64.max()
    print("rfi passband e_gpu=%.3e" % e_band)
    assert e_band <= 1e-5
    # (b) bit for bit the run that is handed the restatement's product
    prof_b, hits_b, _, _ = _run(raw, _cfg(), product_of=want["mask"])
    assert np.array_equal(hits, hits_b) and np.array_equal(_bits(prof), _bits(prof_b)) and np.abs(prof).max() > 0
    # (c) the oracle's filterbank with the product -> detect -> fold
    product = rr.response_multiply(kernel, rr.rfi_expand(want["mask"], kernel.size))
    obs = o.Observation(centre_frequency=pc.FREQ, bandwidth=pc.BW, tsamp_us=pc.TSAMP, dispersion_measure=pc.DM, machine="CASPSR")
    unpacked = o.unpack_8bit(raw, obs)
    fobs = o.filterbank_output_observation(obs, plan)

    def route(dtype):
        fb = o.filterbank(unpacked, plan, kernel=product, dtype=dtype)
        det = o.detect_layout(o.detect_products(fb, "Coherence"), 4)
        ps = o.PhaseSeries(pc.NCHAN, 1, 4, pc.NBIN, data=np.zeros((pc.NCHAN, 1, pc.NBIN, 4), dtype))
        o.fold(det, fobs, o.FoldConfig(nbin=pc.NBIN, folding_period=pc.PERIOD), ps)
        return ps
    ref, f32 = route(np.float64), route(np.float32)
    assert np.array_equal(hits, ref.hits) and ref.hits.sum() == pc.NBLOCK * pc.PARTS * plan.nkeep
    e_gpu = np.abs(prof - ref.data).max() / np.abs(ref.data).max()
    e_f32 = np.abs(f32.data.astype(np.float64) - ref.data).max() / np.abs(ref.data).max()
    print("rfi route e_gpu=%.3e e_f32=%.3e ratio=%.2f" % (e_gpu, e_f32, e_gpu / e_f32))
    assert e_f32 > 0 and e_gpu <= 4 * e_f32, "e_gpu %.3e > 4 x e_f32 %.3e" % (e_gpu, e_f32)
    # the filter does something: the run without it differs
    plain, hits_p, _, _ = _run(raw, _cfg())
    assert np.array_equal(hits, hits_p) and np.abs(plain - prof).max() > 1e-3 * np.abs(prof).max()
    # (d) the reference's literal loop leaves a mask of ones: the profiles of a run without -R, bit for bit
    prof_d, hits_d, found_d, _ = _run(raw, _cfg(zap_rfi=True), keep_zapped=False)
    assert np.all(found_d["mask"] == 1) and np.array_equal(found_d["p0"] == 0, want["mask"] == 0)
    assert np.array_equal(hits_d, hits_p) and np.array_equal(_bits(prof_d), _bits(plain))


@pytest.mark.parametrize("when,freq_res", [("after", pc.FREQ_RES), ("before", 4096)])
def test_the_convolution_engines_take_the_product(case, when, freq_res):
    """(e) convolve_when = "after" (and "before", with the 4096 points the whole band needs): the product goes to the Convolution's
    engine; the mask comes from the same first blocks of the stream"""
    import torch
    _plan, raw, want = case
    ndat_all = raw.size // 2

    def cfg(**kw):
        return pipeline.Config(nchan=pc.NCHAN, dispersion_measure=pc.DM, nbin=pc.NBIN, folding_period=pc.PERIOD, freq_res=freq_res,
                               parts_per_block=1, max_parts=1, convolve_when=when, **kw)

    def run(cfg_, **kw):
        lt = pipeline.LoadToFold(cfg_, _info(), stream=torch.cuda.current_stream().cuda_stream)
        dev = torch.from_numpy(raw).cuda()
        k = lt.response.kernel
        assert k.size >= 1024 and k.size % 1024 == 0                  # the mask is stretched, not dropped
        if when == "after":
            assert (k.size, lt.response.ndat) == (pc.NCHAN * pc.FREQ_RES, pc.FREQ_RES)
        found = None
        if "keep_zapped" in kw:
            filt = rfi.RfiFilter(lt.ctx, _info(), interval=pc.INTERVAL, keep_zapped=kw["keep_zapped"])
            assert filt.integrate_raw(dev, ndat_all) == pc.blocks_used() * pc.BLOCK
            lt.set_rfi_filter(filt)
            found = filt.result
            filt.close()
        if "product_of" in kw:
            # the engine named here, not asked of the pipeline: the Convolution behind (after) or in front of (before) the filterbank
            assert isinstance(lt.fb.conv, dspsr_amd.ConvolutionEngine) and lt.fb.conv.response_ndim() == 2
            lt.fb.conv.set_kernel(rr.response_multiply(k, rr.rfi_expand(kw["product_of"], k.size)))
        step, ovl = lt.nsamp_step, lt.nsamp_overlap
        nblock = min((ndat_all - ovl) // step, 4)
        assert nblock >= 2
        for b in range(nblock):
            lt.process_block(dev[2 * b * step:2 * ((b + 1) * step + ovl)])
        lt.finish_subint()
        prof = pipeline.subint_profile(lt.subints[0]).copy()
        lt.close()
        return prof, found
    prof, found = run(cfg(zap_rfi=True), keep_zapped=True)
    assert np.array_equal(found["mask"], want["mask"])
    prof_b, _ = run(cfg(), product_of=want["mask"])
    assert np.array_equal(_bits(prof), _bits(prof_b)) and np.abs(prof).max() > 0
    plain, _ = run(cfg())
    assert np.abs(plain - prof).max() > 1e-3 * np.abs(prof).max()


def test_zap_rfi_wants_its_filter_and_refuses_before_a_device(case, monkeypatch):
    import torch
    _plan, raw, _want = case
    lt = pipeline.LoadToFold(_cfg(zap_rfi=True), _info(), stream=torch.cuda.current_stream().cuda_stream)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="set_rfi_filter before the first block"):
        lt.process_block(torch.from_numpy(raw).cuda())
    lt.close()

    def no_device(*a, **kw):
        raise AssertionError("a device context was opened before the refusal")
    monkeypatch.setattr(pipeline, "Context", no_device)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="needs a dedispersion kernel"):
        pipeline.LoadToFold(_cfg(zap_rfi=True, convolve_when="never"), _info())


def test_tool_R_reads_the_file_and_prints_the_references_lines(case, tmp_path, capsys):
    """tools/dspsr_amd_fold.py -R: the filter is built from the file's first second -- here the whole file, in whole 8192-sample
    blocks -- before the block loop; the reference's lines go to stderr; the file written is the pipeline's sub-integration"""
    import importlib.util
    import os
    import torch
    from dspsr_amd import dada, synth
    _plan, raw, _want = case
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool_gpu_rfi", os.path.join(root, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = tmp_path / "in.dada"
    path.write_bytes(synth.dada_header(pc.FREQ, pc.BW, 1, 2, 1, pc.TSAMP, instrument="CASPSR", extra={"DM": pc.DM}) + raw.tobytes())
    prefix = str(tmp_path / "out")
    tool.main(["-F", "%d:D" % pc.NCHAN, "-x", str(pc.FREQ_RES), "-b", str(pc.NBIN), "-c", str(pc.PERIOD), "-R", "-O", prefix, str(path)])
    err = capsys.readouterr().err
    hdr, hits, prof = pipeline.read_phase_series(prefix + "_0000.ps")
    # the same through the library: every whole block of the file (it is shorter than a second)
    ndat = raw.size // 2
    blocks = ndat // pc.BLOCK
    band = rr.bandpass_loop(rr.decode_raw(raw, "caspsr", 1, 2, 1, 1.0, np.float32)[:, :, :blocks * pc.BLOCK] * np.float32(dspsr_amd.eight_bit_scale()),
                            1, pc.NCHAN_BP, 2, np.float32)
    want = rr.rfi_calculate(band[0, 0], band[1, 0], pc.WINDOW, True)
    assert want["margin"] >= 1e-3
    lines = [l for l in err.splitlines() if l.startswith("\t")]
    assert len(lines) == want["rounds"] + 1 and lines[-1] == "\tzapped %d channels" % want["total_zapped"]
    assert all(l.startswith("\tround %d cutoff = " % (k + 1)) for k, l in enumerate(lines[:-1]))
    cfg = pipeline.Config(nchan=pc.NCHAN, dispersion_measure=pc.DM, nbin=pc.NBIN, folding_period=pc.PERIOD, freq_res=pc.FREQ_RES)
    lt = dada.fold_file(str(path), cfg, stream=torch.cuda.current_stream().cuda_stream)
    k = lt.response.kernel.copy()
    lt.close()
    lt = pipeline.LoadToFold(cfg, dada.DadaFile(str(path)).info, stream=torch.cuda.current_stream().cuda_stream)
    lt.fb.set_kernel(rr.response_multiply(k, rr.rfi_expand(want["mask"], k.size)))
    f = dada.DadaFile(str(path))
    lt.process_host_blocks(f.blocks(lt))
    lt.finish_subint()
    lt.synchronize()
    assert len(lt.subints) == 1 and np.array_equal(hits, lt.subints[0]["hits"]) and prof.any()
    mine = str(tmp_path / "mine_0000.ps")
    pipeline.write_phase_series(mine, lt.subints[0], f.info, cfg, npol=lt.npol_out, scale=lt.subints[0].get("scale", lt.scalefac),
                                division=0, start_seconds=lt.out_start, folding_period=pc.PERIOD)
    lt.close()
    assert open(prefix + "_0000.ps", "rb").read() == open(mine, "rb").read()
