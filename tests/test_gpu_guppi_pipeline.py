"""GUPPI raw files through the pipelines: a synthetic dispersed pulse in 4 channels written as a raw file (blocks of 4099 kept samples
and 13 overlap samples per run), folded with dada.fold_file against the float64 oracle chain of tests/test_gpu_heaps_pipeline.py --
the voltages going in as float(int8) by the restatement of tests/guppi_cases.py -- through the one-pass convolution (M = 1024) and
the three-pass one (M = 16384); a file with a missing block against the file that holds zeros in its place; search mode through
LoadToFilCoherent; the refusals of the drivers that read raw bytes themselves; and tools/dspsr_amd_fold.py as a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guppi_cases as gc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQ, BW, NCHAN, TSAMP, DM, PERIOD, NBIN = 1382.0, -16.0, 4, 0.25, 10.0, 0.004, 64
NBLOCKS = 3
BN, OVL, PKTS = 4099, 13, 16              # kept and overlap samples of a run; packets per block (4099 * 16 bytes = 16 packets of 4099)
CARDS = {"OBSFREQ": FREQ, "OBSBW": BW, "TBIN": TSAMP * 1e-6}


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
    """(path, samples int8 [chan][pol][ndat][2], response, step, overlap, oracle fold, output observation, directory) of the M-point
    case, made once: at least 5 raw blocks, and NBLOCKS pipeline blocks"""
    if M in _made:
        return _made[M]
    from dspsr_amd import synth
    obs, r = _response(o, M)
    step, ovl = M - r.impulse_pos - r.impulse_neg, r.impulse_pos + r.impulse_neg
    nblk = max(5, -(-(NBLOCKS * ppb * step + ovl) // BN))
    ndat = nblk * BN
    tfp = synth.voltages(ndat, FREQ, BW, TSAMP, DM, PERIOD, npol=2, ndim=2, nchan=NCHAN).reshape(ndat, NCHAN, 2, 2)
    x = np.ascontiguousarray(tfp.transpose(1, 2, 0, 3))
    d = tmp_path_factory.mktemp("guppi%d" % M)
    path = str(d / "pulse.raw")
    gc.write_raw(path, x, BN, OVL, packets_per_block=PKTS, cards=CARDS)
    ps, fobs = _oracle_fold(o, obs, r, gc.rows_of(gc.complex_of(x), 0, ndat), ppb)
    _made[M] = (path, x, r, step, ovl, ps, fobs, d)
    return _made[M]


def _oracle_fold(o, obs, r, rows, ppb):
    """the oracle chain in float64 on float rows [chan][pol][2 * ndat]: convolution of every channel, detection, fold pipeline block
    by pipeline block (the last one ragged)"""
    plan = o.filterbank_plan(obs, NCHAN, r)
    step, ovl = plan.nsamp_step, plan.nsamp_overlap
    npart = (rows.shape[2] // 2 - ovl) // step
    cv = o.convolution(rows, r.ndat, r.impulse_pos, r.impulse_neg, r.buffer, False, npart=npart, dtype=np.float64)
    fobs = o.filterbank_output_observation(obs, plan)
    det = o.detect_layout(o.detect_products(cv, "Coherence"), 4)
    ps = o.PhaseSeries(NCHAN, 1, 4, NBIN, data=np.zeros((NCHAN, 1, NBIN, 4), np.float64))
    fcfg = o.FoldConfig(nbin=NBIN, folding_period=PERIOD)
    done = 0
    while done < npart:
        n = min(ppb, npart - done)
        o.fold(det, fobs, fcfg, ps, idat_start=done * plan.nkeep, ndat_fold=n * plan.nkeep)
        done += n
    return ps, fobs


def _fold(path, M, ppb, **kw):
    from dspsr_amd import dada, pipeline
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, freq_res=M, ndim=4, parts_per_block=ppb,
                          max_parts=2, **kw)
    return dada.fold_file(path, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("M,ppb", [(1024, 3), (16384, 2)])
def test_fold_file_of_a_raw_file(oracle, gpu, tmp_path_factory, M, ppb):
    """hits equal the oracle's exactly; largest error of the folded sums / largest sum <= 1e-5, the bound tests/test_gpu_heaps_pipeline.py
    holds the same chain to"""
    from dspsr_amd import guppi
    path, x, r, step, ovl, ps, fobs, _d = _observation(oracle, tmp_path_factory, M, ppb)
    lt = _fold(path, M, ppb)
    assert lt.info.machine == "GUPPI" and lt.layout & 0xff == gpu.RAW_GUPPI and lt.fb.npass(False) == (1 if M == 1024 else 3)
    assert np.abs(r.buffer - lt.response.kernel).max() <= 1.2e-7 and (r.impulse_pos, r.impulse_neg) == (lt.response.impulse_pos, lt.response.impulse_neg)
    assert (lt.nsamp_step, lt.nsamp_overlap) == (step, ovl)
    f = guppi.GuppiFile(path)
    firsts = [first for _v, _n, first in f.blocks(lt)]
    assert len(firsts) >= NBLOCKS and firsts[0] == 0 and firsts[1] and firsts[2]           # the second and third blocks start inside a raw block
    assert f.ndat == x.shape[2] and lt.nsamples_in == ((f.ndat - ovl) // step) * step
    sub = lt.subints[0]
    hits, prof = sub["hits"].copy(), sub["profile_dev"].cpu().numpy().copy()
    assert abs(lt.out_rate - fobs.rate) <= 1e-9 * fobs.rate and abs(lt.out_start - fobs.start_seconds) <= 1e-12
    lt.close()
    assert np.array_equal(hits, ps.hits)
    got = prof.reshape(NCHAN, 1, NBIN, 4)
    err = np.abs(got - ps.data).max() / np.abs(ps.data).max()
    print("M", M, "largest error of the folded sums / largest sum", err)
    assert err <= 1e-5


def test_a_missing_block_folds_like_a_block_of_zeros(oracle, gpu, tmp_path_factory):
    M, ppb = 1024, 3
    _p, x, r, step, ovl, _ps, _fobs, d = _observation(oracle, tmp_path_factory, M, ppb)
    gap, zeros = str(d / "gap.raw"), str(d / "zeros.raw")
    gc.write_raw(gap, x, BN, OVL, packets_per_block=PKTS, cards=CARDS, seq=[(0, 0), (1, PKTS), (3, 3 * PKTS), (4, 4 * PKTS)])
    gc.write_raw(zeros, x, BN, OVL, packets_per_block=PKTS, cards=CARDS, seq=[(0, 0), (1, PKTS), (None, 2 * PKTS), (3, 3 * PKTS)])
    from dspsr_amd import guppi
    fg, fz = guppi.GuppiFile(gap), guppi.GuppiFile(zeros)
    assert fg.ndat == fz.ndat == 4 * BN and fg.stream[2] is None and None not in fz.stream and len(fg.stream) == 4
    res = []
    for path in (gap, zeros):
        lt = _fold(path, M, ppb)
        assert lt.nsamples_in == ((4 * BN - ovl) // step) * step
        res.append((lt.subints[0]["hits"].copy(), lt.subints[0]["profile_dev"].cpu().numpy().copy()))
        lt.close()
    assert np.abs(res[0][1]).max() > 0
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1].view(np.int32), res[1][1].view(np.int32))


def test_subband_run_on_one_channels_runs(oracle, gpu, tmp_path_factory):
    """rank g of a sub-band sharded run reads channel g's runs alone (nchan 1, block_stride = chan_stride): channel g of the whole run"""
    from dspsr_amd import guppi, pipeline
    M, ppb, g = 1024, 3, 2
    path = _observation(oracle, tmp_path_factory, M, ppb)[0]
    whole = _fold(path, M, ppb)
    want = whole.subints[0]["profile_dev"].cpu().numpy().reshape(NCHAN, NBIN, 4)[g].copy()
    want_hits = whole.subints[0]["hits"].copy()
    whole.close()
    f = guppi.GuppiFile(path)
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, freq_res=M, ndim=4, parts_per_block=ppb, max_parts=2)
    lt = pipeline.LoadToFold(cfg, f.info, device=0, stream=torch.cuda.current_stream().cuda_stream, subband=g)
    assert lt.in_nchan == 1 and lt.guppi == (BN, f.chan_stride, f.chan_stride)
    assert lt.process_host_blocks(f.blocks(lt, channel=g)) == sum(1 for _ in f.blocks(lt))
    lt.finish_subint()
    lt.synchronize()
    got = lt.subints[0]["profile_dev"].cpu().numpy().reshape(1, NBIN, 4)[0]
    assert np.abs(want).max() > 0 and np.array_equal(lt.subints[0]["hits"], want_hits)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    lt.close()


@pytest.mark.parametrize("when", ["after", "before"])
def test_the_other_chains_read_the_raw_file(oracle, gpu, tmp_path_factory, when):
    """`-F 16` and `-F 16:B`: the engine that reads the 8-bit block sits inside a wrapper and is given the geometry all the same --
    the same stream written as 4 blocks of 4099 (+ 13 overlap) samples and as 2 blocks of 8198 folds to the same bits"""
    from dspsr_amd import dada, pipeline
    _p, x, _r, _s, _o, _ps, _fobs, d = _observation(oracle, tmp_path_factory, 1024, 3)
    x = np.ascontiguousarray(x[:, :, :4 * BN])
    res = []
    for name, (bn, ovl) in (("a", (BN, OVL)), ("b", (2 * BN, 0))):
        path = str(d / ("%s_%s.raw" % (when, name)))
        gc.write_raw(path, x, bn, ovl, packets_per_block=PKTS, cards=CARDS)
        cfg = pipeline.Config(nchan=16, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, ndim=4, parts_per_block=3, max_parts=2,
                              convolve_when=when, freq_res=1024 if when == "before" else 0)
        lt = dada.fold_file(path, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)
        assert lt.guppi == (bn, (bn + ovl) * 4, NCHAN * (bn + ovl) * 4) and lt.nsamples_in > 0
        res.append((lt.subints[0]["hits"].copy(), lt.subints[0]["profile_dev"].cpu().numpy().copy()))
        lt.close()
    assert res[0][0].sum() > 0 and np.abs(res[0][1]).max() > 0
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1].view(np.int32), res[1][1].view(np.int32))


def test_search_mode_reads_the_raw_file_through_the_engine(oracle, gpu, tmp_path_factory):
    """`digifil -F 4:D -x 1024 -t 4` (LoadToFilCoherent): the scrunched rows of the raw file == those of the same engine fed the
    restatement's float rows, bit for bit"""
    from dspsr_amd import guppi, pipeline
    M, ppb, ts = 1024, 3, 4
    path, x, r, step, ovl, _ps, _fobs, _d = _observation(oracle, tmp_path_factory, M, ppb)
    cfg = pipeline.SearchConfig(nchan=NCHAN, tscrunch=ts, nbit=8, rescale_seconds=0.0, parts_per_block=ppb, dispersion_measure=DM, freq_res=M,
                                npol=2, max_parts=2)
    f = guppi.GuppiFile(path)
    stream = gc.complex_of(x)
    lt = pipeline.LoadToFilCoherent(cfg, f.info, device=0, stream=torch.cuda.current_stream().cuda_stream)
    ref = pipeline.LoadToFilCoherent(cfg, f.info, device=0, stream=torch.cuda.current_stream().cuda_stream)
    assert (lt.nsamp_step, lt.nsamp_overlap) == (step, ovl)
    carry = torch.zeros((NCHAN, 2), dtype=torch.float32, device="cuda")
    cc, got, want, s0 = 0, [], [], 0
    for view, npart, first in f.blocks(lt):
        assert first == s0 % BN
        out = lt.detect_scrunch(torch.from_numpy(np.array(view)).cuda(), npart, first)
        lt.synchronize()
        got.append(out.cpu().numpy().copy())
        rows = torch.from_numpy(gc.rows_of(stream, s0, npart * step + ovl)).cuda()
        buf = torch.zeros((NCHAN, 2, (cc + npart * step) // ts), dtype=torch.float32, device="cuda")
        nout, cc = ref.fb.perform_search(buf, carry, cc, npart, ts, gpu.PPQQ, inp=rows, in_step=2 * step)
        ref.synchronize()
        want.append(buf[:, :, :nout].cpu().numpy().copy())
        s0 += npart * step
    lt.close()
    ref.close()
    got, want = np.concatenate(got, axis=2), np.concatenate(want, axis=2)
    assert got.shape == want.shape and got.shape[2] == s0 // ts and np.abs(got).max() > 0
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_drivers_that_read_raw_bytes_refuse_the_file_by_name(oracle, gpu, tmp_path_factory):
    from dspsr_amd import dada, guppi, pipeline
    path = _observation(oracle, tmp_path_factory, 1024, 3)[0]
    info = guppi.GuppiFile(path).info
    with pytest.raises(gpu.DspsrAmdError, match=r"\(-R\).*GUPPI raw file"):
        _fold(path, 1024, 3, zap_rfi=True)
    with pytest.raises(gpu.DspsrAmdError, match="LoadToFil:.*GUPPI raw file"):
        pipeline.LoadToFil(pipeline.SearchConfig(nchan=16, tscrunch=4, nbit=8), info, device=0)
    with pytest.raises(gpu.DspsrAmdError, match="LoadToFilDirect.*GUPPI raw file"):
        pipeline.LoadToFilDirect(pipeline.SearchConfig(nchan=NCHAN, tscrunch=4, nbit=8), info, device=0)
    assert not dada.is_valid(path)


def test_fold_tool_takes_the_raw_file_with_no_format_option(oracle, gpu, tmp_path_factory, tmp_path):
    """tools/dspsr_amd_fold.py -F 4:D on the raw file, as a fresh child process: the PhaseSeries file of the pipeline call it makes"""
    from dspsr_amd import pipeline
    M, ppb = 1024, 3
    path, x, r, step, ovl, _ps, _fobs, _d = _observation(oracle, tmp_path_factory, M, ppb)
    prefix = str(tmp_path / "tool")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dspsr_amd_fold.py"), "-F", "%d:D" % NCHAN, "-D", str(DM), "-x", str(M),
                        "-b", str(NBIN), "-c", str(PERIOD), "-O", prefix, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    h, hits, prof = pipeline.read_phase_series(prefix + "_0000.ps")
    assert hits.sum() == int(h["NDAT_TOTAL"]) == ((x.shape[2] - ovl) // step) * step and np.abs(prof).max() > 0
    cfg = pipeline.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, freq_res=M)
    from dspsr_amd import dada
    lt = dada.fold_file(path, cfg, device=0, stream=torch.cuda.current_stream().cuda_stream)
    mine = str(tmp_path / "mine_0000.ps")
    pipeline.write_phase_series(mine, lt.subints[0], lt.info, cfg, npol=lt.npol_out, scale=lt.subints[0].get("scale", lt.scalefac), division=0,
                                start_seconds=lt.out_start, folding_period=PERIOD)
    lt.close()
    assert open(prefix + "_0000.ps", "rb").read() == open(mine, "rb").read()
