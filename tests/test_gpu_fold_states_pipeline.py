"""pipeline.LoadToFold with npol 1 and 2 (dspsr -d 1, -d 2) and one-polarisation input (PP), on the synthetic stream and the small
geometry of the existing pipeline tests (tests/test_gpu_parity.py: 16 channels, 64 bins, blocks of 3 parts).

1. against the oracle chain filterbank -> square_law -> fold composed here, with the bound the parity tests apply to the Coherence
   profile of this geometry (1e-5 of the profile's maximum against float64); hits and integration length exact;
2. bit for bit the model of the fused kernel (fold_state_cases.loadtofold_block_model_sq);
3. -L sub-integrations, two pulsars, -K, a pre_Fold tap and one-polarisation input against Detection + Fold (fused_fold=False);
4. the tool end to end with -d 1 and -d 2."""
import importlib.util
import os

import numpy as np
import pytest

import fold_state_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQ, BW, TSAMP, DM, PERIOD, NCHAN, NBIN = 1382.0, -16.0, 1.0 / 32.0, 30.0, 0.004, 16, 64
STATES = {1: ("Intensity", 1), 2: ("PPQQ", 2)}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    import oracle.dspsr_oracle as o
    from dspsr_amd import dada, pipeline, synth
    return dict(dspsr_amd=dspsr_amd, o=o, dada=dada, pipeline=pipeline, synth=synth, stream=torch.cuda.current_stream().cuda_stream,
                ncu=torch.cuda.get_device_properties(0).multi_processor_count)


def _cfg(env, **kw):
    return env["pipeline"].Config(**{**dict(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, parts_per_block=3, max_parts=2), **kw})


def _info(env, **kw):
    return env["pipeline"].InputInfo(**{**dict(centre_frequency=FREQ, bandwidth=BW, tsamp_us=TSAMP, machine="DADA"), **kw})


@pytest.fixture(scope="module")
def stream4(env):
    """four parts of the synthetic stream and the oracle's float64 filterbank output of them: the reference every test shares"""
    p, o = env["pipeline"], env["o"]
    lt = p.LoadToFold(_cfg(env), _info(env), device=0, stream=env["stream"])
    step, ovl, kernel = lt.nsamp_step, lt.nsamp_overlap, lt.response.kernel.copy()
    lt.close()
    raw = env["synth"].voltages(4 * step + ovl, FREQ, BW, TSAMP, DM, PERIOD)
    obs = o.Observation(centre_frequency=FREQ, bandwidth=BW, tsamp_us=TSAMP, dispersion_measure=DM)
    plan = o.filterbank_plan(obs, NCHAN, o.Dedispersion().match(obs, NCHAN))
    fb = o.filterbank(o.unpack_8bit(raw, obs), plan, kernel, dtype=np.float64)
    fb.setflags(write=False)
    return dict(raw=raw, dev=torch.from_numpy(raw).cuda(), step=step, ovl=ovl, obs=obs, plan=plan, fb=fb)


@pytest.mark.parametrize("npol", [1, 2])
def test_profile_against_the_oracle_chain_and_the_kernel_model(env, stream4, npol):
    p, o, s = env["pipeline"], env["o"], stream4
    name, npo = STATES[npol]
    lt = p.LoadToFold(_cfg(env, npol=npol, force_fused=True), _info(env), device=0, stream=env["stream"])
    assert lt.fused_fold and lt.fused_mode == 1 and lt.state_name() == name and lt.detected.shape[:2] == (NCHAN, npo)
    step, ovl = s["step"], s["ovl"]
    model = np.zeros((NCHAN, npo, NBIN, 1), np.float32)
    hits = np.zeros(NBIN, np.uint32)
    for first, npart in ((0, 3), (3, 1)):
        block = s["dev"][2 * first * step: 2 * ((first + npart) * step + ovl)]
        mode, h, model = sc.loadtofold_block_model_sq(lt, block, npart, model, env["ncu"])
        assert mode == 1 and model is not None
        hits += h
        lt.process_block(block, npart=npart)
    lt.finish_subint()
    lt.synchronize()
    sub = lt.subints[0]
    got = sub["profile_dev"].cpu().numpy().reshape(NCHAN, npo, NBIN, 1)
    assert np.array_equal(sub["hits"], hits)
    assert np.abs(model).max() > 0 and np.array_equal(got.view(np.int32), model.view(np.int32)), "the fused sums are not the model's"
    # the oracle chain
    det = o.square_law(s["fb"], name)[..., None]                    # [chan][npo][ndat][1], float64
    fobs = o.filterbank_output_observation(s["obs"], s["plan"])
    ps = o.PhaseSeries(NCHAN, npo, 1, NBIN, data=np.zeros((NCHAN, npo, NBIN, 1), np.float64))
    fcfg = o.FoldConfig(nbin=NBIN, folding_period=PERIOD)
    nk = s["plan"].nkeep
    o.fold(det, fobs, fcfg, ps, idat_start=0, ndat_fold=3 * nk)
    o.fold(det, fobs, fcfg, ps, idat_start=3 * nk, ndat_fold=nk)
    assert np.array_equal(sub["hits"], ps.hits)
    assert sub["integration_length"] == ps.integration_length and sub["ndat_total"] == ps.ndat_total == 4 * nk
    err = np.abs(got - ps.data).max() / np.abs(ps.data).max()
    print("npol %d: profile against the float64 oracle chain: %.3g of the maximum" % (npol, err))
    assert err <= 1e-5
    lt.close()


def _drive(env, s, cfg, info=None, dev=None, after_block=None, blocks=((0, 3), (3, 1)), **kw):
    """blocks of 3 parts then the last part through a LoadToFold: (instance closed, sub-integration lists as host copies)"""
    lt = env["pipeline"].LoadToFold(cfg, info or _info(env), device=0, stream=env["stream"], **kw)
    dev, per = s["dev"] if dev is None else dev, (2 if (info is None or info.npol == 2) else 1)
    step, ovl = lt.nsamp_step, lt.nsamp_overlap                   # (those of the shared stream unless the run has another DM)
    for first, npart in blocks:
        assert per * ((first + npart) * step + ovl) <= dev.numel()
        lt.process_block(dev[per * first * step: per * ((first + npart) * step + ovl)], npart=npart)
        if after_block is not None:
            lt.synchronize()
            after_block(lt)
    lt.finish_subint()
    lt.synchronize()
    accs = lt.pulsars or [lt]
    out = [[(x["hits"].copy(), x["profile_dev"].cpu().numpy(), x["integration_length"], x["ndat_total"]) for x in a.subints] for a in accs]
    fused = lt.fused_mode
    lt.close()
    return fused, out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) >= 1
        for (h0, p0, t0, n0), (h1, p1, t1, n1) in zip(x, y):
            assert np.array_equal(h0, h1) and t0 == t1 and n0 == n1 and np.abs(p0).max() > 0
            assert np.array_equal(p0.view(np.int32), p1.view(np.int32))


@pytest.mark.parametrize("npol", [1, 2])
def test_combinations_equal_detection_and_fold(env, stream4, npol, tmp_path):
    """every combination here runs in mode 1 (forced) or 0: bit for bit"""
    p, s = env["pipeline"], stream4
    npo = STATES[npol][1]
    plain_mode, plain = _drive(env, s, _cfg(env, npol=npol, force_fused=True))
    _, ref = _drive(env, s, _cfg(env, npol=npol, fused_fold=False))
    assert plain_mode == 1
    _same(plain, ref)
    # -L: sub-integrations that end inside blocks
    mode, fused = _drive(env, s, _cfg(env, npol=npol, force_fused=True, subint_seconds=0.002))
    _, sep = _drive(env, s, _cfg(env, npol=npol, fused_fold=False, subint_seconds=0.002))
    assert mode == 1 and len(fused[0]) >= 2
    _same(fused, sep)
    assert sum(x[3] for x in fused[0]) == plain[0][0][3]
    # two pulsars: the first one is the plain run's
    targets = [p.FoldTarget("a", folding_period=PERIOD, nbin=NBIN), p.FoldTarget("b", folding_period=0.0031, nbin=32)]
    _, two = _drive(env, s, _cfg(env, npol=npol), targets=targets)
    _, two_sep = _drive(env, s, _cfg(env, npol=npol, fused_fold=False), targets=targets)
    _same(two, two_sep)
    assert two[1][0][1].size == NCHAN * npo * 32
    _same([two[0]], plain)
    # -K
    kcfg = dict(npol=npol, interchan_dedispersion=True)
    kmode, k = _drive(env, s, _cfg(env, force_fused=True, **kcfg))
    _, k_sep = _drive(env, s, _cfg(env, fused_fold=False, **kcfg))
    assert kmode == 0
    _same(k, k_sep)
    # a pre_Fold tap: the same profile, and the detected rows in the file under the state's name
    held = []
    tmode, tapped = _drive(env, s, _cfg(env, npol=npol, force_fused=True), dump_before=("Fold",), dump_dir=str(tmp_path),
                           after_block=lambda lt: held.append(lt.detected.cpu().numpy().copy()))
    assert tmode == 0
    _same(tapped, plain)
    text, det = env["dada"].read_dump(str(tmp_path / "pre_Fold.dump"))
    hinfo, _ex = env["dada"].observation(text)
    assert (hinfo.nchan, hinfo.npol, hinfo.ndim) == (NCHAN, npo, 1) and env["dada"].header_get(text, "STATE") == STATES[npol][0]
    nk = s["plan"].nkeep
    assert det.shape == (4 * nk, NCHAN, npo, 1)
    # the file holds, bit for bit, the detected rows the pipeline held in HBM after each block (3 parts, then 1)
    rows = np.concatenate([held[0][:, :, :3 * nk], held[1][:, :, :nk]], axis=2)
    assert np.abs(rows).max() > 0 and np.array_equal(np.moveaxis(det[..., 0], 0, 2).view(np.int32), rows.view(np.int32))


def test_one_polarisation_input_folds_as_pp(env, stream4, capfd):
    p, o, s = env["pipeline"], env["o"], stream4
    one = np.ascontiguousarray(s["raw"].reshape(-1, 2)[:, 0])
    dev = torch.from_numpy(one).cuda()
    info = _info(env, npol=1)
    mode, got = _drive(env, s, _cfg(env, npol=2, force_fused=True), info=info, dev=dev)
    assert "Only single polarization detection available" in capfd.readouterr().err
    _, sep = _drive(env, s, _cfg(env, npol=1, fused_fold=False), info=info, dev=dev)
    assert mode == 1                                      # an object of one polarisation fuses (the store's one-polarisation branch)
    _same(got, sep)
    hits, prof, length, ndat = got[0][0]
    obs = o.Observation(centre_frequency=FREQ, bandwidth=BW, tsamp_us=TSAMP, dispersion_measure=DM, npol=1)
    lt = p.LoadToFold(_cfg(env, npol=1), info, device=0, stream=env["stream"])
    assert lt.state_name() == "PP" and lt._fold_dims() == (1, 1)
    kernel = lt.response.kernel.copy()
    lt.close()
    fb = o.filterbank(o.unpack_8bit(one, obs), s["plan"], kernel, dtype=np.float64)
    det = o.square_law(fb, "Intensity")[..., None]
    ps = o.PhaseSeries(NCHAN, 1, 1, NBIN, data=np.zeros((NCHAN, 1, NBIN, 1), np.float64))
    fobs = o.filterbank_output_observation(obs, s["plan"])
    nk = s["plan"].nkeep
    for a, n in ((0, 3 * nk), (3 * nk, nk)):
        o.fold(det, fobs, o.FoldConfig(nbin=NBIN, folding_period=PERIOD), ps, idat_start=a, ndat_fold=n)
    assert np.array_equal(hits, ps.hits) and length == ps.integration_length
    assert np.abs(prof.reshape(NCHAN, 1, NBIN, 1) - ps.data).max() <= 1e-5 * np.abs(ps.data).max()


@pytest.mark.parametrize("npol", [1, 2])
def test_tool_end_to_end(env, stream4, npol, tmp_path):
    p, s = env["pipeline"], stream4
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool_states", os.path.join(ROOT, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = tmp_path / "in.dada"
    path.write_bytes(env["synth"].dada_header(FREQ, BW, 1, 2, 1, TSAMP, extra={"DM": DM}) + s["raw"].tobytes())
    prefix = str(tmp_path / "out")
    tool.main(["-F", "%d:D" % NCHAN, "-d", str(npol), "-b", str(NBIN), "-c", str(PERIOD), "-O", prefix, str(path)])
    hdr, hits, prof = p.read_phase_series(prefix + "_0000.ps")
    name, npo = STATES[npol]
    assert (hdr["STATE"], int(hdr["NPOL"]), int(hdr["NDIM"]), int(hdr["NCHAN"]), int(hdr["NBIN"])) == (name, npo, 1, NCHAN, NBIN)
    lt = env["dada"].fold_file(str(path), p.Config(nchan=NCHAN, dispersion_measure=DM, nbin=NBIN, folding_period=PERIOD, npol=npol), stream=env["stream"])
    sub = lt.subints[0]
    want = sub["profile"] if sub.get("profile") is not None else sub["profile_dev"].cpu().numpy()
    assert np.array_equal(hits, sub["hits"]) and int(hdr["NDAT_TOTAL"]) == sub["ndat_total"] > 0
    assert prof.any() and np.array_equal(prof.view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).reshape(prof.shape).view(np.uint32))
    lt.close()
    # the profile of the oracle chain over the one block the file holds (four parts), per bin, at the bound of test 1
    o = env["o"]
    nk = s["plan"].nkeep
    assert sub["ndat_total"] == 4 * nk
    ps = o.PhaseSeries(NCHAN, npo, 1, NBIN, data=np.zeros((NCHAN, npo, NBIN, 1), np.float64))
    o.fold(o.square_law(s["fb"], name)[..., None], o.filterbank_output_observation(s["obs"], s["plan"]), o.FoldConfig(nbin=NBIN, folding_period=PERIOD),
           ps, idat_start=0, ndat_fold=4 * nk)
    assert np.array_equal(hits, ps.hits) and float(hdr["INTEGRATION_LENGTH"]) == ps.integration_length
    err = np.abs(prof - ps.data).max() / np.abs(ps.data).max()
    print("tool -d %d: profile against the float64 oracle chain: %.3g of the maximum" % (npol, err))
    assert err <= 1e-5
