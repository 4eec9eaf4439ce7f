"""Fourth-order moments of the Stokes parameters (`dspsr -4`) on the GPU: dspsr_amd_fourth_moment, the moments fold with its two
loaders (csrc/fold_moments.hip), LoadToFold with fourth_moment and tools/dspsr_amd_fold.py -4.

a  the stand-alone operation, bitwise against numpy float32 (tests/moments_cases.py fourth_moment) on placed rows
b  one body, two loaders: fold_moments(stokes) == fold(the stream fourth_moment wrote), bit for bit, on float data
c  bit for bit against the sequential fold of tests/fold_reference.py (it takes ndim 14 unchanged) on sums exact in any order
d  Gaussian data against float64 within the a-priori bound of a float32 sum of n = hits + 1 roundings
e  LoadToFold(fourth_moment=True) against fold_moments applied by the test to the rows of perform_detect
f  the tool writes FourthMoment / 1 / 14 files
The nbin of the moments fold has no upper limit of its own (bins beyond 512 go to further workgroups): 4097 is the case beyond
the 4096 of the ordinary fold's chunk kernels, in nine bin groups.
"""
import math
import os

import numpy as np
import pytest

import moments_cases as mc
from device_buffers import SENTINEL, OutputLayout, device_rows, sentinel_rows
from fold_reference import fold_long_model, fold_time_order, runs_of_plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx, torch.cuda.get_device_properties(0).multi_processor_count
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- a. the stand-alone operation ---------------------------------------------------------------------------------------------------
def _wide(rng, shape):
    """normal values scaled to magnitudes in [2^-20, 2^20]: no product is subnormal or overflows"""
    x = rng.standard_normal(shape)
    x = np.where(np.abs(x) < 1e-3, 1e-3, x)
    x = x * 2.0 ** rng.uniform(-10, 10, shape)
    x = np.clip(np.abs(x), 2.0 ** -20, 2.0 ** 20) * np.sign(x)
    return x.astype(np.float32)


@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("ndat", [1, 5, 1027])
def test_fourth_moment_bitwise_on_placed_rows(gpu, nchan, ndat):
    dspsr_amd, ctx, _ = gpu
    rng = np.random.default_rng(100 * nchan + ndat)
    x = _wide(rng, (nchan, 1, ndat, 4))
    want = mc.fourth_moment(x)
    assert (np.abs(want) >= 2.0 ** -126).all() and np.isfinite(want).all()
    # rows cut from buffers: input 4 floats (16 bytes) past a 256-byte boundary and padded by 8, output 2 floats past and padded by 6
    d_in = device_rows(x.reshape(nchan, 1, ndat * 4), 4, 8)
    lay = OutputLayout(nchan, 1, ndat * 14, offset=2, row_pad=6)
    buf, d_out = sentinel_rows(lay)
    dspsr_amd.fourth_moment(ctx, d_in, d_out, ndat)
    ctx.synchronize()
    got = d_out.cpu().numpy().reshape(nchan, 1, ndat, 14)
    assert np.array_equal(_bits(got), _bits(want))
    inside = np.zeros(lay.size, bool)
    for c in range(nchan):
        inside[lay.first + c * lay.chan_stride:lay.first + c * lay.chan_stride + ndat * 14] = True
    assert (buf.cpu().numpy()[~inside] == SENTINEL).all(), "written outside the rows"


def test_fourth_moment_refusals_come_before_any_launch(gpu):
    dspsr_amd, ctx, _ = gpu
    from dspsr_amd import _lib
    nchan, ndat = 2, 40
    x = _wide(np.random.default_rng(1), (nchan, 1, ndat * 4))
    d_in = device_rows(x, 0, 0)
    lay = OutputLayout(nchan, 1, ndat * 14)
    buf, d_out = sentinel_rows(lay)
    f = lambda i, ics, o, ocs, n=ndat: _lib.lib.dspsr_amd_fourth_moment(ctx.handle, i, ics, o, ocs, nchan, n)
    ip, op = d_in.data_ptr(), d_out.data_ptr()
    assert f(ip, ndat * 4, ip, ndat * 14) == _lib.EINVAL                         # in place
    assert f(ip + 4, ndat * 4, op, ndat * 14) == _lib.EINVAL                     # input rows below 16 bytes
    assert f(ip, ndat * 4 + 2, op, ndat * 14) == _lib.EINVAL
    assert f(ip, ndat * 4, op + 4, ndat * 14) == _lib.EINVAL                     # output rows below 8 bytes
    assert f(ip, ndat * 4, op, ndat * 14 + 1) == _lib.EINVAL
    assert f(ip, ndat * 4 - 4, op, ndat * 14) == _lib.EINVAL                     # strides shorter than the rows
    assert f(ip, ndat * 4, op, ndat * 14 - 2) == _lib.EINVAL
    ctx.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all()
    assert f(ip, ndat * 4, op, ndat * 14, 0) == _lib.OK                          # ndat 0: nothing to do (FourthMoment.C:49-50)
    ctx.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all()
    assert f(ip, ndat * 4, op, ndat * 14) == _lib.OK
    ctx.synchronize()
    assert np.array_equal(_bits(d_out.cpu().numpy().reshape(nchan, ndat, 14)), _bits(mc.fourth_moment(x.reshape(nchan, ndat, 4))))


def test_shapes_accepted_and_refused(gpu):
    dspsr_amd, ctx, _ = gpu
    eng = dspsr_amd.FoldEngine(ctx)
    for npol, ndim in ((2, 14), (4, 14), (1, 3), (1, 8), (1, 16)):
        with pytest.raises(dspsr_amd.DspsrAmdError):
            eng.set_shape(3, npol, ndim, 8)
    x = torch.zeros((3, 1, 64), device="cuda")
    eng.set_shape(3, 1, 4, 8)
    eng.set_nbin(8)
    eng.set_bins(0.0, 0.1, 16, 0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="npol 1 x ndim 14"):
        eng.fold_moments(x)                                                       # a fold of another shape
    eng.fold(x)
    eng.set_shape(3, 1, 14, 8)
    other = dspsr_amd.FoldEngine(ctx)
    other.set_shape(3, 1, 14, 8)
    for e in (eng, other):
        e.set_nbin(8)
        e.set_bins(0.0, 0.1, 4, 0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="fourth moments"):
        dspsr_amd.FoldEngine.fold_many([eng, other], torch.zeros((3, 1, 14 * 4), device="cuda"))
    with pytest.raises(dspsr_amd.DspsrAmdError, match="fourth moments"):
        eng.fold_zeroed(torch.zeros((3, 1, 14 * 4), device="cuda"), torch.zeros((3, 8), dtype=torch.int32, device="cuda"))
    eng.close()
    other.close()


# ---- b. one body, two loaders ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spb,lng", [(1.7, False), (90.0, True)], ids=["short-runs", "long-runs"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
def test_stokes_loader_equals_stream_loader(gpu, oracle, spb, lng, offset):
    dspsr_amd, ctx, ncu = gpu
    nchan, nbin, ndat, i0 = 5, 37, 9001, 3                                       # 9001 - 3: no multiple of either chunk
    rng = np.random.default_rng(int(spb))
    x = (rng.standard_normal((nchan, 1, ndat, 4)) * np.array([3.0, 1.0, 0.5, 0.25]) + np.array([4.0, 0, 0, 0])).astype(np.float32)
    n = ndat - i0 - 2
    phi, pps = 0.31, 1.0 / (spb * nbin)
    runs = runs_of_plan(oracle.fold_binplan(phi, pps, nbin, n), i0)
    g = mc.geometry(nchan, nbin, runs, ncu)
    assert g["lng"] == lng and g["ragged_stokes"] and g["ragged_stream"] and g["nchunk_stokes"] > 1
    # unaligned: the rows start 4 bytes past a 16-byte boundary and their stride is odd -- the float-by-float fill of the same image
    d_x = device_rows(x.reshape(nchan, 1, ndat * 4), offset, 3 * offset)
    stream = torch.empty((nchan, 1, ndat * 14), dtype=torch.float32, device="cuda")
    dspsr_amd.fourth_moment(ctx, device_rows(x.reshape(nchan, 1, ndat * 4), 0, 0), stream)
    d_s = device_rows(stream.cpu().numpy(), 3 * offset, offset)
    prof0 = rng.standard_normal((nchan, 1, nbin, 14)).astype(np.float32)
    got = []
    for rows, moments in ((d_x, True), (d_s, False)):
        eng = dspsr_amd.FoldEngine(ctx)
        p = torch.from_numpy(prof0.reshape(nchan, nbin * 14)).cuda()
        eng.bind_profile(p, nchan, 1, 14, nbin)
        eng.set_nbin(nbin)
        eng.set_ndat(n, i0)
        assert eng.set_bins(phi, pps, n, i0) == n
        eng.fold_moments(rows) if moments else eng.fold(rows)
        got.append(eng.synch())
        eng.close()
    assert np.isfinite(got[0]).all() and not np.array_equal(got[0], prof0)
    assert np.array_equal(_bits(got[0]), _bits(got[1]))
    # and both are the association the kernel documents
    s = mc.fourth_moment(x)
    want = fold_long_model(s, runs, prof0, nchan * g["ngroup"], ncu) if lng else fold_time_order(s, runs, prof0)
    assert np.array_equal(_bits(got[0]), _bits(want))


# ---- c. bit for bit against the sequential reference ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_references(oracle):
    """the expected profile of every case of moments_cases.CASES, computed once: fold_time_order over the restated stream"""
    out = {}
    for case in mc.CASES:
        s = mc.fourth_moment(mc.case_stokes(case))
        prof = np.zeros((case["nchan"], 1, case["nbin"], 14), np.float32)
        for k in range(len(case["calls"])):
            plan, _, _ = mc.case_call_plan(case, k, oracle.fold_binplan)
            prof = fold_time_order(s, runs_of_plan(plan, case["calls"][k][0]), prof)
        prof.setflags(write=False)
        out[case["name"]] = prof
    return out


def _fold_case(dspsr_amd, ctx, oracle, case, rows, moments):
    eng = dspsr_amd.FoldEngine(ctx)
    eng.set_shape(case["nchan"], 1, 14, case["nbin"])
    hits = np.zeros(case["nbin"], np.uint32)
    for k, (i0, n) in enumerate(case["calls"]):
        plan, phi, pps = mc.case_call_plan(case, k, oracle.fold_binplan)
        eng.set_nbin(case["nbin"])
        eng.set_ndat(n, i0)
        if phi is None:
            for i, b in enumerate(plan.tolist()):
                eng.set_bin(i0 + i, float(b))
        else:
            assert eng.set_bins(phi, pps, n, i0, hits) == n
        assert eng.get_ndat_folded() == n
        eng.fold_moments(rows) if moments else eng.fold(rows)
    got = eng.synch()
    eng.close()
    return got


@pytest.mark.parametrize("case", mc.CASES, ids=[c["name"] for c in mc.CASES])
def test_exact_sums_bit_for_bit(gpu, oracle, exact_references, case):
    dspsr_amd, ctx, ncu = gpu
    x = mc.case_stokes(case)
    want = exact_references[case["name"]]
    d_x = device_rows(x.reshape(case["nchan"], 1, -1), 0, 4)
    got = _fold_case(dspsr_amd, ctx, oracle, case, d_x, True)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.abs(want).max() < 1 << 24 and want.any()
    # the stream loader on the restated stream: the same exact sums
    d_s = device_rows(mc.fourth_moment(x).reshape(case["nchan"], 1, -1), 0, 2)
    assert np.array_equal(_bits(_fold_case(dspsr_amd, ctx, oracle, case, d_s, False)), _bits(want))


def test_empty_plan_leaves_the_profile(gpu):
    dspsr_amd, ctx, _ = gpu
    eng = dspsr_amd.FoldEngine(ctx)
    nchan, nbin = 2, 16
    p0 = np.random.default_rng(2).standard_normal((nchan, nbin * 14)).astype(np.float32)
    p = torch.from_numpy(p0).cuda()
    eng.bind_profile(p, nchan, 1, 14, nbin)
    eng.set_nbin(nbin)
    eng.set_ndat(0, 5)
    assert eng.set_bins(0.2, 0.01, 0, 5) == 0                                     # ndat_fold = 0
    eng.fold_moments(torch.full((nchan, 1, 64), float("nan"), device="cuda"))
    eng.fold(torch.full((nchan, 1, 14 * 16), float("nan"), device="cuda"))
    assert eng.get_ndat_folded() == 0
    assert np.array_equal(_bits(eng.synch().reshape(nchan, -1)), _bits(p0))
    eng.close()


@pytest.mark.parametrize("spb", [2.2, 80.0], ids=["exact", "long"])
def test_bound_profile_with_padded_span(gpu, oracle, spb):
    """a caller's profile with rows `span` floats apart: the floats beyond each row keep the sentinel; zero() clears rows only"""
    dspsr_amd, ctx, ncu = gpu
    nchan, nbin, ndat, i0 = 3, 37, 5000, 2
    x = np.random.default_rng(4).integers(-8, 9, (nchan, 1, ndat, 4)).astype(np.float32)
    lay = OutputLayout(nchan, 1, nbin * 14, offset=1, row_pad=5)
    buf, rows = sentinel_rows(lay)
    prof = rows[:, 0, :]
    eng = dspsr_amd.FoldEngine(ctx)
    eng.bind_profile(prof, nchan, 1, 14, nbin)
    eng.zero()
    n = ndat - i0
    phi, pps = 0.6, 1.0 / (spb * nbin)
    eng.set_nbin(nbin)
    eng.set_ndat(n, i0)
    eng.set_bins(phi, pps, n, i0)
    eng.fold_moments(device_rows(x.reshape(nchan, 1, -1), 0, 0))
    got = eng.synch()
    eng.close()
    runs = runs_of_plan(oracle.fold_binplan(phi, pps, nbin, n), i0)
    assert mc.geometry(nchan, nbin, runs, ncu)["lng"] == (spb > 64)
    want = fold_time_order(mc.fourth_moment(x), runs, np.zeros((nchan, 1, nbin, 14), np.float32))
    assert np.array_equal(_bits(got), _bits(want))
    inside = np.zeros(lay.size, bool)
    for c in range(nchan):
        inside[lay.first + c * lay.chan_stride:lay.first + c * lay.chan_stride + nbin * 14] = True
    assert (buf.cpu().numpy()[~inside] == SENTINEL).all()


def test_weighted_plan_with_zero_weight_blocks(gpu, oracle):
    dspsr_amd, ctx, _ = gpu
    nchan, nbin, n = 3, 37, 3000
    x = np.random.default_rng(6).integers(-8, 9, (nchan, 1, n, 4)).astype(np.float32)
    w = np.ones(30, np.uint32)
    w[[0, 13, 14, 29]] = 0                                                        # the start, the middle, the end
    phi, pps = 0.2, 1.0 / (3.1 * nbin)
    runs, keep = mc.weighted_runs(oracle.fold_binplan(phi, pps, nbin, n), 0, w, 100)
    eng = dspsr_amd.FoldEngine(ctx)
    eng.set_shape(nchan, 1, 14, nbin)
    eng.set_nbin(nbin)
    eng.set_ndat(n, 0)
    hits = np.zeros(nbin, np.uint32)
    assert eng.set_bins(phi, pps, n, 0, hits, weights=w, ndatperweight=100) == keep.sum() == 2600
    eng.fold_moments(device_rows(x.reshape(nchan, 1, -1), 0, 0))
    got = eng.synch()
    eng.close()
    assert np.array_equal(hits, np.bincount(runs[:, 1], weights=runs[:, 2], minlength=nbin).astype(np.uint32))
    want = fold_time_order(mc.fourth_moment(x), runs, np.zeros((nchan, 1, nbin, 14), np.float32))
    assert np.array_equal(_bits(got), _bits(want))


# ---- d. general data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spb", [3.3, 150.0], ids=["exact", "long"])
def test_gaussian_data_within_the_summation_bound(gpu, oracle, spb):
    """|err| <= gamma_n * sum |terms|, gamma_n = n u / (1 - n u), u = 2^-24, n = hits + 1 (one rounding of the product, hits - 1
    additions and the addition to the zero profile): the bound of any order of summation, so the LONG association is covered"""
    dspsr_amd, ctx, _ = gpu
    nchan, nbin, ndat = 4, 64, 40000
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((nchan, 1, ndat, 4)) * np.array([2.0, 1.0, 1.0, 0.5]) + np.array([5.0, 0.5, 0, 0])).astype(np.float32)
    phi, pps = 0.45, 1.0 / (spb * nbin)
    plan = oracle.fold_binplan(phi, pps, nbin, ndat)
    eng = dspsr_amd.FoldEngine(ctx)
    eng.set_shape(nchan, 1, 14, nbin)
    eng.set_nbin(nbin)
    eng.set_ndat(ndat, 0)
    hits = np.zeros(nbin, np.uint32)
    eng.set_bins(phi, pps, ndat, 0, hits)
    eng.fold_moments(device_rows(x.reshape(nchan, 1, -1), 0, 0))
    got = eng.synch().astype(np.float64)
    eng.close()
    x64 = x.astype(np.float64)
    terms = np.concatenate([x64] + [(x64[..., i] * x64[..., j])[..., None] for i, j in mc.PAIRS], axis=-1)     # float64 products
    want = np.zeros((nchan, 1, nbin, 14))
    mag = np.zeros_like(want)
    for b in range(nbin):
        sel = plan == b
        want[:, :, b, :] = terms[:, :, sel, :].sum(axis=2)
        mag[:, :, b, :] = np.abs(terms[:, :, sel, :]).sum(axis=2)
    nn = (hits.astype(np.float64) + 1) * 2.0 ** -24
    gamma = (nn / (1 - nn))[None, None, :, None]
    err = np.abs(got - want)
    print("max err / bound = %.3g" % (err / np.maximum(gamma * mag, 1e-300)).max())
    assert (err <= gamma * mag).all() and hits.min() > 0


# ---- e. pipeline wiring -------------------------------------------------------------------------------------------------------------
# the smallest synthetic input of the end-to-end fixture (tests/golden/e2e_small.npz): n_fft 2^12 = 8 channels x 512, 64 bins
E2E = dict(freq=1382.0, bw=-8.0, tsamp_us=1.0 / 16.0, dm=20.0, period=0.002, nchan=8, nbin=64, freq_res=512)
PARTS = 3


def _e2e_config(pipeline, **extra):
    return pipeline.Config(nchan=E2E["nchan"], dispersion_measure=E2E["dm"], nbin=E2E["nbin"], folding_period=E2E["period"],
                           freq_res=E2E["freq_res"], parts_per_block=PARTS, max_parts=2, **extra)


def _e2e_blocks(lt, synth):
    step, ovl = lt.nsamp_step, lt.nsamp_overlap
    raw = synth.voltages(2 * PARTS * step + ovl, E2E["freq"], E2E["bw"], E2E["tsamp_us"], E2E["dm"], E2E["period"])
    dev = torch.from_numpy(raw.reshape(-1)).cuda()
    return [dev[2 * b * PARTS * step:2 * ((b + 1) * PARTS * step + ovl)] for b in range(2)]


def test_pipeline_wiring(gpu):
    dspsr_amd, ctx, _ = gpu
    from dspsr_amd import pipeline, synth
    info = pipeline.InputInfo(centre_frequency=E2E["freq"], bandwidth=E2E["bw"], tsamp_us=E2E["tsamp_us"], machine="DADA")
    stream = torch.cuda.current_stream().cuda_stream
    probe = pipeline.LoadToFold(_e2e_config(pipeline), info, stream=stream)
    nblock = PARTS * probe.nkeep
    subint = 1.6 * nblock / probe.out_rate                                        # one boundary, inside the second block
    probe.close()
    lt = pipeline.LoadToFold(_e2e_config(pipeline, subint_seconds=subint, fourth_moment=True, ndim=2), info, stream=stream)
    ref = pipeline.LoadToFold(_e2e_config(pipeline, subint_seconds=subint, stokes=True, ndim=4, fused_fold=False), info, stream=stream)
    assert lt.moments and not lt.fused_fold and lt.cfg.stokes and lt.cfg.ndim == 4 and lt.fold.shape == (E2E["nchan"], 1, E2E["nbin"], 14)
    pieces = [pipeline.subint_pieces(b * nblock, nblock, subint, lt.out_rate) for b in range(2)]
    assert [len(p) for p in pieces] == [1, 2] and pieces[1][0][3] and not pieces[1][1][3]
    mine = dspsr_amd.FoldEngine(ctx)
    mine.set_shape(E2E["nchan"], 1, 14, E2E["nbin"])
    want = []
    for b, raw in enumerate(_e2e_blocks(lt, synth)):
        lt.process_block(raw)
        ref.process_block(raw)                                                    # leaves the Stokes rows of perform_detect in ref.detected
        for i0, n, _div, complete in pieces[b]:
            t0 = lt.out_start + (b * nblock + i0 + 0.5) / lt.out_rate
            mine.set_nbin(E2E["nbin"])
            mine.set_ndat(n, i0)
            mine.set_bins(math.fmod(t0, E2E["period"]) / E2E["period"], (1.0 / lt.out_rate) / E2E["period"], n, i0)
            mine.fold_moments(ref.detected)
            if complete:
                want.append(mine.synch())
                mine.zero()
    want.append(mine.synch())
    lt.finish_subint()
    ref.finish_subint()
    assert len(lt.subints) == len(ref.subints) == len(want) == 2
    for sub, rsub, w in zip(lt.subints, ref.subints, want):
        got = pipeline.subint_profile(sub).reshape(w.shape)
        assert np.array_equal(_bits(got), _bits(w)) and got.any()
        assert np.array_equal(sub["hits"], rsub["hits"]) and sub["hits"].sum() == sub["ndat_total"]
        assert sub["integration_length"] == rsub["integration_length"] and sub["ndat_total"] == rsub["ndat_total"]
        # the first four components are the Stokes fold itself (same samples, time order: the plan has no long run)
        assert np.array_equal(_bits(got[..., :4]), _bits(pipeline.subint_profile(rsub).reshape(E2E["nchan"], 1, E2E["nbin"], 4)))
    with pytest.raises(dspsr_amd.DspsrAmdError, match=r"fourth_moment \(-4\)"):
        lt.set_communicator(None, 0, 2)
    mine.close()
    lt.close()
    ref.close()


# the geometry the other chains are tested with elsewhere (tests/test_gpu_plain.py, tests/test_gpu_fold_many.py)
OTHER = dict(freq=1382.0, bw=-16.0, tsamp_us=1.0 / 32.0, dm=30.0, period=0.004, nchan=16, nbin=64)


@pytest.mark.parametrize("extra", [dict(), dict(interchan_dedispersion=True), dict(convolve_when="after"), dict(convolve_when="before"),
                                   dict(convolve_when="never")], ids=["during", "K", "after", "before", "never"])
def test_pipeline_other_chains_and_the_fold_tap(gpu, extra, tmp_path):
    """-K and the other convolution orders reach the moments fold through the code paths they have; where the pre_Fold tap is
    built (-F N:D, with and without -K) the run with the tap -- FourthMoment materialised by dspsr_amd_fourth_moment, stream
    loader -- gives the bits of the run without it, and the dump holds the 14-float stream"""
    dspsr_amd, ctx, _ = gpu
    from dspsr_amd import dada, pipeline, synth
    p = OTHER
    info = pipeline.InputInfo(centre_frequency=p["freq"], bandwidth=p["bw"], tsamp_us=p["tsamp_us"], machine="DADA")
    stream = torch.cuda.current_stream().cuda_stream
    taps = [(), ("Fold",)] if extra.get("convolve_when", "during") == "during" else [()]
    res = []
    for tap in taps:
        cfg = pipeline.Config(nchan=p["nchan"], dispersion_measure=p["dm"], nbin=p["nbin"], folding_period=p["period"],
                              parts_per_block=PARTS, max_parts=2, fourth_moment=True, **extra)
        lt = pipeline.LoadToFold(cfg, info, stream=stream, dump_before=tap, dump_dir=str(tmp_path))
        step, ovl = PARTS * lt.nsamp_step, lt.nsamp_overlap
        raw = torch.from_numpy(synth.voltages(2 * step + ovl, p["freq"], p["bw"], p["tsamp_us"], p["dm"], p["period"])).cuda()
        for b in range(2):
            lt.process_block(raw[2 * b * step:2 * ((b + 1) * step + ovl)])
        lt.finish_subint()
        sub = lt.subints[0]
        res.append(pipeline.subint_profile(sub).reshape(p["nchan"], 1, p["nbin"], 14))
        assert sub["ndat_total"] == sub["hits"].sum() > 0 and np.isfinite(res[-1]).all()
        # sums of squares
        assert (res[-1][..., [4, 8, 11, 13]] >= 0).all() and res[-1][:, 0, sub["hits"] > 0, 4].min() > 0
        lt.close()
    if len(res) == 2:
        assert np.array_equal(_bits(res[0]), _bits(res[1]))
        # (the header reader keeps ASCIIObservation's NDIM 1 / 2 / 4: the 14-float dump is read by hand)
        text, hb = dada.read_header(str(tmp_path / "pre_Fold.dump"))
        assert dada.header_get(text, "STATE") == "FourthMoment" and (dada.header_get(text, "NPOL"), dada.header_get(text, "NDIM")) == ("1", "14")
        data = np.fromfile(str(tmp_path / "pre_Fold.dump"), dtype=np.float32, offset=hb).reshape(-1, p["nchan"], 1, 14)
        assert data.shape[0] == sub["ndat_total"]
        assert np.array_equal(_bits(data[..., 4]), _bits(data[..., 0] * data[..., 0]))


# ---- f. the tool ---------------------------------------------------------------------------------------------------------------------
def test_tool_writes_fourth_moment_files(gpu, tmp_path):
    import importlib.util
    from dspsr_amd import pipeline, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dspsr_amd_fold_tool_gpu_moments", os.path.join(root, "tools", "dspsr_amd_fold.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    info = pipeline.InputInfo(centre_frequency=E2E["freq"], bandwidth=E2E["bw"], tsamp_us=E2E["tsamp_us"], machine="DADA")
    probe = pipeline.LoadToFold(_e2e_config(pipeline), info, stream=torch.cuda.current_stream().cuda_stream)
    step, ovl, nkeep, rate = probe.nsamp_step, probe.nsamp_overlap, probe.nkeep, probe.out_rate
    probe.close()
    raw = synth.voltages(6 * step + ovl, E2E["freq"], E2E["bw"], E2E["tsamp_us"], E2E["dm"], E2E["period"])
    path = tmp_path / "in.dada"
    path.write_bytes(synth.dada_header(E2E["freq"], E2E["bw"], 1, 2, 1, E2E["tsamp_us"], extra={"DM": E2E["dm"]}) + raw.tobytes())
    prefix = str(tmp_path / "out")
    tool.main(["-F", "%d:D" % E2E["nchan"], "-4", "-x", str(E2E["freq_res"]), "-b", str(E2E["nbin"]), "-c", str(E2E["period"]),
               "-L", repr(4.8 * nkeep / rate), "-O", prefix, str(path)])
    total = 0
    for n in range(2):
        hdr, hits, prof = pipeline.read_phase_series("%s_%04d.ps" % (prefix, n))
        assert (hdr["STATE"], int(hdr["NPOL"]), int(hdr["NDIM"]), int(hdr["NCHAN"])) == ("FourthMoment", 1, 14, E2E["nchan"])
        assert prof.shape == (E2E["nchan"], 1, E2E["nbin"], 14) and hits.sum() == int(hdr["NDAT_TOTAL"]) > 0
        assert prof[:, 0, hits > 0, 4].min() > 0 and not prof[:, 0, hits == 0].any()
        means, central = pipeline.moments_to_central(prof, hits, float(hdr["SCALE"]))
        assert np.isfinite(central).all() and (central[:, 0, hits >= 8] > 0).all() and (hits >= 8).any()    # the variance of the mean of I
        total += int(hits.sum())
    assert total == 6 * nkeep and not os.path.exists(prefix + "_0002.ps")
