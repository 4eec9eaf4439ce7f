"""The square-law states at the C-ABI (dspsr -d 1, -d 2: DSPSR_AMD_INTENSITY, DSPSR_AMD_PPQQ), every comparison on the bits.

1. perform_detect(state) == perform_raw + dspsr_amd_detect_square_law == oracle.square_law of the complex rows, on one geometry of
   each route, the rows cut from a sentinel buffer in both row orders.
2. perform_fold(state) on every case of tests/fold_state_cases.py (records checked by tests/test_fold_state_cases_host.py):
   the model of the fused kernel k_inv_chan<., 3 | 7, .> (fold_state_cases.fused_fold_model_sq) or of Detection + Fold
   (fold_reference), fed with the rows of perform_detect on the same block; hits, fold_is_fused_state, and the floats around a
   bound profile's rows.
3. The four-pass geometry: mode 0 for these states, 3 for Coherence; the fold is Detection + Fold.
4. The stand-alone fold of npol 2 x ndim 1 equals two folds of npol 1 (kernels that existed before: see the test's docstring).
5. An object of one polarisation: Intensity folds the power of its polarisation (PP), fused; PPQQ is refused."""
import numpy as np
import pytest

import fold_state_cases as sc
import fused_fold_cases as fc
from fold_reference import fold_long_model, fold_time_order

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S8 = 1.0 / 48.0


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx, torch.cuda.get_device_properties(0).multi_processor_count
    ctx.close()


@pytest.fixture(scope="module")
def oracle():
    import oracle.dspsr_oracle as o
    return o


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.standard_normal(n) * 24.0), -128, 127).astype(np.int8)


def _kernel(n):
    return np.exp(1j * np.random.default_rng(17).uniform(-np.pi, np.pi, n)).astype(np.complex64)


# ---- 1. perform_detect ---------------------------------------------------------------------------------------------------------------
DETECT = {
    "three-pass-real": dict(C=32, M=256, nfilt=(100, 92), real=True, input_nchan=1),
    "two-pass-complex": dict(C=16, M=512, nfilt=(40, 3), real=False, input_nchan=1),
    "four-pass": dict(C=4, M=16384, nfilt=(301, 212), real=True, input_nchan=1),
    "nchan-3x32": dict(C=96, M=256, nfilt=(20, 21), real=True, input_nchan=1),
}


def _placed(nchan, npo, ndat, order):
    """rows [nchan][npo][ndat] cut from a NaN buffer at an odd float offset, with odd paddings: (buffer, view, mask of the rows)"""
    row = ndat + 3
    if order == "channel-major":
        ps, cs = row, npo * row + 5
    else:
        cs, ps = row, nchan * row + 7
    n = 8 + 1 + (nchan - 1) * cs + (npo - 1) * ps + ndat + 8
    buf = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    view = torch.as_strided(buf, (nchan, npo, ndat), (cs, ps, 1), 9)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.as_strided(mask, (nchan, npo, ndat), (cs, ps, 1), 9)[:] = True
    return buf, view, mask.cpu().numpy()


@pytest.mark.parametrize("geo", sorted(DETECT))
def test_perform_detect_is_filterbank_then_square_law(gpu, oracle, geo):
    dspsr_amd, ctx, _ncu = gpu
    c = DETECT[geo]
    C, M, parts = c["C"], c["M"], 3
    nkeep = M - sum(c["nfilt"])
    ndat = parts * nkeep
    eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, c["nfilt"][0], c["nfilt"][1], 1, 2, c["real"], _kernel(C * M), max_parts=2)
    assert eng.npass(True) == {"three-pass-real": 3, "two-pass-complex": 2, "four-pass": 4, "nchan-3x32": 3}[geo]
    raw = torch.from_numpy(_raw(fc.raw_bytes(c, parts), 77)).cuda()
    cplx = torch.zeros((C, 2, 2 * ndat), dtype=torch.float32, device="cuda")
    eng.perform_raw(raw, dspsr_amd.RAW_GENERIC, S8, cplx, parts)
    fb = cplx.cpu().numpy().reshape(C, 2, ndat, 2)
    fb = (fb[..., 0] + 1j * fb[..., 1]).astype(np.complex64)
    for state, npo, name in ((dspsr_amd.INTENSITY, 1, "Intensity"), (dspsr_amd.PPQQ, 2, "PPQQ")):
        sep = torch.zeros((C, npo, ndat), dtype=torch.float32, device="cuda")
        dspsr_amd.DetectionEngine(ctx).square_law(cplx, sep, intensity=state == dspsr_amd.INTENSITY)
        want = sep.cpu().numpy()
        assert np.abs(want).max() > 0
        assert np.array_equal(want.view(np.int32), oracle.square_law(fb, name).astype(np.float32).view(np.int32))
        for order in ("channel-major", "plane-major"):
            buf, view, mask = _placed(C, npo, ndat, order)
            before = buf.view(torch.int32).cpu().numpy().copy()
            eng.perform_detect(view, parts, state, 1, raw=raw, scale=S8)
            eng.finish()
            assert np.array_equal(view.cpu().numpy().view(np.int32), want.view(np.int32)), (geo, name, order)
            after = buf.view(torch.int32).cpu().numpy()
            assert np.array_equal(before[~mask], after[~mask]), "a float outside the rows changed"
    with pytest.raises(dspsr_amd.DspsrAmdError, match="overlap"):
        eng.perform_detect(torch.as_strided(torch.zeros(C * 2 * ndat, device="cuda"), (C, 2, ndat), (ndat, ndat - 1, 1)), parts, dspsr_amd.PPQQ, 1,
                           raw=raw, scale=S8)
    eng.close()


# ---- 2. perform_fold on the table ------------------------------------------------------------------------------------------------------
def _set_plan(fold, c, name, k, hits):
    runs, table_hits, ndat = sc.call_runs(name, k)
    plan = c["calls"][k][1]
    fold.set_nbin(c["nbin"])
    fold.set_ndat(ndat, 0)
    if plan[0] == "hand":
        for off, b, n in runs:
            for i in range(int(off), int(off + n)):
                fold.set_bin(i, float(b))
        hits += table_hits
    else:
        fold.set_bins(plan[1], plan[2], ndat, 0, hits)


def _run(gpu, name, max_parts=None):
    dspsr_amd, ctx, _ncu = gpu
    c = sc.by_name(name)
    C, M, inch = c["C"], c["M"], c["input_nchan"]
    nkeep = M - sum(c["nfilt"])
    nchan, npol, nbin, ndim = sc.shape(c)
    state = sc.STATE[c["prof"]]
    eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, c["nfilt"][0], c["nfilt"][1], inch, 2, c["real"], _kernel(inch * C * M),
                                                max_parts=max_parts or c["max_parts"], force_four_pass=c["four"], fused_fold=c["policy"])
    mode = eng.fold_is_fused(state)
    assert eng.fold_is_fused() == eng.fold_is_fused(dspsr_amd.STOKES)
    fold = dspsr_amd.FoldEngine(ctx)
    buf = pad = None
    if c["bound"] is None:
        fold.set_shape(nchan, npol, ndim, nbin)
    else:
        off, rpad = c["bound"]
        span = nbin * ndim + rpad
        buf = torch.full((64 + off + nchan * npol * span + 64,), float("nan"), dtype=torch.float32, device="cuda")
        lead = ((-buf.data_ptr()) % 256) // 4
        rows = buf[lead + off:lead + off + nchan * npol * span].view(nchan * npol, span)
        assert rows.data_ptr() % 256 == 4 * off
        rows[:, :nbin * ndim] = 0
        pad = buf.view(torch.int32).cpu().numpy().copy()
        fold.bind_profile(rows, nchan, npol, ndim, nbin)
    hits = np.zeros(nbin, np.uint32)
    dets = []
    for k, (parts, _plan) in enumerate(c["calls"]):
        raw = torch.from_numpy(_raw(fc.raw_bytes(c, parts), 3000 + 10 * sc.NAMES.index(name) + k)).cuda()
        det = torch.zeros((nchan, npol, parts * nkeep), dtype=torch.float32, device="cuda")
        eng.perform_detect(det, parts, state, 1, raw=raw, scale=S8)
        _set_plan(fold, c, name, k, hits)
        eng.perform_fold(fold, parts, state, raw=raw, scale=S8)
        dets.append(det.cpu().numpy())
    eng.finish()
    if buf is None:
        prof, after = fold.synch(), None
    else:
        after = buf.view(torch.int32).cpu().numpy()
        prof = rows[:, :nbin * ndim].cpu().numpy().reshape(nchan, npol, nbin, ndim)
        keep = np.ones(buf.numel(), bool)
        for r in range(nchan * npol):
            keep[lead + off + r * span:lead + off + r * span + nbin * ndim] = False
        pad, after = pad[keep], after[keep]
    eng.close()
    fold.close()
    return mode, hits, prof, dets, (pad, after)


def _model(name, dets, ncu):
    c, rec = sc.by_name(name), sc.record(name, ncu)
    nchan, npol, nbin, ndim = sc.shape(c)
    nkeep = c["M"] - sum(c["nfilt"])
    prof = np.zeros((nchan, npol, nbin, ndim), np.float32)
    hits = np.zeros(nbin, np.uint32)
    for k, call in enumerate(rec["calls"]):
        runs, h, _ndat = sc.call_runs(name, k)
        hits += h
        if call["path"] == "fused":
            nseg = {l["ns"]: l["nseg"] for l in call["launches"]}
            prof = sc.fused_fold_model_sq(dets[k], runs, prof, nkeep, [l["ns"] for l in call["launches"]], rec["mode"], nseg.__getitem__)
        else:
            rows = dets[k][..., None]                                    # [chan][pol][ndat][1]
            prof = fold_long_model(rows, runs, prof, nchan * npol, ncu) if call["assoc"] == "long" else fold_time_order(rows, runs, prof)
    return hits, prof


def _check(gpu, name, **kw):
    mode, hits, prof, dets, (pad, after) = _run(gpu, name, **kw)
    ncu = gpu[2]
    assert mode == sc.record(name, ncu)["mode"], "fold_is_fused_state is not the mode of the table (device of %d compute units)" % ncu
    want_hits, want = _model(name, dets, ncu)
    assert np.array_equal(hits, want_hits)
    assert np.abs(want).max() > 0
    bad = np.argwhere(prof.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, "%s: %d sums differ from the model, first at (chan, pol, bin, dim) = %s: %r != %r" % (
        name, len(bad), tuple(bad[0]), prof[tuple(bad[0])], want[tuple(bad[0])])
    if pad is not None:
        assert np.array_equal(pad, after), "a float outside the bound profile's rows changed"
    return prof


@pytest.mark.parametrize("name", sc.of_group("psl"))
def test_part_offsets_in_lds_and_in_global_memory(gpu, name):
    prof = _check(gpu, name)
    assert np.array_equal(prof, _run(gpu, name, max_parts=2)[2])


@pytest.mark.parametrize("name", sc.of_group("seg"))
def test_segmented_launches(gpu, name):
    prof = _check(gpu, name)
    assert np.array_equal(prof, _run(gpu, name)[2])            # deterministic


@pytest.mark.parametrize("name", sc.of_group("cap") + sc.of_group("runs") + sc.of_group("grid"))
def test_inside_a_tile(gpu, name):
    _check(gpu, name)


@pytest.mark.parametrize("name", sc.of_group("placement"))
def test_bound_profiles_fuse_at_any_float_address(gpu, name):
    _check(gpu, name)


def test_refused_pairings_name_state_and_shape(gpu):
    dspsr_amd, ctx, _ncu = gpu
    eng = dspsr_amd.FilterbankEngine(ctx).setup(32, 256, 100, 92, 1, 2, True, None, max_parts=2, fused_fold=dspsr_amd.FUSED_ALWAYS)
    raw = torch.from_numpy(_raw(fc.raw_bytes(DETECT["three-pass-real"], 1), 5)).cuda()
    fold = dspsr_amd.FoldEngine(ctx)
    for state, shape, text in ((dspsr_amd.INTENSITY, (2, 1), r"Intensity.*npol=1 ndim=1 \(is 32/2/1\)"),
                               (dspsr_amd.PPQQ, (1, 1), r"PPQQ.*npol=2 ndim=1 \(is 32/1/1\)"),
                               (dspsr_amd.INTENSITY, (1, 4), r"Intensity.*npol=1 ndim=1 \(is 32/1/4\)"),
                               (dspsr_amd.COHERENCE, (2, 1), r"npol=1 ndim=4 or npol=2 ndim=2 \(is 32/2/1\)")):
        fold.set_shape(32, shape[0], shape[1], 16)
        fold.set_nbin(16)
        with pytest.raises(dspsr_amd.DspsrAmdError, match=text):
            eng.perform_fold(fold, 1, state, raw=raw, scale=S8)
    # (the Python wrapper always asks for ndim 1; the C-ABI refuses any other)
    from dspsr_amd.engine import _check
    det = torch.zeros((32, 1, 4 * 64), dtype=torch.float32, device="cuda")
    with pytest.raises(dspsr_amd.DspsrAmdError, match="ndim=1, not ndim=4"):
        _check(ctx.handle, dspsr_amd.lib.dspsr_amd_filterbank_perform_detect(eng.handle, None, 0, 0, 0, raw.data_ptr(), dspsr_amd.RAW_GENERIC, S8,
                                                                             dspsr_amd.INTENSITY, 4, det.data_ptr(), det.stride(0), det.stride(1), 1),
               "dspsr_amd_filterbank_perform_detect")
    eng.close()
    fold.close()


# ---- 3. four passes ------------------------------------------------------------------------------------------------------------------
def test_four_pass_objects_run_detection_and_fold(gpu):
    dspsr_amd, ctx, ncu = gpu
    c = fc.by_name("segsum-exact")
    C, M, nbin = c["C"], c["M"], c["nbin"]
    nkeep = M - sum(c["nfilt"])
    parts = c["calls"][0][0]
    runs, table_hits, ndat = fc.call_runs("segsum-exact", 0)
    eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, c["nfilt"][0], c["nfilt"][1], 1, 2, True, _kernel(C * M), max_parts=c["max_parts"])
    assert eng.fold_is_fused() == 3 and eng.fold_is_fused(dspsr_amd.INTENSITY) == 0 and eng.fold_is_fused(dspsr_amd.PPQQ) == 0
    raw = torch.from_numpy(_raw(fc.raw_bytes(c, parts), 11)).cuda()
    for state, npo in ((dspsr_amd.INTENSITY, 1), (dspsr_amd.PPQQ, 2)):
        det = torch.zeros((C, npo, (ndat + 3) // 4 * 4), dtype=torch.float32, device="cuda")[:, :, :ndat]     # 16-byte aligned rows
        eng.perform_detect(det, parts, state, 1, raw=raw, scale=S8)
        got = []
        for fused in (True, False):
            fold = dspsr_amd.FoldEngine(ctx)
            fold.set_shape(C, npo, 1, nbin)
            fold.set_nbin(nbin)
            fold.set_ndat(ndat, 0)
            for off, b, n in runs:
                for i in range(int(off), int(off + n)):
                    fold.set_bin(i, float(b))
            if fused:
                eng.perform_fold(fold, parts, state, raw=raw, scale=S8)
            else:
                fold.fold(det)
            got.append(fold.synch())
            fold.close()
        assert np.abs(got[1]).max() > 0 and np.array_equal(got[0], got[1])
        assert np.array_equal(got[1], fold_long_model(det.cpu().numpy()[..., None], runs, np.zeros_like(got[1]), C * npo, ncu))
    eng.close()


# ---- 4. the stand-alone fold of npol 2 x ndim 1 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["phase", "hand-gaps", "long-runs"])
def test_two_rows_fold_as_two_single_rows(gpu, plan):
    """The shape perform_fold's Detection + Fold hands to the stand-alone fold.  No new kernel runs here: a FoldInstance<1, 2> is
    not built (tests/test_fold_plan_host.py pins fold_shape's answer for npol 2 x ndim 1 and the set of instantiations), so this
    holds the existing k_fold_*<1, 1> kernels on these rows and passes without the square-law states."""
    dspsr_amd, ctx, ncu = gpu
    nchan, nbin, ndat = 5, 48, 3 * 2048 + 76          # (rows of whole float4: the chunk kernels)
    rng = np.random.default_rng(3)
    det = torch.from_numpy((rng.standard_normal((nchan, 2, ndat)) * 50).astype(np.float32)).cuda()
    if plan == "phase":
        runs = fc.runs_of(fc.phase_plan(0.37, 1.0 / (nbin * 2.3), nbin, ndat), nbin)
    elif plan == "hand-gaps":
        pieces, t, i = [], 0, 0
        while t < ndat:
            n = min(ndat - t, (1, 7, 8, 9, 33, 63)[i % 6])
            pieces.append((None if i % 5 == 4 else (7 * i) % nbin, n))
            t += n
            i += 1
        runs, _ = fc.hand_runs(pieces)
    else:
        runs = fc.runs_of(fc.phase_plan(0.11, 1.0 / (nbin * 130.0), nbin, ndat), nbin)       # runs of 130 samples: the long-run kernel
        assert runs[:, 2].max() >= 64

    def fold_rows(rows, npol):
        f = dspsr_amd.FoldEngine(ctx)
        f.set_shape(nchan, npol, 1, nbin)
        f.set_nbin(nbin)
        f.set_ndat(ndat, 0)
        for off, b, n in runs:
            for i in range(int(off), int(off + n)):
                f.set_bin(i, float(b))
        f.fold(rows)
        out = f.synch()
        f.close()
        return out

    both = fold_rows(det, 2)
    assert both.shape == (nchan, 2, nbin, 1) and np.abs(both).max() > 0
    if plan != "long-runs":                      # (the long-run association depends on the number of rows: fold_plan.h fold_long_segments)
        for q in range(2):
            assert np.array_equal(both[:, q:q + 1], fold_rows(det[:, q:q + 1, :], 1))
        assert np.array_equal(both, fold_time_order(det.cpu().numpy()[..., None], runs, np.zeros_like(both)))
    else:
        assert np.array_equal(both, fold_long_model(det.cpu().numpy()[..., None], runs, np.zeros_like(both), nchan * 2, ncu))
        for q in range(2):
            one = fold_rows(det[:, q:q + 1, :], 1)
            assert np.array_equal(one, fold_long_model(det.cpu().numpy()[:, q:q + 1, :, None], runs, np.zeros_like(one), nchan, ncu))


# ---- 5. one polarisation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", [True, False])
def test_one_polarisation_folds_its_power(gpu, oracle, real):
    dspsr_amd, ctx, ncu = gpu
    C, M, nfilt, parts, nbin = 16, 256, (20, 21), 3, 32
    nkeep = M - sum(nfilt)
    ndat = parts * nkeep
    eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, nfilt[0], nfilt[1], 1, 1, real, _kernel(C * M), max_parts=2,
                                                fused_fold=dspsr_amd.FUSED_ALWAYS)
    assert eng.fold_is_fused(dspsr_amd.INTENSITY) == 1           # fused: the store's one-polarisation branch (real and complex input)
    nsamp = (2 if real else 1) * C * (parts * nkeep + sum(nfilt))
    raw = torch.from_numpy(_raw(nsamp * (1 if real else 2), 21)).cuda()
    cplx = torch.zeros((C, 1, 2 * ndat), dtype=torch.float32, device="cuda")
    eng.perform_raw(raw, dspsr_amd.RAW_GENERIC, S8, cplx, parts)
    fb = cplx.cpu().numpy().reshape(C, 1, ndat, 2)
    want = oracle.square_law((fb[..., 0] + 1j * fb[..., 1]).astype(np.complex64), "Intensity").astype(np.float32)
    det = torch.zeros((C, 1, ndat), dtype=torch.float32, device="cuda")
    eng.perform_detect(det, parts, dspsr_amd.INTENSITY, 1, raw=raw, scale=S8)
    assert np.abs(want).max() > 0 and np.array_equal(det.cpu().numpy().view(np.int32), want.view(np.int32))
    fold = dspsr_amd.FoldEngine(ctx)
    fold.set_shape(C, 1, 1, nbin)
    hits = np.zeros(nbin, np.uint32)
    fold.set_nbin(nbin)
    fold.set_ndat(ndat, 0)
    pps = 1.0 / (nbin * 1.9)
    fold.set_bins(0.2, pps, ndat, 0, hits)
    eng.perform_fold(fold, parts, dspsr_amd.INTENSITY, raw=raw, scale=S8)
    runs = fc.runs_of(fc.phase_plan(0.2, pps, nbin, ndat), nbin)
    assert np.array_equal(fold.synch(), fold_time_order(want[..., None], runs, np.zeros((C, 1, nbin, 1), np.float32)))
    with pytest.raises(dspsr_amd.DspsrAmdError, match="PPQQ needs two polarisations"):
        eng.perform_detect(torch.zeros((C, 2, ndat), dtype=torch.float32, device="cuda"), parts, dspsr_amd.PPQQ, 1, raw=raw, scale=S8)
    f2 = dspsr_amd.FoldEngine(ctx)
    f2.set_shape(C, 2, 1, nbin)
    f2.set_nbin(nbin)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="PPQQ needs two polarisations"):
        eng.perform_fold(f2, parts, dspsr_amd.PPQQ, raw=raw, scale=S8)
    eng.close()
    fold.close()
    f2.close()
