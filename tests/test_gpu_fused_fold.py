"""dspsr_amd_filterbank_perform_fold at every branch of its plan, bit for bit: the cases of tests/fused_fold_cases.py (their
records are checked without a GPU by tests/test_fused_fold_cases_host.py) against tests/fold_reference.py fused_fold_model.

The detected samples come from perform_detect of the same object on the same block (that the fused kernels detect the same bits
is what test_fused_fold_bit_identical and test_two_pass_fused_fold_bit_identical establish); the model adds them in the order the
kernels do.  Every comparison is np.array_equal; the one tolerance is the segment-sum plan's (2e-6 of the maximum against a
float64 fold, the bound of test_four_pass_fused_fold_segment_sums)."""
import numpy as np
import pytest

import fused_fold_cases as fc
from fold_reference import fold_long_model, fold_time_order, fused_fold_model

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S8 = 1.0 / 48.0          # any scale: detection and fold see the same products


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx, torch.cuda.get_device_properties(0).multi_processor_count
    ctx.close()


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.standard_normal(n) * 24.0), -128, 127).astype(np.int8)


def _shape(c):
    nchan = c["input_nchan"] * c["C"]
    return (nchan, 2, c["nbin"], 2) if c["prof"] == "2x2" else (nchan, 1, c["nbin"], 4)


def _set_plan(fold, c, k, hits):
    """the plan of call k: set_bins for the phase law, set_bin sample by sample for a hand-made plan"""
    runs, table_hits, ndat = fc.call_runs(c["name"], k)
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
    """the case on the device: (fold_is_fused(), hits, profile [chan][npol][nbin][ndim], detected samples per call, the floats
    around a bound profile's rows as bits before and after)"""
    dspsr_amd, ctx, _ncu = gpu
    c = fc.by_name(name)
    C, M, inch = c["C"], c["M"], c["input_nchan"]
    nkeep = M - sum(c["nfilt"])
    nchan, npol, nbin, ndim = _shape(c)
    kernel = np.exp(1j * np.random.default_rng(17).uniform(-np.pi, np.pi, inch * C * M)).astype(np.complex64)
    eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, c["nfilt"][0], c["nfilt"][1], inch, 2, c["real"], kernel,
                                                max_parts=max_parts or c["max_parts"], force_four_pass=c["four"], fused_fold=c["policy"])
    assert eng.nkeep == nkeep
    mode = eng.fold_is_fused()
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
    state = dspsr_amd.COHERENCE
    for k, (parts, _plan) in enumerate(c["calls"]):
        raw = torch.from_numpy(_raw(fc.raw_bytes(c, parts), 1000 + 10 * fc.NAMES.index(name) + k)).cuda()
        det = torch.zeros((nchan, 1, 4 * parts * nkeep), dtype=torch.float32, device="cuda")
        eng.perform_detect(det, parts, state, 4, raw=raw, scale=S8)
        _set_plan(fold, c, k, hits)
        eng.perform_fold(fold, parts, state, raw=raw, scale=S8)
        dets.append(det.view(nchan, parts * nkeep, 4).cpu().numpy())
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
    """(per-bin hits, profile) the calls must leave, from the path the restated dispatcher names for every call"""
    c = fc.by_name(name)
    rec = fc.record(name, ncu)
    nchan, npol, nbin, ndim = _shape(c)
    nkeep = c["M"] - sum(c["nfilt"])
    prof = np.zeros((nchan, npol, nbin, ndim), np.float32)
    hits = np.zeros(nbin, np.uint32)
    for k, call in enumerate(rec["calls"]):
        runs, h, ndat = fc.call_runs(name, k)
        hits += h
        if call["path"] == "fused":
            nseg = {l["ns"]: l["nseg"] for l in call["launches"]}
            prof = fused_fold_model(dets[k], runs, prof, nkeep, [l["ns"] for l in call["launches"]], rec["mode"], nseg.__getitem__)
        else:
            # Detection + Fold: rows [chan][pol][ndat][ndim] of the profile's shape
            rows = dets[k].reshape(nchan, ndat, npol, ndim).transpose(0, 2, 1, 3)
            prof = fold_long_model(rows, runs, prof, nchan * npol, ncu) if call["assoc"] == "long" else fold_time_order(rows, runs, prof)
    return hits, prof


def _check(gpu, name, **kw):
    mode, hits, prof, dets, (pad, after) = _run(gpu, name, **kw)
    ncu = gpu[2]
    assert mode == fc.record(name, ncu)["mode"], "fold_is_fused() is not the mode of the table (device of %d compute units)" % ncu
    want_hits, want = _model(name, dets, ncu)
    assert np.array_equal(hits, want_hits)
    assert np.abs(want).max() > 0
    bad = np.argwhere(prof.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, "%s: %d sums differ from the model, first at (chan, pol, bin, dim) = %s: %r != %r" % (
        name, len(bad), tuple(bad[0]), prof[tuple(bad[0])], want[tuple(bad[0])])
    if pad is not None:
        assert np.array_equal(pad, after), "a float outside the bound profile's rows changed"
    return prof


@pytest.mark.parametrize("name", fc.of_group("psl"))
def test_part_offsets_in_lds_and_in_global_memory(gpu, name):
    """one exact launch of 127 parts (fnp + 1 = FB_PSL_MAX: offsets in LDS, entries by DMA, prefetched accumulators), of 128 and
    of 130 (offsets and entries from global memory): the model, and the same stream folded two parts per launch"""
    prof = _check(gpu, name)
    assert np.array_equal(prof, _run(gpu, name, max_parts=2)[2])


@pytest.mark.parametrize("name", fc.of_group("seg"))
def test_segmented_launches(gpu, name):
    """fold_is_fused() == 2: run 0 onto the profile, the other runs from zero, added in run order; ragged and empty runs, fewer
    parts than runs, the cap of 16 runs, both profile shapes, two and three passes, one and three input channels; twice"""
    prof = _check(gpu, name)
    assert np.array_equal(prof, _run(gpu, name)[2])


@pytest.mark.parametrize("name", fc.of_group("cap") + fc.of_group("runs") + fc.of_group("grid"))
def test_inside_a_tile(gpu, name):
    """active bins either side of plan_cap and of the workgroup's threads; first intervals around the 8-sample loop, bins
    revisited in a part, an empty part in the middle of a launch, the longest fused run and the first one that is not; exact
    launches whose workgroups walk two tiles"""
    _check(gpu, name)


@pytest.mark.parametrize("name", fc.of_group("placement"))
def test_bound_profiles(gpu, name):
    """bound profiles with row spans that are a multiple of 4, even and odd, and one float past an aligned address: fused or
    Detection + Fold as the dispatcher decides, the same sums, and the NaN around the rows untouched"""
    _check(gpu, name)


@pytest.mark.parametrize("name", fc.of_group("segsum"))
def test_segment_sum_qualification(gpu, name):
    """fold_is_fused() == 3 (four passes, 4 channels x 16384): inner intervals of exactly one segment qualify for the segment
    sums -- the project's bound for them, 2e-6 of the maximum against a float64 fold --; one inner interval a sample shorter, or
    a plan one sample short of the call, take Detection + Fold: the same bits as perform_detect + fold"""
    dspsr_amd, ctx, ncu = gpu
    c = fc.by_name(name)
    rec = fc.record(name, ncu)
    mode, hits, prof, dets, _ = _run(gpu, name)
    runs, table_hits, ndat = fc.call_runs(name, 0)
    assert mode == rec["mode"] == 3 and np.array_equal(hits, table_hits)
    if rec["calls"][0]["path"] == "segsum":
        want = np.zeros(prof.shape, np.float64)
        for off, b, n in runs:
            want[:, 0, b, :] += dets[0][:, off:off + n, :].astype(np.float64).sum(axis=1)
        err = np.abs(prof - want).max() / np.abs(want).max()
        print("%s: segment sums against the float64 fold: %.3g of the maximum" % (name, err))
        assert err <= 2e-6
    else:
        sep = dspsr_amd.FoldEngine(ctx)
        sep.set_shape(*[_shape(c)[i] for i in (0, 1, 3, 2)])
        _set_plan(sep, c, 0, np.zeros(c["nbin"], np.uint32))
        sep.fold(torch.from_numpy(dets[0].reshape(c["C"], 1, -1)).cuda())
        want = sep.synch()
        sep.close()
        assert np.abs(want).max() > 0 and np.array_equal(prof, want)
        assert np.array_equal(want, fold_long_model(dets[0][:, None], runs, np.zeros_like(want), c["C"], ncu))


def test_refusals_leave_the_profile_and_the_objects_usable(gpu):
    """a plan sample beyond the parts of the call: DSPSR_AMD_EINVAL, profile untouched; npart == 0: OK, nothing changes; a correct
    call on the same objects then folds what the model says"""
    dspsr_amd, ctx, ncu = gpu
    name = "psl-127-4"
    c = fc.by_name(name)
    C, M, nbin = c["C"], c["M"], c["nbin"]
    nkeep = M - sum(c["nfilt"])
    eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, c["nfilt"][0], c["nfilt"][1], 1, 2, True, None, max_parts=2, fused_fold=dspsr_amd.FUSED_ALWAYS)
    fold = dspsr_amd.FoldEngine(ctx)
    fold.set_shape(C, 1, 4, nbin)
    want = np.zeros((C, 1, nbin, 4), np.float32)
    pps = 1.0 / (nbin * 1.7)

    def call(parts, plan_parts, seed):
        raw = torch.from_numpy(_raw(fc.raw_bytes(c, max(parts, 1)), seed)).cuda()
        det = torch.zeros((C, 1, 4 * max(parts, 1) * nkeep), dtype=torch.float32, device="cuda")
        eng.perform_detect(det, max(parts, 1), dspsr_amd.COHERENCE, 4, raw=raw, scale=S8)
        fold.set_nbin(nbin)
        fold.set_ndat(plan_parts * nkeep, 0)
        fold.set_bins(0.3, pps, plan_parts * nkeep, 0, None)
        eng.perform_fold(fold, parts, dspsr_amd.COHERENCE, raw=raw, scale=S8)
        return det.view(C, -1, 4).cpu().numpy()

    def good(seed):
        det = call(3, 3, seed)
        runs = fc.runs_of(fc.phase_plan(0.3, pps, nbin, 3 * nkeep), nbin)
        return fused_fold_model(det, runs, want, nkeep, [2, 1], 1)

    want = good(1)
    assert np.array_equal(fold.synch(), want) and np.abs(want).max() > 0
    with pytest.raises(dspsr_amd.DspsrAmdError, match=r"\(-1\).*beyond the 2 parts"):           # DSPSR_AMD_EINVAL
        call(2, 3, 2)
    assert np.array_equal(fold.synch(), want)
    want = good(3)
    assert np.array_equal(fold.synch(), want)
    call(0, 0, 4)                                  # npart == 0 (and no plan): OK
    assert np.array_equal(fold.synch(), want)
    want = good(5)
    assert np.array_equal(fold.synch(), want)
    eng.close()
    fold.close()
