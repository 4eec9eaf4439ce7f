"""Every kernel of the stand-alone fold (dspsr_amd_fold_fold / _fold_zeroed, csrc/fold.hip) at the addresses, strides, plans and
profiles the C-ABI accepts, bit for bit against tests/fold_reference.py.

fold_fold_impl picks its kernel from the call: the input's alignment and strides (`aligned`), nbin (`chunked`), the longest
run (`lng`, FOLD_LONG_RUN), the dense table (plan_scan of fold_plan.h), the bin split (`nsplit`, `threads`), the rows per
workgroup (`nrw`) and, for LONG runs, the time segments (`nseg`, `cps`).  Each case states the branch it is there for, and fold_reference.fold_dispatch -- the same choice restated
-- asserts that it reaches it.  Rows are placed by device_buffers.device_rows (an offset from a 256-byte boundary, padded rows,
NaN everywhere else) and the profiles are asserted finite.  k_fold_direct, k_fold_chunked<., false, .> and k_fold_dense add in
time order (fold_time_order); the LONG path (k_fold_chunked<., true, .> + k_fold_combine) adds in the association fold_long_model
states, which depends on the device's compute units: both are compared bit for bit, LONG also against float64.
The expected launch shapes (NROW, nsplit, threads, the LONG segment count) are worked out for the MI355X's 256 compute units:
NROW > 1 needs nchan * nsplit >= 2 * ncu (520 channels here) and the segment count follows from ncu and nchan * npol.  On a
device with another CU count the dispatch assertions of those cases fail and name the difference; the references themselves
take the device's ncu.
"""
import math

import numpy as np
import pytest

from fold_reference import FOLD_CHUNK, fold_dispatch, fold_long_model, fold_time_order, plan_span, runs_of_plan
from device_buffers import device_rows as _device_rows

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


def _data(rng, nchan, npol, ndat, ndim):
    return (rng.standard_normal((nchan, npol, ndat, ndim)) ** 2 + rng.random((nchan, npol, ndat, ndim))).astype(np.float32)


def _hand_plan(rng, nbin, n, lo, hi):
    """per-sample bins of runs with random lengths in [lo, hi] (at least one of exactly hi) and random bins, each unlike the
    bin before it"""
    lens = [int(rng.integers(lo, hi + 1)), hi]
    while sum(lens) < n:
        lens.append(int(rng.integers(lo, hi + 1)))
    lens[-1] -= sum(lens) - n
    assert lens[-1] > 0 and max(lens) == hi
    plan, b = [], -1
    for k in lens:
        nb = int(rng.integers(0, nbin - 1)) if nbin > 1 else 0
        b = nb + (nb >= b) if b >= 0 and nbin > 1 else nb
        plan += [b] * k
    return np.array(plan, np.uint32)


def _recur_phi(phi, pps, n):
    """phi after n samples of the plan recurrence (Fold.C:744-787): where a plan that continues this one starts"""
    for _ in range(n):
        phi -= math.floor(phi)
        phi += pps
    return phi


def _feed(eng, oracle, nbin, idat_start, spec):
    """one plan handed to the engine: spec ("bins", phi, pps, n) goes through set_bins, ("bin", plan) through set_bin sample by
    sample.  Returns the per-sample plan; asserts hits and ndat_folded."""
    if spec[0] == "bins":
        _, phi, pps, n = spec
        hits = np.zeros(nbin, np.uint32)
        assert eng.set_bins(phi, pps, n, idat_start, hits) == n
        plan = oracle.fold_binplan(phi, pps, nbin, n)
        assert np.array_equal(hits, np.bincount(plan, minlength=nbin).astype(np.uint32))
        return plan
    plan = spec[1]
    for i, b in enumerate(plan.tolist()):
        eng.set_bin(idat_start + i, float(b))
    return plan


def _reference(kind, x, runs, prof, ncu):
    nchan, npol = x.shape[:2]
    return fold_long_model(x, runs, prof, nchan * npol, ncu) if kind == "long" else fold_time_order(x, runs, prof)


def _check_f64(got, x, runs, prof0, nfold):
    want = prof0.astype(np.float64)
    for _ in range(nfold):
        for off, b, n in runs:
            want[:, :, b, :] += x[:, :, off:off + n, :].astype(np.float64).sum(axis=2)
    assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()


def _run(gpu, oracle, nchan, npol, ndim, nbin, ndat, idat_start, spec, expect, offset=0, row_pad=0, nfold=1, seed=1):
    """fold the same plan `nfold` times (the later folds into a profile that holds sums), against the reference of the kernel
    `expect` names; returns (runs, dispatch)"""
    dspsr_amd, ctx, ncu = gpu
    rng = np.random.default_rng(seed)
    x = _data(rng, nchan, npol, ndat, ndim)
    d = _device_rows(x.reshape(nchan, npol, ndat * ndim), offset, row_pad)
    eng = dspsr_amd.FoldEngine(ctx)
    eng.set_shape(nchan, npol, ndim, nbin)
    want = np.zeros((nchan, npol, nbin, ndim), np.float32)
    for _ in range(nfold):
        eng.set_nbin(nbin)
        n = spec[3] if spec[0] == "bins" else spec[1].size
        eng.set_ndat(n, idat_start)
        plan = _feed(eng, oracle, nbin, idat_start, spec)
        assert eng.get_ndat_folded() == plan.size
        runs = runs_of_plan(plan, idat_start)
        disp = fold_dispatch(d.data_ptr(), d.stride(0), d.stride(1), nchan, npol, ndim, nbin, runs, ncu)
        assert {k: disp[k] for k in expect} == expect, (disp, "expectations worked out for 256 CUs, device has %d" % ncu)
        eng.fold(d)
        want = _reference(disp["kernel"], x, runs, want, ncu)
    got = eng.synch()
    eng.close()
    assert np.isfinite(got).all()
    assert np.array_equal(got, want)
    if expect["kernel"] == "long":
        _check_f64(got, x, runs, np.zeros_like(want), nfold)
    return runs, disp


# ---- 1. k_fold_direct<1|2|4> with nbin <= 4096: unaligned rows (fold_fold_impl: `aligned` false, the k_fold_direct branch) ----------
# (offset, row_pad, ndim, npol, nchan, nbin, samples per bin, nsplit): offsets 1-3 break the 16-byte address, row_pad 1 and 3
# the strides; nsplit > 1 where few rows meet nbin >= 128 (`nsplit`); runs shorter and longer than FOLD_LONG_RUN (always time order)
@pytest.mark.parametrize("offset,row_pad,ndim,npol,nchan,nbin,spb,nsplit", [
    (1, 0, 4, 1, 3, 256, 9.3, 4),
    (2, 0, 2, 2, 5, 64, 200.5, 1),
    (3, 0, 1, 4, 2, 1000, 3.7, 8),
    (0, 1, 1, 4, 4, 256, 150.0, 4),
    (0, 3, 2, 2, 3, 4096, 2.2, 8),
    (1, 3, 4, 1, 7, 128, 70.0, 2),
])
def test_direct_unaligned_rows(oracle, gpu, offset, row_pad, ndim, npol, nchan, nbin, spb, nsplit):
    ndat, i0 = 20010, 5                                         # (ndat * ndim + row_pad: odd strides)
    runs, _ = _run(gpu, oracle, nchan, npol, ndim, nbin, ndat, i0, ("bins", 0.29, 1.0 / (spb * nbin), ndat - i0 - 3),
                   dict(kernel="direct", ndim=ndim, nsplit=nsplit), offset=offset, row_pad=row_pad, nfold=2)
    assert (runs[:, 2].max() >= 64) == (spb > 64)


# ---- 2. k_fold_chunked<., false, .>: aligned, longest run < 64 (`lng` false), not dense (plan_scan refuses) ----------------------
# every instantiation (NDIM, NROW) = (4,1) (2,1) (2,2) (1,1) (1,4); nsplit 1/2/4/8 and 256/512/1024 threads (`nsplit`, `threads`); hand-made
# plans with a longest run of exactly 63, runs across chunk ends, a first sample that is not a multiple of 4 (`first -= first % 4`) and a ragged
# last chunk ((last - first) * ndim not a multiple of 4: the scalar tail of the chunk loads)
@pytest.mark.parametrize("name,nchan,npol,ndim,nbin,ndat,i0,plan,nrow,nsplit,threads", [
    ("4x1-split8-hand63", 2, 1, 4, 512, 20000, 13, ("hand", 1, 63), 1, 8, 256),
    ("2x1-split8", 40, 1, 2, 4096, 16000, 6, ("spb", 0.3), 1, 8, 256),
    ("2x2-rows", 520, 2, 2, 2048, 6000, 3, ("spb", 0.7), 2, 1, 512),
    ("1x1-1024-ragged", 600, 1, 1, 4096, 20000, 1, ("spb", 0.45), 1, 1, 1024),
    ("1x4-rows-hand63", 520, 4, 1, 100, 5000, 9, ("hand", 1, 63), 4, 1, 256),
    ("4x1-split4", 130, 1, 4, 1024, 6000, 2, ("spb", 1.1), 1, 4, 256),
    ("4x1-split2-512", 300, 1, 4, 4096, 3000, 0, ("spb", 0.3), 1, 2, 512),
])
def test_chunked_exact_instantiations(oracle, gpu, name, nchan, npol, ndim, nbin, ndat, i0, plan, nrow, nsplit, threads):
    rng = np.random.default_rng(7)
    n = ndat - i0 - 2
    spec = ("bin", _hand_plan(rng, nbin, n, plan[1], plan[2])) if plan[0] == "hand" else ("bins", 0.71, 1.0 / (plan[1] * nbin), n)
    runs, disp = _run(gpu, oracle, nchan, npol, ndim, nbin, ndat, i0, spec,
                      dict(kernel="chunked", ndim=ndim, nrow=nrow, nsplit=nsplit, threads=threads), nfold=2)
    first, last = plan_span(runs)
    assert runs[:, 2].max() < 64
    if plan[0] == "hand":                                       # runs across chunk ends, the first sample off the 4-sample grid
        assert runs[:, 2].max() == 63 and runs[0, 0] % 4 != 0
        assert ((runs[:, 0] - first) // FOLD_CHUNK != (runs[:, 0] + runs[:, 2] - 1 - first) // FOLD_CHUNK).any()
    if name.endswith("ragged"):
        assert (last - first) * ndim % 4 != 0


# ---- 3. k_fold_dense (one run per (chunk, bin): plan_scan), every instantiation; and the neighbours it refuses ------------------
@pytest.mark.parametrize("nchan,npol,ndim,ndat,nrow", [
    (6, 1, 4, 20000, 1), (4, 1, 2, 20000, 1), (520, 2, 2, 4100, 2), (3, 1, 1, 20000, 1), (520, 4, 1, 4100, 4)])
def test_dense_instantiations(oracle, gpu, nchan, npol, ndim, ndat, nrow):
    nbin = 64                                                   # 40.3 samples per bin: a period of 2579 > FOLD_CHUNK samples
    _run(gpu, oracle, nchan, npol, ndim, nbin, ndat, 7, ("bins", 0.52, 1.0 / (40.3 * nbin), ndat - 9),
         dict(kernel="dense", ndim=ndim, nrow=nrow), nfold=2)


def test_dense_refuses_a_second_run_in_a_chunk(oracle, gpu):
    """the same plan with two samples of one run moved to a bin that already has a run in that chunk (plan_scan's `lastc`): chunked, and both
    sides in time order"""
    nchan, npol, ndim, nbin, ndat, i0 = 6, 1, 4, 64, 20000, 7
    base = oracle.fold_binplan(0.52, 1.0 / (40.3 * nbin), nbin, ndat - 9)
    _run(gpu, oracle, nchan, npol, ndim, nbin, ndat, i0, ("bin", base), dict(kernel="dense", ndim=4))
    mod = base.copy()
    k = 5 * FOLD_CHUNK + 1500                                   # chunk 5 holds plan samples [5 * 2048 - 3, 6 * 2048 - 3)
    other = [b for b in np.unique(mod[5 * FOLD_CHUNK:k - 100]) if b != mod[k]][0]
    mod[k:k + 2] = other
    runs, _ = _run(gpu, oracle, nchan, npol, ndim, nbin, ndat, i0, ("bin", mod), dict(kernel="chunked", ndim=4))
    assert (runs[:, 1] == other).sum() > (runs_of_plan(base, i0)[:, 1] == other).sum()


@pytest.mark.parametrize("nchan,kernel", [(1, "chunked"), (2, "dense")])
def test_dense_refuses_a_table_larger_than_a_quarter_of_the_data(oracle, gpu, nchan, kernel):
    """one row of one float per sample, 600 bins of 4 samples (a period of 2400 > FOLD_CHUNK): 4 * ntab > data words (plan_scan)
    refuses the table; two rows take it"""
    _run(gpu, oracle, nchan, 1, 1, 600, 24000, 4, ("bins", 0.1, 1.0 / (4.0 * 600), 23990), dict(kernel=kernel, ndim=1))


# ---- 4. LONG: k_fold_chunked<., true, .> + k_fold_combine (`lng` true), every instantiation ------------------------------------
# hand-made plans with a longest run of exactly 64 (FOLD_LONG_RUN), folded twice (the second into a profile holding sums: the order
# of k_fold_combine shows even with one segment); nseg == 1 and nseg >= 3 (`nseg`, `cps`), runs across segment ends, bins that get
# nothing in some segment
@pytest.mark.parametrize("nchan,npol,ndim,ndat,nrow,nseg", [
    (3, 1, 4, 12000, 1, 6),
    (2, 1, 4, 2000, 1, 1),
    (200, 1, 2, 40000, 1, 5),
    (200, 2, 2, 12000, 2, 3),
    (1, 1, 1, 30000, 1, 15),
    (1100, 1, 1, 6000, 1, 1),
    (520, 4, 1, 5000, 4, 1),
])
def test_long_instantiations_bit_exact(oracle, gpu, nchan, npol, ndim, ndat, nrow, nseg):
    nbin, i0 = 64, 3
    plan = _hand_plan(np.random.default_rng(nchan + ndat), nbin, ndat - i0 - 5, 1, 64)
    runs, disp = _run(gpu, oracle, nchan, npol, ndim, nbin, ndat, i0, ("bin", plan),
                      dict(kernel="long", ndim=ndim, nrow=nrow, nseg=nseg), nfold=2, seed=nchan)
    assert runs[:, 2].max() == 64
    first, _ = plan_span(runs)
    seg_of = lambda s: (s - first) // FOLD_CHUNK // disp["cps"]
    if nseg > 1:
        assert (seg_of(runs[:, 0]) != seg_of(runs[:, 0] + runs[:, 2] - 1)).any()          # a run across a segment end
        got = np.zeros((nseg, nbin), bool)
        for off, b, n in runs:
            got[seg_of(off):seg_of(off + n - 1) + 1, b] = True
        assert not got.all()                                                             # a bin without samples in a segment


def test_long_wide_bins_bit_exact(oracle, gpu):
    """test_fold_long_runs_reassociated's plan (1090.7 samples per bin, set_bins' run-by-run path) bit for bit"""
    ndat, i0 = 50000, 37
    _run(gpu, oracle, 3, 1, 4, 16, ndat, i0, ("bins", 0.13, 1.0 / (16 * 1090.7), ndat - 100), dict(kernel="long", ndim=4), nfold=2)


# ---- 5. nbin 4096 (aligned: dense or chunked) against 4097 (`chunked` false: direct) --------------------------------------------
@pytest.mark.parametrize("nbin,kernel", [(4096, "dense"), (4097, "direct")])
def test_nbin_4096_and_4097(oracle, gpu, nbin, kernel):
    ndat = 20000
    _run(gpu, oracle, 8, 1, 4, nbin, ndat, 0, ("bins", 0.4, 1.0 / (1.3 * nbin), ndat), dict(kernel=kernel, ndim=4))


# ---- the four families on one small shape (nchan 5, npol 2, ndim 2, nbin 64) -------------------------------------------------
FAMILIES = {
    "direct": dict(offset=1, spec=lambda rng, n: ("bins", 0.3, 1.0 / (9.0 * 64), n)),
    "chunked": dict(offset=0, spec=lambda rng, n: ("bins", 0.3, 1.0 / (3.0 * 64), n)),
    "dense": dict(offset=0, spec=lambda rng, n: ("bins", 0.3, 1.0 / (40.3 * 64), n)),
    "long": dict(offset=0, spec=lambda rng, n: ("bin", _hand_plan(rng, 64, n, 1, 64))),
}


# ---- 6. fold_zeroed through each family: k_fold_count_hits next to the fold (end of fold_fold_impl) ------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_fold_zeroed_each_family(oracle, gpu, family):
    """hits per channel = planned samples whose first float of polarisation 0 is not zero; the profile is the plain fold's"""
    dspsr_amd, ctx, ncu = gpu
    nchan, npol, ndim, nbin, ndat, i0 = 5, 2, 2, 64, 9000, 6
    rng = np.random.default_rng(11)
    x = _data(rng, nchan, npol, ndat, ndim)
    for c in range(nchan):
        x[c, :, rng.random(ndat) < 0.1 * (c + 1)] = 0.0
    fam = FAMILIES[family]
    spec = fam["spec"](rng, ndat - i0 - 4)
    d = _device_rows(x.reshape(nchan, npol, ndat * ndim), fam["offset"], 0)
    hits_dev = torch.zeros((nchan, nbin), dtype=torch.int32, device="cuda")
    z, p = dspsr_amd.FoldEngine(ctx), dspsr_amd.FoldEngine(ctx)
    for e in (z, p):
        e.set_shape(nchan, npol, ndim, nbin)
        e.set_nbin(nbin)
        e.set_ndat(ndat - i0 - 4, i0)
        plan = _feed(e, oracle, nbin, i0, spec)
    runs = runs_of_plan(plan, i0)
    assert fold_dispatch(d.data_ptr(), d.stride(0), d.stride(1), nchan, npol, ndim, nbin, runs, ncu)["kernel"] == family
    z.fold_zeroed(d, hits_dev)
    p.fold(d)
    want_hits = np.zeros((nchan, nbin), np.int64)
    for c in range(nchan):
        np.add.at(want_hits[c], plan, (x[c, 0, i0:i0 + plan.size, 0] != 0).astype(np.int64))
    got = z.synch()
    assert np.array_equal(hits_dev.cpu().numpy().astype(np.int64), want_hits) and want_hits.sum() < nchan * plan.size
    assert np.isfinite(got).all() and np.array_equal(got, p.synch())
    assert np.array_equal(got, _reference(family, x, runs, np.zeros_like(got), ncu))
    z.close()
    p.close()


# ---- 7. profiles bound to a caller's buffer (dspsr_amd_fold_bind_profile): padded rows at an odd float offset ---------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_bound_profile_each_family(oracle, gpu, family):
    dspsr_amd, ctx, ncu = gpu
    nchan, npol, ndim, nbin, ndat, i0 = 3, 2, 2, 64, 9000, 6
    span, base = nbin * ndim + 3, 5
    nrow = nchan * npol
    rng = np.random.default_rng(12)
    x = _data(rng, nchan, npol, ndat, ndim)
    fam = FAMILIES[family]
    spec = fam["spec"](rng, ndat - i0 - 4)
    d = _device_rows(x.reshape(nchan, npol, ndat * ndim), fam["offset"], 0)
    buf = torch.full((64 + base + nrow * span + 64,), float("nan"), dtype=torch.float32, device="cuda")
    lead = ((-buf.data_ptr()) % 256) // 4
    prof = buf[lead + base:lead + base + nrow * span].view(nrow, span)
    assert prof.data_ptr() % 8 == 4
    p0 = rng.standard_normal((nchan, npol, nbin, ndim)).astype(np.float32)
    prof[:, :nbin * ndim] = torch.from_numpy(p0.reshape(nrow, nbin * ndim)).cuda()
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[lead + base:lead + base + nrow * span].view(nrow, span)[:, :nbin * ndim] = True

    eng = dspsr_amd.FoldEngine(ctx)
    eng.bind_profile(prof, nchan, npol, ndim, nbin)
    eng.set_nbin(nbin)
    eng.set_ndat(ndat - i0 - 4, i0)
    plan = _feed(eng, oracle, nbin, i0, spec)
    runs = runs_of_plan(plan, i0)
    assert fold_dispatch(d.data_ptr(), d.stride(0), d.stride(1), nchan, npol, ndim, nbin, runs, ncu)["kernel"] == family
    eng.fold(d)
    want = _reference(family, x, runs, p0, ncu)
    packed = eng.synch()                                                     # packed [chan][pol][nbin][ndim]
    assert np.isfinite(packed).all() and np.array_equal(packed, want)
    b = buf.cpu().numpy()
    assert np.isnan(b[~inside.cpu().numpy()]).all()                          # padding and guards untouched
    assert np.array_equal(prof[:, :nbin * ndim].cpu().numpy().reshape(want.shape), want)
    eng.set_shape(nchan, npol, ndim, nbin)                                   # the bound shape: accepted
    with pytest.raises(dspsr_amd.DspsrAmdError, match=r"\(-4\)"):
        eng.set_shape(nchan, npol, ndim, nbin * 2)                           # another shape: ESTATE
    eng.zero()                                                               # the rows only
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert not b[inside.cpu().numpy()].any() and np.isnan(b[~inside.cpu().numpy()]).all()
    assert not eng.synch().any()
    eng.bind_profile(None, nchan, npol, ndim, nbin)                          # back to a library-owned (zeroed) profile
    eng.set_nbin(nbin)
    eng.set_ndat(ndat - i0 - 4, i0)
    plan = _feed(eng, oracle, nbin, i0, spec)
    eng.fold(d)
    got = eng.synch()
    assert np.array_equal(got, _reference(family, x, runs, np.zeros_like(p0), ncu))
    b2 = buf.cpu().numpy()
    assert np.array_equal(b2, b, equal_nan=True)                             # the caller's buffer is no longer written
    eng.close()


# ---- 8. several folds on one engine, no host sync between them: both plan slots (slot_acquire) and the LONG partial sums (f->part) ---
def _slot_cap(niv):
    """the interval capacity slot_reserve gives a slot it grows for niv intervals (fold.hip slot_reserve)"""
    return niv + niv // 2 + 16


def test_fold_sequence_reuses_plan_slots(oracle, gpu):
    """six folds issued back to back -- every input uploaded and every plan worked out before the first, nothing in between
    waits for the device -- cycling dense, LONG, direct, chunked, LONG, dense.  Folds alternate between the two plan slots, so
    each slot is refilled while the other's fold may still run.  The plans grow so that slot 0 is regrown at steps 3 and 5, and
    slot 1 at step 4 (intervals) and step 6 (its first dense table).  The second LONG fold has more time segments than the
    partial-sum buffer holds.  The profile is the per-step references applied in order."""
    dspsr_amd, ctx, ncu = gpu
    nchan, npol, ndim, nbin = 8, 1, 4, 64
    rng = np.random.default_rng(13)
    #         family     ndat    offset  phi   samples per bin
    steps = [("dense", 20000, 0, 0.52, 40.3),
             ("long", 8000, 0, 0.11, 100.3),
             ("direct", 20000, 1, 0.10, 9.0),
             ("chunked", 20000, 0, 0.70, 3.0),
             ("long", 300000, 0, 0.45, 70.3),
             ("dense", 30000, 0, 0.33, 50.1)]
    prep = []
    for k, (family, ndat, offset, phi, spb) in enumerate(steps):
        x = _data(rng, nchan, npol, ndat, ndim)
        d = _device_rows(x.reshape(nchan, npol, ndat * ndim), offset, 0)
        i0, n = 4 + k, ndat - 10
        plan = oracle.fold_binplan(phi, 1.0 / (spb * nbin), nbin, n)
        runs = runs_of_plan(plan, i0)
        disp = fold_dispatch(d.data_ptr(), d.stride(0), d.stride(1), nchan, npol, ndim, nbin, runs, ncu)
        assert disp["kernel"] == family, (k, disp)
        prep.append((x, d, i0, n, phi, 1.0 / (spb * nbin), plan, runs, disp))
    # the growth the docstring names, from the run counts (slot k % 2 takes fold k)
    cap, grew = [0, 0], []
    for k, p in enumerate(prep):
        if len(p[7]) > cap[k % 2]:
            cap[k % 2] = _slot_cap(len(p[7]))
            grew.append(k + 1)
    assert {3, 4, 5} <= set(grew), grew
    assert prep[4][8]["nseg"] > prep[1][8]["nseg"] > 1
    eng = dspsr_amd.FoldEngine(ctx)
    eng.set_shape(nchan, npol, ndim, nbin)
    hits = [np.zeros(nbin, np.uint32) for _ in steps]
    torch.cuda.synchronize()                                                   # inputs and the zeroed profile are in place
    for k, (x, d, i0, n, phi, pps, plan, runs, disp) in enumerate(prep):
        eng.set_nbin(nbin)
        eng.set_ndat(n, i0)
        eng.set_bins(phi, pps, n, i0, hits[k])
        eng.fold(d)
    got = eng.synch()
    eng.close()
    want = np.zeros((nchan, npol, nbin, ndim), np.float32)
    for k, (x, d, i0, n, phi, pps, plan, runs, disp) in enumerate(prep):
        assert np.array_equal(hits[k], np.bincount(plan, minlength=nbin).astype(np.uint32)), k
        want = _reference(disp["kernel"], x, runs, want, ncu)
    assert np.isfinite(got).all() and np.array_equal(got, want)


# ---- 9. plans built across calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spb,family", [(5.0, "chunked"), (300.0, "long")])
def test_plan_from_two_set_bins_calls(oracle, gpu, spb, family):
    """two set_bins calls, the second continuing the phase of the first inside a run, then one fold: the run left open by the
    first call goes on (one run: for LONG, one micro-block walk), hits and ndat_folded count every sample once"""
    dspsr_amd, ctx, ncu = gpu
    nchan, npol, ndim, nbin, ndat, i0 = 4, 1, 4, 32, 30000, 3
    pps, phi = 1.0 / (spb * nbin), 0.21
    full = oracle.fold_binplan(phi, pps, nbin, ndat - i0 - 7)
    n1 = int(np.flatnonzero(np.diff(full.astype(np.int64)))[len(full) // int(2 * spb)]) - 2    # two samples before a bin change
    assert full[n1 - 1] == full[n1]
    x = _data(np.random.default_rng(14), nchan, npol, ndat, ndim)
    d = _device_rows(x.reshape(nchan, npol, ndat * ndim), 0, 0)
    eng = dspsr_amd.FoldEngine(ctx)
    eng.set_shape(nchan, npol, ndim, nbin)
    eng.set_nbin(nbin)
    eng.set_ndat(full.size, i0)
    hits = np.zeros(nbin, np.uint32)
    a = eng.set_bins(phi, pps, n1, i0, hits)
    b = eng.set_bins(_recur_phi(phi, pps, n1), pps, full.size - n1, i0 + n1, hits)
    assert a + b == full.size == eng.get_ndat_folded()
    assert np.array_equal(hits, np.bincount(full, minlength=nbin).astype(np.uint32))
    runs = runs_of_plan(full, i0)
    assert fold_dispatch(d.data_ptr(), d.stride(0), d.stride(1), nchan, npol, ndim, nbin, runs, ncu)["kernel"] == family
    eng.fold(d)
    got = eng.synch()
    eng.close()
    assert np.array_equal(got, _reference(family, x, runs, np.zeros_like(got), ncu))


@pytest.mark.parametrize("spb,family", [(5.0, "chunked"), (300.0, "long")])
def test_plan_after_a_fold_without_set_nbin(oracle, gpu, spb, family):
    """fold, then a plan that continues the phase without set_nbin and starts inside the bin the last plan ended in: the new
    plan opens a fresh run (fold.hip plan_close), so every sample counted in hits and ndat_folded is folded"""
    dspsr_amd, ctx, ncu = gpu
    nchan, npol, ndim, nbin, ndat, i0 = 4, 1, 4, 32, 30000, 3
    pps, phi = 1.0 / (spb * nbin), 0.21
    full = oracle.fold_binplan(phi, pps, nbin, ndat - i0 - 7)
    n1 = int(np.flatnonzero(np.diff(full.astype(np.int64)))[len(full) // int(2 * spb)]) - 2
    assert full[n1 - 1] == full[n1]
    x = _data(np.random.default_rng(15), nchan, npol, ndat, ndim)
    d = _device_rows(x.reshape(nchan, npol, ndat * ndim), 0, 0)
    eng = dspsr_amd.FoldEngine(ctx)
    eng.set_shape(nchan, npol, ndim, nbin)
    eng.set_nbin(nbin)
    eng.set_ndat(n1, i0)
    hits = np.zeros(nbin, np.uint32)
    eng.set_bins(phi, pps, n1, i0, hits)
    eng.fold(d)
    eng.set_ndat(full.size - n1, i0 + n1)
    eng.set_bins(_recur_phi(phi, pps, n1), pps, full.size - n1, i0 + n1, hits)
    eng.fold(d)
    got = eng.synch()
    assert eng.get_ndat_folded() == full.size
    assert np.array_equal(hits, np.bincount(full, minlength=nbin).astype(np.uint32))
    eng.close()
    r1, r2 = runs_of_plan(full[:n1], i0), runs_of_plan(full[n1:], i0 + n1)
    for r in (r1, r2):
        assert fold_dispatch(d.data_ptr(), d.stride(0), d.stride(1), nchan, npol, ndim, nbin, r, ncu)["kernel"] == family
    want = _reference(family, x, r2, _reference(family, x, r1, np.zeros_like(got), ncu), ncu)
    assert np.array_equal(got, want)
    # every planned sample reached the profile (float64: the hits above were counted for all of them)
    _check_f64(got, x, runs_of_plan(full, i0), np.zeros_like(got), 1)


# fused folds (dspsr_amd_filterbank_perform_fold) use up their plan in fold_build_part_plan (fold.hip, fold_is_fused() 1
# and 2) and fold_build_segment_plan (fold_is_fused() 3): (C, M, nfilt, nbin, samples per bin, fused_fold, mode)
@pytest.mark.parametrize("C,M,nfilt,nbin,spb,force,mode", [
    (64, 128, (9, 10), 100, 12.345, True, 1),
    (4, 16384, (301, 212), 64, 700.3, False, 3),
])
def test_fused_fold_then_a_plan_without_set_nbin(oracle, gpu, C, M, nfilt, nbin, spb, force, mode):
    """a fused fold, then a plan that continues the phase without set_nbin and starts in the bin the last plan ended in, then a
    second fused fold: the same hits and the same profile, bit for bit, as with set_nbin in front of the second plan (the
    documented order), and every counted sample folded"""
    dspsr_amd, ctx, ncu = gpu
    o = oracle
    N, nkeep = C * M, M - sum(nfilt)
    step, ovl = 2 * (N - sum(nfilt) * C), 2 * sum(nfilt) * C
    npart = 5
    ndat = npart * nkeep
    rng = np.random.default_rng(41)
    kernel = np.exp(1j * rng.uniform(-np.pi, np.pi, N)).astype(np.complex64)
    eng = dspsr_amd.FilterbankEngine(ctx).setup(C, M, nfilt[0], nfilt[1], 1, 2, True, kernel, max_parts=2,
                                                fused_fold=dspsr_amd.FUSED_ALWAYS if force else dspsr_amd.FUSED_AUTO)
    assert eng.fold_is_fused() == mode
    pps, phi1 = 1.0 / (spb * nbin), 0.37
    phi2 = _recur_phi(phi1, pps, ndat)
    p1, p2 = o.fold_binplan(phi1, pps, nbin, ndat), o.fold_binplan(phi2, pps, nbin, ndat)
    assert p1[-1] == p2[0]                                       # the second plan starts inside the last run of the first
    raws = [torch.from_numpy(np.clip(np.rint(rng.standard_normal(2 * (npart * step + ovl)) * 24.0), -128, 127).astype(np.int8)).cuda()
            for _ in range(2)]                                   # 8-bit real samples of two polarisations
    cont, doc = dspsr_amd.FoldEngine(ctx), dspsr_amd.FoldEngine(ctx)
    hits = [np.zeros(nbin, np.uint32), np.zeros(nbin, np.uint32)]
    for k, f in enumerate((cont, doc)):
        f.set_shape(C, 1, 4, nbin)
        f.set_nbin(nbin)
        f.set_ndat(ndat, 0)
        f.set_bins(phi1, pps, ndat, 0, hits[k])
        eng.perform_fold(f, npart, dspsr_amd.COHERENCE, raw=raws[0], scale=float(o.S8))
        if f is doc:
            f.set_nbin(nbin)
        f.set_ndat(ndat, 0)
        f.set_bins(phi2, pps, ndat, 0, hits[k])
        eng.perform_fold(f, npart, dspsr_amd.COHERENCE, raw=raws[1], scale=float(o.S8))
    a, b = cont.synch(), doc.synch()
    want_hits = (np.bincount(p1, minlength=nbin) + np.bincount(p2, minlength=nbin)).astype(np.uint32)
    assert np.array_equal(hits[0], want_hits) and np.array_equal(hits[1], want_hits)
    assert cont.get_ndat_folded() == 2 * ndat
    assert np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(a, b)
    eng.close()
    cont.close()
    doc.close()


# ---- 10. one engine's two plan slots refilled by different consumers with different buffer layouts ---------------------------------
def _slot_growth(steps):
    """slot_reserve restated for a sequence of plans (consumer, slot, words, intervals, aux words): the words are sized exactly,
    intervals as _slot_cap, aux words n + n / 4 + 1024.  Returns (step, buffer pair, consumer that sized it before) for every
    step that regrows a pair (None: the pair was never sized)."""
    cap, events = {}, []
    for k, (who, slot, words, niv, naux) in enumerate(steps, 1):
        for pair, need, alloc in (("words", words, words), ("iv", niv, _slot_cap(niv)), ("aux", naux, naux + naux // 4 + 1024)):
            have, by = cap.get((slot, pair), (0, None))
            if need > have:
                events.append((k, pair, by))
                cap[(slot, pair)] = (alloc, who)
    return events


@pytest.mark.parametrize("C,M,nfilt,nbin,spb,force,mode", [
    (64, 128, (9, 10), 100, 12.345, True, 1),
    (4, 16384, (301, 212), 64, 700.3, False, 3),
])
def test_slots_shared_by_every_plan_consumer(oracle, gpu, C, M, nfilt, nbin, spb, force, mode):
    """six plans back to back on ONE engine bound to a caller's buffer, nothing in between waits for the device: a stand-alone
    dense fold (slot 0), a fused perform_fold (slot 1: the part plan of fold_is_fused() 1, the segment plan of 3), a chunked fold
    of short runs (slot 0), a second fused perform_fold (slot 1), fold_many with a second engine (slot 0: this engine's dense
    table over the group's grid; the other engine walks), a LONG fold (slot 1).  From the run counts: the chunked fold regrows
    the intervals the dense fold sized, fold_many regrows the table (aux) the dense fold sized, the LONG fold regrows the
    intervals the fused plan sized -- while it finds the part plan's words (fold_is_fused() 1) larger than its own.  (The words
    of a stand-alone plan are nbin + 1 in every consumer: only the part plan sizes them otherwise, and in this order of steps it
    meets a slot no one sized.)
    The reference is the same six steps, each on a FRESH engine -- both slots never used, every buffer sized for this plan alone --
    bound to a second buffer: the same sums in the same order, so the two buffers hold the same bits."""
    import fused_fold_cases as fc
    dspsr_amd, ctx, ncu = gpu
    o = oracle
    N, nkeep = C * M, M - sum(nfilt)
    step, ovl = 2 * (N - sum(nfilt) * C), 2 * sum(nfilt) * C
    npart = 5
    ndat_f = npart * nkeep
    rng = np.random.default_rng(43)
    kernel = np.exp(1j * rng.uniform(-np.pi, np.pi, N)).astype(np.complex64)
    fb = dspsr_amd.FilterbankEngine(ctx).setup(C, M, nfilt[0], nfilt[1], 1, 2, True, kernel, max_parts=2,
                                               fused_fold=dspsr_amd.FUSED_ALWAYS if force else dspsr_amd.FUSED_AUTO)
    assert fb.fold_is_fused() == mode
    raws = [torch.from_numpy(np.clip(np.rint(rng.standard_normal(2 * (npart * step + ovl)) * 24.0), -128, 127).astype(np.int8)).cuda()
            for _ in range(2)]
    ndat = 80000
    gen = torch.Generator(device="cuda")
    gen.manual_seed(44)
    rows = torch.rand((C, 1, ndat * 4), dtype=torch.float32, device="cuda", generator=gen) + 0.5
    nbin2 = 64                                                   # the second engine of fold_many
    i0 = 4
    #        kind     nbin   phi   samples per bin       samples
    plans = [("fold", nbin, 0.52, 40.3, 20000),                  # 1. dense: a period above FOLD_CHUNK samples, runs under 64
             ("fused", nbin, 0.37, spb, ndat_f),                 # 2.
             ("fold", nbin, 0.70, 3.0, 20000),                   # 3. chunked: short runs, more intervals than step 1
             ("fused", nbin, 0.61, spb, ndat_f),                 # 4.
             ("many", nbin, 0.33, 40.3, ndat - 10),              # 5. dense over a longer grid: a larger table than step 1
             ("fold", nbin, 0.45, 70.3, 20000)]                  # 6. LONG
    many2 = (nbin2, 0.21, 5.0, ndat - 10)                        #    ... with a walk plan of the second engine
    per_sample = [o.fold_binplan(phi, 1.0 / (s * nb), nb, n) for _k, nb, phi, s, n in plans]
    runs = [runs_of_plan(p, 0 if k[0] == "fused" else i0) for k, p in zip(plans, per_sample)]
    plan2 = o.fold_binplan(many2[1], 1.0 / (many2[2] * nbin2), nbin2, many2[3])
    disp = [fold_dispatch(rows.data_ptr(), rows.stride(0), rows.stride(1), C, 1, 4, nbin, r, ncu)["kernel"] for r in runs]
    assert [disp[0], disp[2], disp[4], disp[5]] == ["dense", "chunked", "dense", "long"]
    assert fold_dispatch(rows.data_ptr(), rows.stride(0), rows.stride(1), C, 1, 4, nbin2, runs_of_plan(plan2, i0), ncu)["kernel"] == "chunked"
    assert plan_span(runs[4]) == plan_span(runs_of_plan(plan2, i0))          # the group's chunk grid is this engine's own

    def ntab(r):
        first, last = plan_span(r)
        return -(-(last - first) // FOLD_CHUNK) * nbin
    if mode == 1:
        def fused_need(r):
            pp = fc.part_plan(r, nkeep, npart, nbin)
            return ("part", ((npart + 4) & ~3) + 4 * sum(len(p) for p in pp), sum(len(iv) for p in pp for _b, iv in p), 0)
    else:
        def fused_need(r):
            assert int(r[:, 2].max()) >= 64 and (r[1:-1, 2] >= 32).all()     # the segment plan qualifies
            return ("segment", nbin + 1, len(r), len(r) + 1 + (ndat_f >> 10) + 1)
    needs = [("fold", 0, nbin + 1, len(runs[0]), ntab(runs[0])), fused_need(runs[1])[:1] + (1,) + fused_need(runs[1])[1:],
             ("fold", 0, nbin + 1, len(runs[2]), 0), fused_need(runs[3])[:1] + (1,) + fused_need(runs[3])[1:],
             ("fold_many", 0, nbin + 1, len(runs[4]), ntab(runs[4])), ("fold", 1, nbin + 1, len(runs[5]), 0)]
    grew = _slot_growth(needs)
    assert {(3, "iv", "fold"), (5, "aux", "fold"), (6, "iv", needs[1][0])} <= set(grew), grew
    assert (mode == 1) == (needs[1][2] > nbin + 1)               # the LONG fold meets the part plan's larger words

    def run(bufs, fresh):
        """the six steps into bufs = (bound buffer, second engine's buffer); fresh: a new engine for every step"""
        hits, engines = [], []

        def engine(buf, nb):
            e = dspsr_amd.FoldEngine(ctx)
            e.bind_profile(buf, C, 1, 4, nb)
            engines.append(e)
            return e
        eng = None
        for (kind, nb, phi, s, n), r in zip(plans, runs):
            if fresh or eng is None:
                eng = engine(bufs[0], nbin)
            start = 0 if kind == "fused" else i0
            h = np.zeros(nb, np.uint32)
            eng.set_nbin(nb)
            eng.set_ndat(n, start)
            assert eng.set_bins(phi, 1.0 / (s * nb), n, start, h) == n
            hits.append(h)
            if kind == "fused":
                fb.perform_fold(eng, npart, dspsr_amd.COHERENCE, raw=raws[len(hits) // 2 - 1], scale=float(o.S8))
            elif kind == "many":
                other = engine(bufs[1], nbin2)
                h2 = np.zeros(nbin2, np.uint32)
                other.set_nbin(nbin2)
                other.set_ndat(many2[3], i0)
                other.set_bins(many2[1], 1.0 / (many2[2] * nbin2), many2[3], i0, h2)
                hits.append(h2)
                assert dspsr_amd.FoldEngine.fold_many([eng, other], rows) == 2
            else:
                eng.fold(rows)
        torch.cuda.synchronize()
        for e in engines:
            e.close()
        return hits

    span = nbin * 4 + 4                                          # (padded rows, float4 aligned: the fused kernels take them)
    bufs = [(torch.zeros((C, span), dtype=torch.float32, device="cuda"), torch.zeros((C, nbin2 * 4), dtype=torch.float32, device="cuda"))
            for _ in range(2)]
    torch.cuda.synchronize()                                     # inputs and the zeroed profiles are in place
    hits = run(bufs[0], False)
    hits_ref = run(bufs[1], True)
    want_hits = [np.bincount(p, minlength=nb).astype(np.uint32) for (_k, nb, *_), p in zip(plans, per_sample)]
    want_hits.insert(5, np.bincount(plan2, minlength=nbin2).astype(np.uint32))
    for k, w in enumerate(want_hits):
        assert np.array_equal(hits[k], w) and np.array_equal(hits_ref[k], w), k
    for got, ref in zip(bufs[0], bufs[1]):
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        assert np.isfinite(got).all() and np.abs(got).max() > 0
        assert np.array_equal(got, ref)
    assert (bufs[0][0].cpu().numpy()[:, nbin * 4:] == 0).all()   # the padding of the bound rows is never written
    fb.close()
