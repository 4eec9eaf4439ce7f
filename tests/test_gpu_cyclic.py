"""Cyclic-spectrum folding on the device (csrc/cyclic_fold.hip) against the CPU restatement (tests/cyclic_reference.py):
exact data bit for bit, noise data within twice the error of the reference's own float32 association, determinism."""
import numpy as np
import pytest

import cyclic_cases as cc
import cyclic_reference as cr
import dspsr_amd
from device_buffers import SENTINEL, OutputLayout, sentinel_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _place(rows, offset, row_pad):
    """complex rows [nchan][npol][ndat] as float rows inside a buffer of SENTINEL: `offset` floats (even: 8-byte rows) past a
    256-byte boundary, rows `row_pad` floats apart.  Returns (buffer as int32, snapshot of its bits, float32 view)."""
    import torch
    nchan, npol, ndat = rows.shape
    flat = np.ascontiguousarray(np.stack([rows.real, rows.imag], axis=-1).astype(np.float32)).reshape(nchan, npol, 2 * ndat)
    buf, view = sentinel_rows(OutputLayout(nchan, npol, 2 * ndat, offset=offset, row_pad=row_pad))
    view.copy_(torch.from_numpy(flat))
    return buf, buf.clone(), view


def _lags(eng):
    a = eng.synch_lags()
    return a[..., 0] + 1j * a[..., 1]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("index", range(len(cr.EXACT_CASES)), ids=[c["name"] for c in cr.EXACT_CASES])
def test_exact_rows_bit_for_bit(ctx, index):
    case = cr.EXACT_CASES[index]
    cr.check_exact(case)
    eng = dspsr_amd.CyclicFoldEngine(ctx)
    eng.set_shape(case["nchan"], case["npol_in"], case["npol_out"], case["nlag"], 1, case["nbin"])
    for k, ((ndat, start, phi, pps, zero), (rows, rhits, ref)) in enumerate(zip(case["calls"], cr.exact_reference(index))):
        buf, before, view = _place(rows, offset=2 * (k + 1) + 2 * index, row_pad=2 * (3 + k))
        if zero:
            eng.zero()
        hits = np.zeros(case["nbin"], np.uint32)
        eng.set_ndat(ndat, start)
        if k % 2:                                           # the per-sample form of the plan, as Fold::fold drives it
            phase, dn = float(phi), float(case["nbin"])
            for i in range(ndat):
                phase -= np.floor(phase)
                eng.set_bin(start + i, phase * dn, pps * dn)
                hits[int(phase * dn)] += 1
                phase += pps
        else:
            assert eng.set_bins(phi, pps, ndat, start, hits) == ndat
        eng.fold(view)
        got = _lags(eng)
        assert np.array_equal(hits, rhits), "hits of call %d" % k
        assert _same_bits(got.astype(np.complex64), ref), "call %d: %d of %d lag values differ, first at %s" % (
            k, (got != ref).sum(), ref.size, np.argwhere(got != ref)[:1])
        assert bool((buf == before).all()), "call %d wrote into the input buffer" % k
        assert int((buf == SENTINEL).sum()) > 0
    eng.close()


def test_refusals_before_a_launch(ctx):
    import torch
    eng = dspsr_amd.CyclicFoldEngine(ctx)
    for bad in [(1, 1, 2, 33, 1, 8), (1, 2, 3, 33, 1, 8), (1, 2, 2, 1, 1, 8), (1, 2, 2, 33, 0, 8), (1, 2, 2, 33, 3, 8),
                (1, 2, 2, 70000, 1, 2), (1, 3, 1, 33, 1, 8)]:
        with pytest.raises(dspsr_amd.DspsrAmdError):
            eng.set_shape(*bad)
    eng.set_shape(2, 2, 2, 33, 1, 8)
    eng.set_ndat(100, 0)
    eng.set_bins(0.0, 0.01, 100, 0)
    x = torch.zeros((2, 2, 203), dtype=torch.float32, device="cuda")
    with pytest.raises(dspsr_amd.DspsrAmdError):
        eng.fold(x[:, :, 1:201])                            # rows on a 4-byte boundary
    y = torch.zeros((2, 2, 100), dtype=torch.float32, device="cuda")
    with pytest.raises(dspsr_amd.DspsrAmdError):
        eng.fold(y.as_strided((2, 2, 200), (100, 50, 1)))   # strides shorter than the row
    assert not eng.synch_lags().any()
    eng.close()


# ---- noise ---------------------------------------------------------------------------------------------------------------------
NOISE = [dict(npol_in=2, npol_out=4, nlag=129, nbin=32, nchan=2, ndat=2500, pps=1.0 / 32 / 11.3),
         dict(npol_in=2, npol_out=1, nlag=33, nbin=8, nchan=2, ndat=3000, pps=1.0 / 8 / 300.0),
         dict(npol_in=1, npol_out=1, nlag=513, nbin=64, nchan=1, ndat=2200, pps=1.0 / 64 / 2.5)]


@pytest.mark.parametrize("c", NOISE, ids=["nlag%d-npol%d" % (c["nlag"], c["npol_out"]) for c in NOISE])
def test_noise_rows_within_twice_the_reference_association(ctx, c):
    """Gaussian rows at the scale the filterbank emits for 8-bit input (rms about 30 per component after an unnormalised
    transform pair).  e(X) = max |X - R64| / max |R64| per (chan, pol) lag function; the yardstick is the error of the float32
    strict-time-order sums.  Twice that for the re-association and the fused multiply-adds, with a floor of 4 * 2^-24."""
    rows = cr.noise_rows(5 + c["nlag"], c["nchan"], c["npol_in"], c["ndat"], 30.0)
    p0, p1, _ = cr.plans(0.37, c["pps"], c["nbin"], c["ndat"])
    r64 = cr.fold(rows, p0, p1, c["nlag"], c["npol_out"], c["nbin"])
    f32 = cr.fold(rows, p0, p1, c["nlag"], c["npol_out"], c["nbin"], dtype=np.float32)
    eng = dspsr_amd.CyclicFoldEngine(ctx)
    eng.set_shape(c["nchan"], c["npol_in"], c["npol_out"], c["nlag"], 1, c["nbin"])
    eng.set_ndat(c["ndat"], 0)
    eng.set_bins(0.37, c["pps"], c["ndat"], 0)
    _, _, view = _place(rows, offset=6, row_pad=10)
    eng.fold(view)
    got = _lags(eng)
    e_gpu, e_f32 = cr.lag_error(got, r64), cr.lag_error(f32, r64)
    bound = np.maximum(2 * e_f32, 4 * 2.0 ** -24)
    print("e(GPU) max %.3g, e(F32 strict order) max %.3g" % (e_gpu.max(), e_f32.max()))
    assert (e_gpu <= bound).all(), "e(GPU) = %s\ne(F32 strict order) = %s" % (e_gpu, e_f32)
    # the same call again on this engine after zero: identical bits
    eng.zero()
    eng.set_ndat(c["ndat"], 0)
    eng.set_bins(0.37, c["pps"], c["ndat"], 0)
    eng.fold(view)
    assert _same_bits(eng.synch_lags(), np.stack([got.real, got.imag], axis=-1).astype(np.float32))
    eng.close()


def test_same_pieces_same_bits_whatever_comes_between(ctx):
    """two engines fold the same two pieces; one of them reads its lag data between the calls (an extra combine of the partial
    arrays): the same bits"""
    c = NOISE[0]
    rows = cr.noise_rows(77, c["nchan"], c["npol_in"], 2 * c["ndat"], 30.0)
    _, _, view = _place(rows, offset=2, row_pad=4)
    res = []
    for variant in range(2):
        eng = dspsr_amd.CyclicFoldEngine(ctx)
        eng.set_shape(c["nchan"], c["npol_in"], c["npol_out"], c["nlag"], 1, c["nbin"])
        for piece in range(2):
            start = piece * c["ndat"]
            eng.set_ndat(c["ndat"], start)
            eng.set_bins(0.1 + 0.2 * piece, c["pps"], c["ndat"], start)
            eng.fold(view)
            if variant:
                eng.synch_lags()
        res.append(eng.synch_lags())
        eng.close()
    assert _same_bits(res[0], res[1])


def test_a_new_shape_of_the_same_size_starts_from_zero(ctx):
    rows = cr.exact_rows(9, 2, 2, 300)
    _, _, view = _place(rows, offset=4, row_pad=2)
    eng = dspsr_amd.CyclicFoldEngine(ctx)
    eng.set_shape(2, 2, 2, 33, 1, 4)
    eng.set_ndat(300, 0)
    eng.set_bins(0.2, 0.01, 300, 0)
    eng.fold(view)
    assert eng.synch_lags().any()
    eng.set_shape(2, 2, 2, 33, 1, 4)                        # the same shape again keeps the sums
    assert eng.synch_lags().any()
    eng.set_shape(4, 2, 2, 33, 1, 2)                        # nbin and nchan exchanged: the same size, another meaning
    assert not eng.synch_lags().any()
    eng.close()


# ---- where a segment walks several tiles (tests/cyclic_cases.py; tests/test_cyclic_cases_host.py proves what each case reaches) ----
def _first_difference(case, ndat, got, ref):
    """the first wrong lag value as the kernel sees it: owner lane and the steps of u it covers"""
    bad = np.argwhere(got != ref)
    b, q, chan, ilag = (int(v) for v in bad[0])
    p = cc.partition(case["nchan"], case["npol_out"], case["nlag"], case["nbin"], ndat)
    return "%d of %d lag values differ, first at bin %d pol %d chan %d lag %d (parity %d, workgroup x %d; %d tiles, %d per segment, %d " \
           "parts): got %s, reference %s" % (len(bad), ref.size, b, q, chan, ilag, ilag % 2, ilag // (2 * cc.CY_HL), p.ntile, p.tps,
                                             p.nparts, got[b, q, chan, ilag], ref[b, q, chan, ilag])


@pytest.mark.parametrize("name", cc.NAMES)
def test_table_rows_bit_for_bit(ctx, name):
    case, index = cc.by_name(name), cc.NAMES.index(name)
    cr.check_exact(case)
    nbin = case["nbin"]
    eng = dspsr_amd.CyclicFoldEngine(ctx)
    eng.set_shape(case["nchan"], case["npol_in"], case["npol_out"], case["nlag"], 1, nbin)
    for k, ((ndat, start, phi, pps, zero), (rhits, ref)) in enumerate(zip(case["calls"], cc.reference(name))):
        buf, before, view = _place(cc.case_rows(name, k), offset=2 * (k + 1) + 2 * index, row_pad=2 * (3 + k))
        if zero:
            eng.zero()
        hits = np.zeros(nbin, np.uint32)
        eng.set_ndat(ndat, start)
        if case["placed"][k] is not None:                   # both plans given sample by sample: plan1 = (ibin + k) % nbin
            p0, p1 = case["placed"][k]
            for i in range(ndat):
                eng.set_bin(start + i, float(p0[i]), 2.0 * float((p1[i] - p0[i]) % nbin))
                hits[p0[i]] += 1
        elif k % 2:                                         # the per-sample form of the plan, as Fold::fold drives it
            phase, dn = float(phi), float(nbin)
            for i in range(ndat):
                phase -= np.floor(phase)
                eng.set_bin(start + i, phase * dn, pps * dn)
                hits[int(phase * dn)] += 1
                phase += pps
        else:
            assert eng.set_bins(phi, pps, ndat, start, hits) == ndat
        eng.fold(view)
        got = _lags(eng).astype(np.complex64)
        assert np.array_equal(hits, rhits), "hits of call %d" % k
        assert _same_bits(got, ref), "call %d: %s" % (k, _first_difference(case, ndat, got, ref))
        assert bool((buf == before).all()), "call %d wrote into the input buffer" % k
        assert int((buf == SENTINEL).sum()) > 0
        del buf, before, view
    eng.close()


def test_a_new_shape_refuses_the_plan_of_the_old_one(ctx):
    """set_shape(nbin 64), set_ndat, set_bins, set_shape(nbin 8), fold: the plan holds bins up to 63 and belongs to the old
    shape.  The fold is refused before anything is launched; set_ndat makes the engine usable again."""
    ndat, pps = 700, 1.0 / 3.0
    rows = cr.exact_rows(21, 2, 2, ndat)
    _, _, view = _place(rows, offset=4, row_pad=2)
    eng = dspsr_amd.CyclicFoldEngine(ctx)
    eng.set_shape(2, 2, 2, 33, 1, 64)
    eng.set_ndat(ndat, 0)
    eng.set_bins(0.2, pps / 64, ndat, 0)
    assert cr.plans(0.2, pps / 64, 64, ndat)[0].max() == 63
    eng.set_shape(2, 2, 2, 33, 1, 8)
    with pytest.raises(dspsr_amd.DspsrAmdError, match=r"\(-4\).*set_ndat"):        # DSPSR_AMD_ESTATE
        eng.fold(view)
    assert not eng.synch_lags().any()
    with pytest.raises(dspsr_amd.DspsrAmdError):                                    # no block: no sample to plan either
        eng.set_bins(0.2, pps / 8, ndat, 0)
    with pytest.raises(dspsr_amd.DspsrAmdError):
        eng.set_bin(0, 0.0, 0.0)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="set_ndat"):
        eng.fold(view)
    assert not eng.synch_lags().any()
    p0, p1, rhits = cr.plans(0.2, pps / 8, 8, ndat)
    ref = cr.fold(rows, p0, p1, 33, 2, 8, dtype=np.float32)
    hits = np.zeros(8, np.uint32)
    eng.set_ndat(ndat, 0)
    eng.set_bins(0.2, pps / 8, ndat, 0, hits)
    eng.fold(view)
    assert np.array_equal(hits, rhits) and _same_bits(_lags(eng).astype(np.complex64), ref)
    eng.set_shape(2, 2, 2, 33, 1, 8)                        # the same shape again keeps the plan, as it keeps the sums
    eng.fold(view)
    assert _same_bits(_lags(eng).astype(np.complex64), cr.fold(rows, p0, p1, 33, 2, 8, ref, np.float32))
    eng.close()


MANY_TILES = dict(npol_in=2, npol_out=4, nlag=129, nbin=64, nchan=64, ndat=6000, pps=1.0 / 64 / 11.3)


def test_noise_rows_with_several_tiles_per_segment(ctx):
    """the rule of test_noise_rows_within_twice_the_reference_association, unchanged, where 8 parts walk 12 tiles in pairs: a
    run's float32 sum is then cut at the segment's ends only, and the combine adds six partial sums that all count"""
    c = MANY_TILES
    assert cc.partition(c["nchan"], c["npol_out"], c["nlag"], c["nbin"], c["ndat"]) == (8, 12, 8, 2, 2)
    test_noise_rows_within_twice_the_reference_association(ctx, c)


def test_same_pieces_same_bits_with_several_partial_sums(ctx):
    """test_same_pieces_same_bits_whatever_comes_between at the shape of "multi-tile": four parts of 3, 3, 3 and 1 tiles, runs of
    1300 samples -- a bin's sum is in several partial arrays, and the extra combine between the pieces must not change what the
    second piece adds to"""
    c = cc.by_name("multi-tile")
    ndat, pps = 4700, c["calls"][1][3]
    assert cc.partition(c["nchan"], c["npol_out"], c["nlag"], c["nbin"], ndat) == (4, 10, 4, 3, 0)
    rows = cr.noise_rows(78, c["nchan"], c["npol_in"], 2 * ndat, 30.0)
    _, _, view = _place(rows, offset=2, row_pad=4)
    res = []
    for variant in range(2):
        eng = dspsr_amd.CyclicFoldEngine(ctx)
        eng.set_shape(c["nchan"], c["npol_in"], c["npol_out"], c["nlag"], 1, c["nbin"])
        for piece in range(2):
            start = piece * ndat
            eng.set_ndat(ndat, start)
            eng.set_bins(0.1 + 0.2 * piece, pps, ndat, start)
            eng.fold(view)
            if variant:
                eng.synch_lags()
        res.append(eng.synch_lags())
        eng.close()
    assert res[0].any() and _same_bits(res[0], res[1])


def test_one_lag_more_than_the_largest_is_refused(ctx):
    """the case "max-nlag" shows CY_MAX_NLAG lags accepted and right; one more is refused, and the engine stays usable"""
    eng = dspsr_amd.CyclicFoldEngine(ctx)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="nlag=%d" % (cc.CY_MAX_NLAG + 1)):
        eng.set_shape(1, 1, 1, cc.CY_MAX_NLAG + 1, 1, 8)
    with pytest.raises(dspsr_amd.DspsrAmdError, match="nchan=%d" % (cc.MAX_NCHAN + 1)):
        eng.set_shape(cc.MAX_NCHAN + 1, 1, 1, 2, 1, 2)
    eng.set_shape(1, 1, 1, cc.CY_MAX_NLAG, 1, 8)
    assert eng.synch_lags().shape == (8, 1, 1, cc.CY_MAX_NLAG, 2) and not eng.synch_lags().any()
    eng.close()
