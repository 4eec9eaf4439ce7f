"""Search mode with the four Coherence products (digifits -p 4, digifil -d 4) inside the inverse pass:
dspsr_amd_filterbank_perform_search(DSPSR_AMD_COHERENCE) against the route it replaces -- perform_detect(COHERENCE, ndim 1) of the SAME
object on the SAME raw blocks, then TScrunch (the oracle's sequential float32 loop, which k_tscrunch_fpt equals bit for bit) -- bit for
bit, as a stream over several calls, on every case of tests/coherence_search_cases.py (what each is there for:
tests/test_coherence_search_cases_host.py).  Then against the oracle's own arithmetic, its repeatability, its refusals and the two
drivers that use it behind `fuse_coherence`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coherence_search_cases as cc                                                  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dspsr_amd
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    yield dspsr_amd, ctx
    ctx.close()


@pytest.fixture(scope="module")
def oracle():
    import oracle.dspsr_oracle as o
    return o


def _engine(dspsr_amd, ctx, case):
    if case.real:
        fb = dspsr_amd.FilterbankEngine(ctx).setup(case.C, case.M, case.nfilt[0], case.nfilt[1], 1, 2, True, cc.kernel_of(case),
                                                   max_parts=case.maxp, split_in_inverse=case.split_in_inverse)
    else:                                                  # test_gpu_search._fb_case(nchan, freq_res, dm, False, max_parts)
        r = dspsr_amd.Dedispersion(1382.0, -50.0, case.dm, input_nchan=1, ndim=2)
        r.set_frequency_resolution(case.M)
        r.match(case.C)
        # (a complex 8-bit block of this size takes the two-pass path when left to itself: case j switches it off, force_four_pass = 2)
        fb = dspsr_amd.FilterbankEngine(ctx).setup(case.C, r.ndat, r.impulse_pos, r.impulse_neg, 1, 2, False, r.kernel, max_parts=case.maxp,
                                                   force_four_pass=2 if case.npass == 3 else 0)
    assert fb.nkeep == case.nkeep and fb.npass(True) == case.npass
    return fb


def _blocks(case, fb, seed):
    """the raw 8-bit block of every call of the case, on the device"""
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(cc.raw_block(rng, npart * fb.nsamp_step + fb.nsamp_overlap, case.real)).cuda() for npart in case.parts]


def _search(dspsr_amd, fb, case, sf, blocks):
    """perform_search(COHERENCE) over the calls, fresh carry: (rows [C][4][N] on the host, carry_count).  Every call writes into a
    buffer one sample longer than its nout, pre-filled with a sentinel that must survive."""
    carry = torch.zeros((case.C, 4), dtype=torch.float32, device="cuda")
    cnt, got = 0, []
    for npart, raw in zip(case.parts, blocks):
        want_nout = (cnt + npart * case.nkeep) // sf
        out = torch.full((case.C, 4, want_nout + 1), SENTINEL, dtype=torch.float32, device="cuda")
        nout, cnt = fb.perform_search(out, carry, cnt, npart, sf, dspsr_amd.COHERENCE, raw=raw, layout=dspsr_amd.RAW_GENERIC, scale=cc.SCALE)
        o = out.cpu().numpy()
        assert nout == want_nout
        assert np.all(o[:, :, nout] == SENTINEL), "a sample behind the nout complete ones was written"
        got.append(o[:, :, :nout])
    return np.concatenate(got, axis=2), cnt


def _detected(dspsr_amd, fb, case, blocks):
    """perform_detect(COHERENCE, ndim 1) of the same object on the same blocks, concatenated: [C][4][total]"""
    dets = []
    for npart, raw in zip(case.parts, blocks):
        det = torch.zeros((case.C, 4, npart * case.nkeep), dtype=torch.float32, device="cuda")
        fb.perform_detect(det, npart, dspsr_amd.COHERENCE, 1, raw=raw, layout=dspsr_amd.RAW_GENERIC, scale=cc.SCALE)
        dets.append(det.cpu().numpy())
    return np.concatenate(dets, axis=2)


RUNS = [(c, k) for c in cc.CASES for k in range(len(c.sfs))]


@pytest.mark.parametrize("case,k", RUNS, ids=["%s-t%d" % (c.name, c.sfs[k]) for c, k in RUNS])
def test_coherence_search_equals_detection_and_tscrunch_bit_for_bit(oracle, gpu, case, k):
    dspsr_amd, ctx = gpu
    sf = case.sfs[k]
    fb = _engine(dspsr_amd, ctx, case)
    try:
        assert fb.search_fuses(dspsr_amd.COHERENCE, sf) == cc.fits(case.C, case.M, case.nkeep, sf) == case.fused[k]
        if case.name == "i":
            assert not fb.search_fuses(dspsr_amd.COHERENCE, 16) and fb.search_fuses(dspsr_amd.PPQQ, 16)
        if case.name == "l":
            assert not fb.presplit()
        assert not fb.search_fuses(dspsr_amd.STOKES, sf) and not fb.search_fuses(17, sf) and not fb.search_fuses(dspsr_amd.COHERENCE, 0)
        blocks = _blocks(case, fb, 7000 + 13 * ord(case.name) + sf)
        got, cnt = _search(dspsr_amd, fb, case, sf, blocks)
        det = _detected(dspsr_amd, fb, case, blocks)
    finally:
        fb.close()
    want = oracle.tscrunch_fpt(det, sf)
    assert cnt == det.shape[2] % sf
    assert got.shape == want.shape and want.shape[2] > 0
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%d of %d samples differ, first (chan, row, out) %s" % (len(bad), got.size, bad[:4].tolist())


def test_presplit_is_the_form_of_the_real_cases(gpu):
    """the real cases run the pre-split instantiations (k_inv_chan<., 22, .>) where the object takes the pre-split spectrum; case l, the
    same kind of geometry with split_in_inverse, the others (<., 18, .>)"""
    dspsr_amd, ctx = gpu
    l = cc.BY_NAME["l"]
    fb = dspsr_amd.FilterbankEngine(ctx).setup(l.C, l.M, l.nfilt[0], l.nfilt[1], 1, 2, True, cc.kernel_of(l), max_parts=l.maxp)
    try:
        assert fb.presplit() and fb.search_fuses(dspsr_amd.COHERENCE, l.sfs[0])
    finally:
        fb.close()
    taken = []
    for name in "aefgh":
        fb = _engine(dspsr_amd, ctx, cc.BY_NAME[name])
        taken.append(fb.presplit())
        fb.close()
    assert any(taken)


@pytest.mark.parametrize("name", ["a", "e", "j"])
def test_coherence_search_against_the_oracles_products(oracle, gpu, name):
    """the same call against cross_detect's products formed by the oracle from the object's complex output and scrunched by the
    oracle: within rtol 3e-7, atol 3e-7 * sf * max|detected| -- the tolerance test_gpu_parity holds perform_detect to (rtol 3e-7,
    atol 3e-7 * max|want|: a product is two multiplies and an add of float32, contracted on the device), times the sf terms of a
    sum that both sides add in the same order."""
    dspsr_amd, ctx = gpu
    case = cc.BY_NAME[name]
    sf = case.sfs[0]
    fb = _engine(dspsr_amd, ctx, case)
    try:
        blocks = _blocks(case, fb, 9100 + ord(name))
        got, _ = _search(dspsr_amd, fb, case, sf, blocks)
        cplx = []
        for npart, raw in zip(case.parts, blocks):
            c = torch.zeros((case.C, 2, 2 * npart * case.nkeep), dtype=torch.float32, device="cuda")
            fb.perform_raw(raw, dspsr_amd.RAW_GENERIC, cc.SCALE, c, npart)
            cplx.append(c.cpu().numpy().view(np.complex64))
    finally:
        fb.close()
    det = oracle.detect_layout(oracle.detect_products(np.concatenate(cplx, axis=2), "Coherence"), 1)
    want = oracle.tscrunch_fpt(det, sf)
    assert got.shape == want.shape and want.shape[2] > 0
    atol = 3e-7 * sf * float(np.abs(det).max())
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) - 3e-7 * np.abs(want.astype(np.float64))
    print("case %s: max |got - want| = %.3g, atol = %.3g" % (name, float(np.abs(got - want).max()), atol))
    assert err.max() <= atol, (float(err.max()), atol)


def test_coherence_search_is_repeatable(gpu):
    """no atomics: two runs of case a on fresh carries give the same bytes"""
    dspsr_amd, ctx = gpu
    case = cc.BY_NAME["a"]
    fb = _engine(dspsr_amd, ctx, case)
    try:
        blocks = _blocks(case, fb, 4242)
        first, c1 = _search(dspsr_amd, fb, case, case.sfs[0], blocks)
        second, c2 = _search(dspsr_amd, fb, case, case.sfs[0], blocks)
    finally:
        fb.close()
    assert c1 == c2 and first.tobytes() == second.tobytes()


def _call(dspsr_amd, fb, raw, state, sf, out, cs, ps, carry, cnt, npart):
    """the C entry point itself: (return code, message, carry_count after, nout after); nout starts from a mark"""
    lib = dspsr_amd.lib
    count, nout = C.c_uint32(cnt), C.c_uint64(0xABCDEF)
    rc = lib.dspsr_amd_filterbank_perform_search(fb.handle, None, 0, 0, 0, raw.data_ptr(), dspsr_amd.RAW_GENERIC, cc.SCALE, state, sf,
                                                 out.data_ptr(), cs, ps, carry.data_ptr(), C.byref(count), npart, C.byref(nout))
    return rc, lib.dspsr_amd_last_error(fb.ctx.handle).decode(), count.value, nout.value


def test_coherence_search_refusals(gpu):
    """each by name, with nothing launched -- output and carry keep their fill -- and *carry_count and *nout as they were"""
    dspsr_amd, ctx = gpu
    case = cc.BY_NAME["a"]
    sf, npart = case.sfs[0], 3
    nout = npart * case.nkeep // sf
    out = torch.full((case.C, 4, nout + 1), SENTINEL, dtype=torch.float32, device="cuda")
    carry = torch.full((case.C, 4), SENTINEL, dtype=torch.float32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((out == SENTINEL).all()) and bool((carry == SENTINEL).all())

    fb = _engine(dspsr_amd, ctx, case)
    one = dspsr_amd.FilterbankEngine(ctx).setup(case.C, case.M, case.nfilt[0], case.nfilt[1], 1, 1, True, cc.kernel_of(case), max_parts=case.maxp)
    try:
        rng = np.random.default_rng(5)
        raw = torch.from_numpy(cc.raw_block(rng, npart * fb.nsamp_step + fb.nsamp_overlap, True)).cuda()
        cs, ps = out.stride(0), out.stride(1)
        # one polarisation
        rc, msg, cnt, no = _call(dspsr_amd, one, raw, dspsr_amd.COHERENCE, sf, out, cs, ps, carry, 2, npart)
        assert rc != 0 and "Coherence needs two polarisations (npol=1)" in msg and (cnt, no) == (2, 0xABCDEF) and untouched()
        assert not one.search_fuses(dspsr_amd.COHERENCE, sf) and not one.search_fuses(dspsr_amd.PPQQ, sf)
        # Stokes
        rc, msg, cnt, no = _call(dspsr_amd, fb, raw, dspsr_amd.STOKES, sf, out, cs, ps, carry, 2, npart)
        assert rc != 0 and "Stokes" in msg and (cnt, no) == (2, 0xABCDEF) and untouched()
        # carry_count >= tscrunch
        rc, msg, cnt, no = _call(dspsr_amd, fb, raw, dspsr_amd.COHERENCE, sf, out, cs, ps, carry, sf, npart)
        assert rc != 0 and "carry_count=%d must be < tscrunch=%d" % (sf, sf) in msg and (cnt, no) == (sf, 0xABCDEF) and untouched()
        # four rows per channel that overlap: a channel stride one float short; a row stride one float short; a channel stride of two rows
        for bad_cs, bad_ps in ((3 * ps + nout - 1, ps), (cs, nout - 1), (2 * nout, nout)):
            rc, msg, cnt, no = _call(dspsr_amd, fb, raw, dspsr_amd.COHERENCE, sf, out, bad_cs, bad_ps, carry, 0, npart)
            assert rc != 0 and "output rows of %d floats overlap" % nout in msg and (cnt, no) == (0, 0xABCDEF) and untouched(), (bad_cs, bad_ps)
        # ... which two rows per channel (PPQQ) fit
        rc, msg, cnt, no = _call(dspsr_amd, fb, raw, dspsr_amd.PPQQ, sf, out, 2 * nout, nout, carry, 0, npart)
        assert rc == 0 and (cnt, no) == (npart * case.nkeep % sf, nout)
        # the Python wrapper: four rows and [nchan][4] carries
        with pytest.raises(dspsr_amd.DspsrAmdError, match="out needs 4 polarisation rows per channel"):
            fb.perform_search(out[:, :2], carry, 0, npart, sf, dspsr_amd.COHERENCE, raw=raw, layout=dspsr_amd.RAW_GENERIC, scale=cc.SCALE)
    finally:
        fb.close()
        one.close()


# ---- the drivers ------------------------------------------------------------------------------------------------------------------

def test_digifil_d4_fused_equals_unfused_bytes(gpu):
    """LoadToFilCoherent -F 64:D -x 1024 -D 2 -t 16 -d 4 -b 8 over three blocks: with fuse_coherence every block is one
    perform_search (nkeep 595: 16 * 39 = 624 <= 1024, the tile fits), and the packed bytes are the unfused chain's"""
    dspsr_amd, ctx = gpu
    from dspsr_amd import pipeline
    info = pipeline.InputInfo(centre_frequency=1382.0, bandwidth=-400.0, nchan=1, npol=2, ndim=1, tsamp_us=0.00125, machine="DADA")
    kw = dict(nchan=64, freq_res=1024, dispersion_measure=2.0, tscrunch=16, npol=4, nbit=8, rescale_seconds=2e-4, parts_per_block=6, max_parts=4)
    stream = torch.cuda.current_stream().cuda_stream
    a = pipeline.LoadToFilCoherent(pipeline.SearchConfig(fuse_coherence=True, **kw), info, device=0, stream=stream)
    b = pipeline.LoadToFilCoherent(pipeline.SearchConfig(**kw), info, device=0, stream=stream)
    try:
        assert a.nkeep == 595 and cc.fits(64, 1024, a.nkeep, 16)
        assert a.fused and not b.fused and a.fb.search_fuses(dspsr_amd.COHERENCE, 16)
        rng = np.random.default_rng(61)
        step, nblk = 6 * a.nsamp_step, 6 * a.nsamp_step + a.nsamp_overlap
        data = np.clip(np.rint(rng.standard_normal((3 * step + a.nsamp_overlap) * 2) * 24.0), -128, 127).astype(np.int8)
        total = 0
        for blk in range(3):
            raw = torch.from_numpy(data[blk * step * 2:(blk * step + nblk) * 2].copy()).cuda()
            pa, pb = a.process_block(raw), b.process_block(raw)
            assert pa.dtype == pb.dtype and torch.equal(pa, pb), blk
            total += pa.numel()
        assert total > 0
    finally:
        a.close()
        b.close()


def test_digifits_p4_fused_equals_unfused_blocks(gpu):
    """LoadToFITS -p 4 on the input of test_gpu_fits_pipeline's "real" shape.  That shape itself (-D 1 -x 256: 2044 of 2048 samples
    kept, tscrunch 16) does not fit -- 16 * 129 = 2064 > 2048 -- so this is the nearest one that does, the same 2048-point transform
    and factor with a response that discards more: -D 10 -x 32, 2014 samples kept, 16 * 127 = 2032 <= 2048 (asserted from the
    restatement).  The blocks -- DAT_OFFS, DAT_SCL, DATA -- are identical, for a stream cut into unequal calls."""
    dspsr_amd, ctx = gpu
    from dspsr_amd import pipeline
    info = pipeline.InputInfo(centre_frequency=1400.0, bandwidth=-16.0, nchan=1, npol=2, ndim=1, tsamp_us=1.0 / 32.0, machine="DADA")
    kw = dict(nchan=16, convolve=True, freq_res=32, dispersion_measure=10.0, coherent_dedisp=True, tsamp=16e-6, parts_per_block=14, npol=4, nbit=4,
              nsblk=128)
    stream = torch.cuda.current_stream().cuda_stream
    a = pipeline.LoadToFITS(pipeline.FitsConfig(fuse_coherence=True, **kw), info, device=0, stream=stream)
    b = pipeline.LoadToFITS(pipeline.FitsConfig(**kw), info, device=0, stream=stream)
    try:
        fa, fb_ = a.front, b.front
        assert a.tres_factor == 16 and fa.nkeep == 2014 and fa.response.ndat == 2048
        assert not cc.fits(16, 2048, 2044, 16) and cc.fits(16, 2048, fa.nkeep, 16)
        assert fa.fused and not fb_.fused and fa.fb.search_fuses(dspsr_amd.COHERENCE, 16)
        rng = np.random.default_rng(62)
        parts = (1, 5, 2, 6)
        data = np.clip(np.rint(rng.normal(0.0, 24.0, (sum(parts) * fa.nsamp_step + fa.nsamp_overlap) * 2)), -128, 127).astype(np.int8)
        s0, nblocks = 0, 0
        for n in parts:
            raw = torch.from_numpy(data[s0 * 2:(s0 + n * fa.nsamp_step + fa.nsamp_overlap) * 2].copy()).cuda()
            da, db = a.process_block(raw, n), b.process_block(raw, n)
            assert len(da) == len(db)
            for ba, bb in zip(da, db):
                assert len(ba) == len(bb) == 3
                for ta, tb in zip(ba, bb):
                    assert ta.dtype == tb.dtype and torch.equal(ta, tb)
            nblocks += len(da)
            s0 += n * fa.nsamp_step
        assert nblocks >= 3
    finally:
        a.close()
        b.close()
